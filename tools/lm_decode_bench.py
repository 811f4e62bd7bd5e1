"""Speed of the language-model chain (lm_decode.hip) at the configuration of PaddleOCR-VL's text decoder (ERNIE-4.5-0.3B: D 1024, 18 layers, 16 heads,
2 kv heads, head size 128, F 3072, vocabulary 103424, untied lm-head), random weights.

Per (weights dtype, sequences n, cache length C): a prompt of C positions per sequence is prefilled and 1 + K tokens are generated with the profiler filtered to
the decode steps' classes; their event intervals are K decode steps at cache length C .. C + K.  `kernel_us` is that sum per step (kernel
time, no gaps; the prefill line also has the host wall clock of the whole call with the profiler off).  Beside them the floor: oar_lm_cost bytes / 6.29 TB/s
(the measured copy rate of the part) + (5 L + 2) kernel boundaries of 1.2 us (the measured gap between a decode layer's short GEMV launches); and the same step in
torch-ROCm eager, f32 and bf16, as the only outside yardstick.  `--processes 3` runs three fresh processes and prints medians with min .. max.

`--prefill-mode rows|gemm|both` chooses how the prefill lines prefill; `both` measures the two arms in the same process, one after the other, for every
length of `--prefill`.  A GEMM line sums the `lm_gemm_*` classes plus the handover step (the decode classes of a call with one new token), and carries the floor of
oar_lm_prefill_cost: flops / 157.3 TFLOP/s (the exact-f32 matrix peak) or bytes / 6.29 TB/s, whichever is larger.  `--no-decode` leaves the decode lines out.

`--attention serial|split|both` chooses the attention of the decode lines; `--split-keys N [N ...]` the spans of the split arm (0: the library's default).
With `both` the arms alternate inside one process: for every (weights, cache, sequences) the serial line, then one split line per N, on the same model and prompt.
A split line carries `attention: "split"` and `split_keys`, and its classes are lm_rows / lm_attn_split / lm_attn_merge / lm_head / lm_combine.  `--decode-prefill gemm`
fills the cache of the decode lines through the GEMM prefill (much faster at long caches; its handover step is one more decode step of the same classes and is counted).
`--stop-at-eos T` adds two lines: the wall clock of a call with max_new_tokens 4096 whose sequences all end at token T, with stop_at_eos off and on.
`--queue N` measures queued generation instead of the lines above: N prompts of mixed lengths (16 .. 512), bf16 weights, prefill "gemm", split attention,
`--queue-new` tokens asked for.  Random weights would never emit one token in two sequences, so the lengths are made to spread: the lm-head row of the eos token is
scaled by `--queue-eos-gain`, and every step is fed a random forced token instead of its argmax (both arms alike), so that eos wins at about two percent of the steps,
independently from step to step; a first call prints the histogram of the lengths.  Two arms alternate in the process: "groups"
(generate in groups of 16 with stop_at_eos, summed over the groups) and "refill" (schedule="refill", slots 16); each prints wall clock, steps, rows, dead rows and
tokens per second; then the same pair without eos (even lengths: refill should tie), and the kernel time of the refill arm's GEMM phases, during which the decoding
slots wait.  `--lib PATH` loads another build of the library (build.py's OAR_LM_QUEUE_LAG), `--lag S/L` labels its lines.
`--logits-processors R N` measures the decode step with repetition_penalty R and no_repeat_ngram_size N instead of the lines above: for every
(weights, cache, sequences) the plain arm and the processors arm alternate on one model and prompt (the prompt's ids are the history); a line carries the step's
kernel time, its classes and, for the processors arm, the `lm_select` class alone.  `--parent-lib PATH` adds, after every process, a fresh process that loads the
library built from the parent commit and measures the plain arm with it (arm "parent").  Defaults of this mode: --seqs 1 16 --cache 256.

Usage: python tools/lm_decode_bench.py [--processes 3] [--seqs 1 4 16] [--cache 256 2048] [--steps 8] [--prefill 64 256 1024 4096] [--prefill-mode both] [--no-decode] [--no-torch]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api, vl                      # noqa: E402

CFG = dict(hidden_size=1024, num_hidden_layers=18, num_attention_heads=16, num_key_value_heads=2, head_dim=128, intermediate_size=3072, vocab_size=103424,
           rms_norm_eps=1e-5, rope_theta=500000.0, mrope_section=[16, 24, 24], qkv_bias=False, tie_word_embeddings=False)
COPY_RATE, BOUNDARY_US, F32_MATRIX_PEAK = 6.29e12, 1.2, 157.3e12
CLASSES = ("lm_rows", "lm_attn", "lm_head", "lm_combine")
SPLIT_CLASSES = ("lm_rows", "lm_attn_split", "lm_attn_merge", "lm_head", "lm_combine")
PREFILL_CLASSES = ("lm_prefill_rows", "lm_prefill_attn", "lm_prefill_head", "lm_prefill_combine")   # steps with prompt positions that give no token
GEMM_CLASSES = ("lm_gemm_linear", "lm_gemm_attn")                                                    # the GEMM phase; its handover step runs under CLASSES


def weights(cfg, rng):
    D, Hd, Kd, F, V = cfg.hidden_size, cfg.num_attention_heads * cfg.head_dim, cfg.num_key_value_heads * cfg.head_dim, cfg.intermediate_size, cfg.vocab_size
    mat = lambda n, k: (rng.standard_normal((n, k), dtype=np.float32) / np.float32(np.sqrt(k)))   # noqa: E731
    w = {"model.embed_tokens.weight": mat(V, D), "lm_head.weight": mat(V, D), "model.norm.weight": np.ones(D, np.float32)}
    for l in range(cfg.num_hidden_layers):
        p = f"model.layers.{l}."
        w.update({p + "input_layernorm.weight": np.ones(D, np.float32), p + "post_attention_layernorm.weight": np.ones(D, np.float32),
                  p + "self_attn.q_proj.weight": mat(Hd, D), p + "self_attn.k_proj.weight": mat(Kd, D), p + "self_attn.v_proj.weight": mat(Kd, D),
                  p + "self_attn.o_proj.weight": mat(D, Hd), p + "mlp.gate_proj.weight": mat(F, D), p + "mlp.up_proj.weight": mat(F, D), p + "mlp.down_proj.weight": mat(D, F)})
    return w


def bf16_bits(a):
    u = a.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def profiled(lm, ids, max_new, classes, prefill="rows", **kw):
    api.prof_reset()
    api.prof_filter(",".join(classes))                # (only these are bracketed with events: a long prefill in front of the decode steps runs as it is)
    api.prof_enable(True)
    try:
        lm.generate(input_ids=ids, max_new_tokens=max_new, prefill=prefill, **kw)
        return {e["name"]: e["total_ms"] * 1e3 for e in api.prof_snapshot() if e["name"].startswith("lm_")}
    finally:
        api.prof_enable(False)
        api.prof_filter("")


def wall(lm, ids, max_new, prefill="rows", **kw):
    t = time.perf_counter()
    lm.generate(input_ids=ids, max_new_tokens=max_new, prefill=prefill, **kw)
    return (time.perf_counter() - t) * 1e6


def torch_step_us(cfg, n, C, dtype, steps):
    """One decode step of the same model in torch eager on the GPU: the ops a straightforward implementation issues, a preallocated cache of C positions."""
    import torch
    dev = "cuda"
    D, H, KVH, dh, F, V, L = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, device=dev, generator=g) / s[-1] ** 0.5).to(dtype)   # noqa: E731
    layers = [dict(q=rnd(H * dh, D), k=rnd(KVH * dh, D), v=rnd(KVH * dh, D), o=rnd(D, H * dh), g=rnd(F, D), u=rnd(F, D), d=rnd(D, F), n1=torch.ones(D, device=dev, dtype=dtype),
                   n2=torch.ones(D, device=dev, dtype=dtype), K=rnd(n, KVH, C + steps, dh), V=rnd(n, KVH, C + steps, dh)) for _ in range(L)]
    emb, head, nf = rnd(V, D), rnd(V, D), torch.ones(D, device=dev, dtype=dtype)
    cos, sin = torch.randn(n, 1, 1, dh, device=dev).to(dtype), torch.randn(n, 1, 1, dh, device=dev).to(dtype)
    rms = lambda x, w: x * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5).to(dtype) * w   # noqa: E731
    rot = lambda x: torch.cat([-x[..., dh // 2:], x[..., :dh // 2]], -1)   # noqa: E731
    tok = torch.zeros(n, dtype=torch.long, device=dev)

    def step(pos):
        x = emb[tok]
        for W in layers:
            xn = rms(x, W["n1"])
            q, k, v = (xn @ W["q"].T).view(n, H, 1, dh), (xn @ W["k"].T).view(n, KVH, 1, dh), (xn @ W["v"].T).view(n, KVH, 1, dh)
            q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
            W["K"][:, :, pos:pos + 1], W["V"][:, :, pos:pos + 1] = k, v
            Kc, Vc = W["K"][:, :, :pos + 1].repeat_interleave(H // KVH, 1), W["V"][:, :, :pos + 1].repeat_interleave(H // KVH, 1)
            a = torch.softmax((q @ Kc.transpose(-1, -2)).float() * dh ** -0.5, -1).to(dtype)
            x = x + (a @ Vc).reshape(n, H * dh) @ W["o"].T
            xn = rms(x, W["n2"])
            x = x + (torch.nn.functional.silu(xn @ W["g"].T) * (xn @ W["u"].T)) @ W["d"].T
        return torch.argmax(rms(x, nf) @ head.T, -1)

    with torch.no_grad():
        for i in range(3):
            tok = step(C + i)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(steps):
            tok = step(C + i)
        b.record()
        torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def child(a):
    cfg = vl.CausalLMConfig(max_positions=max(max(a.cache), max(a.prefill), 4096 if a.stop_at_eos else 0) + a.steps + 2, max_sequences=max(a.seqs), **CFG)
    arms = ([("serial", None)] if a.attention in ("serial", "both") else []) + ([("split", sk) for sk in a.split_keys] if a.attention in ("split", "both") else [])
    rng = np.random.default_rng(0)
    w32 = weights(cfg, rng)
    for dtype in a.dtypes:
        w = w32 if dtype == "f32" else {k: (bf16_bits(v) if v.ndim == 2 else v) for k, v in w32.items()}
        with vl.CausalLM.from_state_dict(cfg, w) as lm:
            del w
            lm.generate(input_ids=[1, 2, 3], max_new_tokens=3)                      # warm-up: code objects, LDS opt-in
            if a.attention != "serial":
                lm.generate(input_ids=[1, 2, 3], max_new_tokens=3, decode_attention="split")
            if a.decode_prefill == "gemm":
                lm.generate(input_ids=list(range(70)), max_new_tokens=1, prefill="gemm")
            measured = a.steps + (1 if a.decode_prefill == "gemm" else 0)               # (the GEMM prefill's handover step runs under the decode classes)
            for C in ([] if a.no_decode else a.cache):
                for n in a.seqs:
                    ids = [rng.integers(0, cfg.vocab_size, C).astype(np.int32) for _ in range(n)]
                    for arm, sk in arms:                                                # the arms alternate: the same model, the same prompt, one after the other
                        classes = CLASSES if arm == "serial" else SPLIT_CLASSES
                        pk = profiled(lm, ids, 1 + a.steps, classes, prefill=a.decode_prefill, decode_attention=arm, split_keys=sk or None)
                        per = {c: pk.get(c, 0.0) / measured for c in classes}
                        flops, nbytes, launches = lm.cost(n, C + a.steps // 2)
                        line = {"kind": "decode", "weights": dtype, "seqs": n, "cache": C, "kernel_us": sum(per.values()), "by_class_us": per,
                                "floor_us": nbytes / COPY_RATE * 1e6 + launches * BOUNDARY_US, "cost_bytes": nbytes, "launches": launches}
                        if a.attention != "serial":
                            line.update(attention=arm, split_keys=sk)
                        print(json.dumps(line), flush=True)
            if a.stop_at_eos:
                # sequences that all end at token T: eos is whatever the model emits there (random weights: found by a first call), the prompts are short
                T = a.stop_at_eos
                ids = [rng.integers(0, cfg.vocab_size, 4).astype(np.int32)]
                eos = int(lm.generate(input_ids=ids, max_new_tokens=T + 1).tokens[0][T])
                for flag in (False, True):
                    lm.generate(input_ids=ids, max_new_tokens=8, eos_token_id=eos, stop_at_eos=flag)
                    us = wall(lm, ids, 4096, eos_token_id=eos, stop_at_eos=flag)
                    limit, enq = lm.decode_stats()
                    print(json.dumps({"kind": "stop_at_eos_" + ("on" if flag else "off"), "weights": dtype, "wall_us": us, "steps_limit": limit, "steps_enqueued": enq}), flush=True)
            lm.set_decode()
            for T in a.prefill:
                ids = rng.integers(0, cfg.vocab_size, T).astype(np.int32)
                if a.prefill_mode in ("rows", "both"):
                    p = profiled(lm, ids, 1, PREFILL_CLASSES)
                    print(json.dumps({"kind": "prefill", "weights": dtype, "positions": T, "kernel_us": sum(p.get(c, 0.0) for c in PREFILL_CLASSES), "wall_us": wall(lm, ids, 1),
                                      "by_class_us": {c.replace("_prefill", ""): p.get(c, 0.0) for c in PREFILL_CLASSES}}), flush=True)
                if a.prefill_mode in ("gemm", "both"):
                    lm.generate(input_ids=ids[:70], max_new_tokens=1, prefill="gemm")        # warm-up of this arm's code objects
                    for arm, sk in arms:
                        classes = GEMM_CLASSES + (CLASSES if arm == "serial" else SPLIT_CLASSES)
                        kw = dict(decode_attention=arm, split_keys=sk or None)
                        p = profiled(lm, ids, 1, classes, prefill="gemm", **kw)
                        flops, nbytes, launches = lm.prefill_cost([T])
                        line = {"kind": "prefill_gemm", "weights": dtype, "positions": T, "kernel_us": sum(p.get(c, 0.0) for c in classes),
                                "wall_us": wall(lm, ids, 1, "gemm", **kw), "by_class_us": {c: p.get(c, 0.0) for c in classes},
                                "floor_us": max(flops / F32_MATRIX_PEAK, nbytes / COPY_RATE) * 1e6, "cost_flops": flops, "cost_bytes": nbytes, "launches": launches}
                        if a.attention != "serial":
                            line.update(attention=arm, split_keys=sk)
                        print(json.dumps(line), flush=True)


def queue_child(a):
    """--queue: the groups schedule against the refill schedule on one list of prompts."""
    if a.lib:
        api.LIB_PATH = Path(a.lib).resolve()
    N, MN, eos = a.queue, a.queue_new, 7
    cfg = vl.CausalLMConfig(max_positions=512 + MN + 2, max_sequences=16, **CFG)
    rng = np.random.default_rng(0)
    w = weights(cfg, rng)
    w["lm_head.weight"][eos] *= np.float32(a.queue_eos_gain)
    w = {k: (bf16_bits(v) if v.ndim == 2 else v) for k, v in w.items()}
    ids = [rng.integers(0, cfg.vocab_size, int(T)).astype(np.int32) for T in rng.integers(16, 513, N)]
    forced = [row for row in rng.integers(0, cfg.vocab_size, (N, MN)).astype(np.int32)]
    mode = dict(prefill="gemm", decode_attention="split")

    def groups(lm, eos_id):
        t = time.perf_counter()
        steps = rows = live = 0
        for i in range(0, N, 16):
            out = lm.generate(input_ids=ids[i:i + 16], max_new_tokens=MN, eos_token_id=eos_id, stop_at_eos=True, forced_tokens=forced[i:i + 16], **mode)
            enq = lm.decode_stats()[1]
            steps, rows, live = steps + enq, rows + enq * len(out.counts), live + int(out.counts.sum())
        return dict(wall_us=(time.perf_counter() - t) * 1e6, steps=steps, rows=rows, dead_rows=rows - live, tokens=live)

    def refill(lm, eos_id):
        t = time.perf_counter()
        out = lm.generate(input_ids=ids, max_new_tokens=MN, eos_token_id=eos_id, schedule="refill", forced_tokens=forced, **mode)
        us = (time.perf_counter() - t) * 1e6
        q = lm.queue_stats()
        return dict(wall_us=us, steps=q["steps"], rows=q["rows"], dead_rows=q["dead_rows"], tokens=int(out.counts.sum()), gemm_phases=q["gemm_phases"],
                    max_dead_rows=q["max_dead_rows"])

    with vl.CausalLM.from_state_dict(cfg, w) as lm:
        del w
        free = lm.generate(input_ids=ids, max_new_tokens=MN, eos_token_id=eos, schedule="refill", forced_tokens=forced, **mode)   # warm-up of the code objects, and the lengths
        hist = np.bincount(np.minimum(free.counts - 1, MN - 1) * 8 // MN, minlength=8).tolist()
        print(json.dumps({"kind": "queue_lengths", "weights": "bf16", "n": N, "max_new": MN, "eighths_of_max_new": hist, "at_limit": int((free.counts == MN).sum()),
                          "mean": float(free.counts.mean())}), flush=True)
        groups(lm, eos)
        for workload, eos_id in (("uneven", eos), ("even", None)):
            for rep in range(a.queue_reps if eos_id is not None else 1):                                             # the arms alternate
                for arm, fn in (("groups", groups), ("refill", refill)):
                    r = fn(lm, eos_id)
                    r.update(kind="queue", weights="bf16", arm=arm, workload=workload, lag=a.lag, rep=rep, tokens_per_s=r["tokens"] / r["wall_us"] * 1e6)
                    print(json.dumps(r), flush=True)
        api.prof_reset()
        api.prof_filter(",".join(GEMM_CLASSES))
        api.prof_enable(True)
        try:
            lm.generate(input_ids=ids, max_new_tokens=MN, eos_token_id=eos, schedule="refill", forced_tokens=forced, **mode)
            p = {e["name"]: (e["total_ms"] * 1e3, e["launches"]) for e in api.prof_snapshot() if e["name"] in GEMM_CLASSES}
        finally:
            api.prof_enable(False)
            api.prof_filter("")
        q = lm.queue_stats()
        print(json.dumps({"kind": "queue_gemm_phases", "weights": "bf16", "lag": a.lag, "phases": q["gemm_phases"], "admissions": q["admissions"],
                          "kernel_us": sum(v[0] for v in p.values()), "launches": sum(v[1] for v in p.values()),
                          "kernel_us_per_phase": sum(v[0] for v in p.values()) / max(q["gemm_phases"], 1)}), flush=True)


def logits_child(a):
    """--logits-processors: the plain step and the step with processors, alternating; with --lib (another build, which may lack the entry): the plain arm alone."""
    if a.lib:
        api.LIB_PATH = Path(a.lib).resolve()
    r, n = float(a.logits_processors[0]), int(a.logits_processors[1])
    cfg = vl.CausalLMConfig(max_positions=max(a.cache) + a.steps + 2, max_sequences=max(a.seqs), **CFG)
    rng = np.random.default_rng(0)
    w32 = weights(cfg, rng)
    arms = [("parent", {})] if a.lib else [("plain", {}), ("processors", dict(repetition_penalty=r, no_repeat_ngram_size=n))]
    for dtype in a.dtypes:
        w = w32 if dtype == "f32" else {k: (bf16_bits(v) if v.ndim == 2 else v) for k, v in w32.items()}
        with vl.CausalLM.from_state_dict(cfg, w) as lm:
            del w
            for _, kw in arms:
                lm.generate(input_ids=[1, 2, 3], max_new_tokens=3, **kw)                # warm-up: code objects, LDS opt-in, the processors' workspace
            for C in a.cache:
                for ns in a.seqs:
                    ids = [rng.integers(0, cfg.vocab_size, C).astype(np.int32) for _ in range(ns)]
                    for rep_ in range(2):                                                 # the arms alternate, twice; the second round is reported
                        for arm, kw in arms:
                            classes = CLASSES + (("lm_select",) if kw else ())
                            pk = profiled(lm, ids, 1 + a.steps, classes, **kw)
                            per = {c: pk.get(c, 0.0) / a.steps for c in classes}
                            if rep_:
                                print(json.dumps({"kind": "decode_logits", "arm": arm, "weights": dtype, "seqs": ns, "cache": C, "kernel_us": sum(per.values()), "by_class_us": per,
                                                  "select_us": per.get("lm_select"), "repetition_penalty": r, "no_repeat_ngram_size": n}), flush=True)


def logits_main(a):
    if a.child or a.processes <= 1 and not a.parent_lib:
        logits_child(a)
        return
    rows = {}
    argv = [x for x in sys.argv[1:]]
    for _ in range(max(a.processes, 1)):                                             # fresh processes, one after the other; the parent's build right behind this one
        for extra in [[]] + ([["--lib", a.parent_lib]] if a.parent_lib else []):
            p = subprocess.Popen([sys.executable, __file__, "--child"] + argv + extra, stdout=subprocess.PIPE, text=True)
            for line in p.stdout:
                sys.stderr.write(line)
                sys.stderr.flush()
                if line.startswith("{"):
                    d = json.loads(line)
                    rows.setdefault((d["arm"], d["weights"], d["seqs"], d["cache"]), []).append(d)
            if p.wait() != 0:
                sys.exit(p.returncode)
    stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}   # noqa: E731
    for (arm, wt, ns, C), ds in rows.items():
        out = {"kind": "decode_logits", "arm": arm, "weights": wt, "seqs": ns, "cache": C, "processes": len(ds), "kernel_us": stat([d["kernel_us"] for d in ds]),
               "by_class_us": {c: round(float(np.median([d["by_class_us"][c] for d in ds])), 1) for c in ds[0]["by_class_us"]}}
        if ds[0]["select_us"] is not None:
            out["select_us"] = stat([d["select_us"] for d in ds])
        print(json.dumps(out), flush=True)


def torch_child(a):
    """In a process of its own: torch brings its own HIP runtime."""
    import torch
    cfg = vl.CausalLMConfig(max_positions=4096, **CFG)
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        for C in a.cache:
            for n in a.seqs:
                print(json.dumps({"kind": "torch_eager", "weights": name, "seqs": n, "cache": C, "step_us": torch_step_us(cfg, n, C, dt, a.steps)}), flush=True)


def queue_main(a):
    if a.child or a.processes <= 1:
        queue_child(a)
        return
    rows = {}
    for _ in range(a.processes):                                                     # fresh processes, one after the other
        r = subprocess.Popen([sys.executable, __file__, "--child"] + sys.argv[1:], stdout=subprocess.PIPE, text=True)
        for line in r.stdout:
            sys.stderr.write(line)
            sys.stderr.flush()
            if line.startswith("{"):
                d = json.loads(line)
                rows.setdefault((d["kind"], d.get("arm"), d.get("workload"), d.get("lag")), []).append(d)
        if r.wait() != 0:
            sys.exit(r.returncode)
    stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}   # noqa: E731
    for (kind, arm, workload, lag), ds in rows.items():
        out = {"kind": kind, "arm": arm, "workload": workload, "lag": lag, "samples": len(ds)}
        out.update({f: stat([d[f] for d in ds]) for f in ("wall_us", "tokens_per_s", "kernel_us", "kernel_us_per_phase") if f in ds[0]})
        out.update({f: ds[0][f] for f in ("steps", "rows", "dead_rows", "tokens", "gemm_phases", "max_dead_rows", "phases", "launches", "eighths_of_max_new", "at_limit", "mean")
                    if f in ds[0]})
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=1)
    ap.add_argument("--seqs", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--cache", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--prefill", type=int, nargs="+", default=[1024])
    ap.add_argument("--prefill-mode", choices=["rows", "gemm", "both"], default="rows")
    ap.add_argument("--attention", choices=["serial", "split", "both"], default="serial")
    ap.add_argument("--split-keys", type=int, nargs="+", default=[0])
    ap.add_argument("--decode-prefill", choices=["rows", "gemm"], default="rows")
    ap.add_argument("--stop-at-eos", type=int, default=0)
    ap.add_argument("--queue", type=int, default=0)
    ap.add_argument("--queue-new", type=int, default=128)
    ap.add_argument("--queue-eos-gain", type=float, default=3.3)
    ap.add_argument("--queue-reps", type=int, default=2)
    ap.add_argument("--lib", default="")
    ap.add_argument("--logits-processors", nargs=2, metavar=("R", "N"), default=None)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--lag", default="")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--torch-child", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        torch_child(a)
        return
    if a.queue:
        queue_main(a)
        return
    if a.logits_processors:
        if "--seqs" not in sys.argv:
            a.seqs = [1, 16]
        if "--cache" not in sys.argv:
            a.cache = [256]
        logits_main(a)
        return
    if a.child or a.processes <= 1:
        child(a)
        if not a.no_torch and not a.child:
            subprocess.run([sys.executable, __file__, "--torch-child"] + sys.argv[1:], check=True)
        return
    rows = {}
    argv = [x for x in sys.argv[1:]]
    runs = [["--child"]] * a.processes + ([] if a.no_torch else [["--torch-child"]] * a.processes)
    for mode in runs:                                                                # fresh processes, one after the other
        r = subprocess.Popen([sys.executable, __file__] + mode + argv, stdout=subprocess.PIPE, text=True)
        for line in r.stdout:
            sys.stderr.write(line)                                                   # (progress: a process takes minutes)
            sys.stderr.flush()
            if line.startswith("{"):
                d = json.loads(line)
                key = (d["kind"], d["weights"], d.get("seqs"), d.get("cache", d.get("positions")), d.get("attention"), d.get("split_keys"))
                rows.setdefault(key, []).append(d)
        if r.wait() != 0:
            sys.exit(r.returncode)
    stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}   # noqa: E731
    for key, ds in rows.items():
        out = {"kind": key[0], "weights": key[1], "seqs": key[2], "cache_or_positions": key[3], "processes": len(ds)}
        if key[4] is not None:
            out.update(attention=key[4], split_keys=key[5])
        if "steps_enqueued" in ds[0]:
            out.update(steps_limit=ds[0]["steps_limit"], steps_enqueued=ds[0]["steps_enqueued"])
        for f in ("kernel_us", "wall_us", "step_us"):
            if f in ds[0]:
                out[f] = stat([d[f] for d in ds])
        if "by_class_us" in ds[0]:
            out["by_class_us"] = {c: round(float(np.median([d["by_class_us"][c] for d in ds])), 1) for c in ds[0]["by_class_us"]}
        if "floor_us" in ds[0]:
            out["floor_us"] = round(ds[0]["floor_us"], 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
