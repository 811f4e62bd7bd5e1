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


def profiled(lm, ids, max_new, classes, prefill="rows"):
    api.prof_reset()
    api.prof_filter(",".join(classes))                # (only these are bracketed with events: a long prefill in front of the decode steps runs as it is)
    api.prof_enable(True)
    try:
        lm.generate(input_ids=ids, max_new_tokens=max_new, prefill=prefill)
        return {e["name"]: e["total_ms"] * 1e3 for e in api.prof_snapshot() if e["name"].startswith("lm_")}
    finally:
        api.prof_enable(False)
        api.prof_filter("")


def wall(lm, ids, max_new, prefill="rows"):
    t = time.perf_counter()
    lm.generate(input_ids=ids, max_new_tokens=max_new, prefill=prefill)
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
    cfg = vl.CausalLMConfig(max_positions=max(max(a.cache), max(a.prefill)) + a.steps + 2, max_sequences=max(a.seqs), **CFG)
    rng = np.random.default_rng(0)
    w32 = weights(cfg, rng)
    for dtype in a.dtypes:
        w = w32 if dtype == "f32" else {k: (bf16_bits(v) if v.ndim == 2 else v) for k, v in w32.items()}
        with vl.CausalLM.from_state_dict(cfg, w) as lm:
            del w
            lm.generate(input_ids=[1, 2, 3], max_new_tokens=3)                      # warm-up: code objects, LDS opt-in
            for C in ([] if a.no_decode else a.cache):
                for n in a.seqs:
                    ids = [rng.integers(0, cfg.vocab_size, C).astype(np.int32) for _ in range(n)]
                    pk = profiled(lm, ids, 1 + a.steps, CLASSES)
                    per = {c: pk.get(c, 0.0) / a.steps for c in CLASSES}
                    flops, nbytes, launches = lm.cost(n, C + a.steps // 2)
                    print(json.dumps({"kind": "decode", "weights": dtype, "seqs": n, "cache": C, "kernel_us": sum(per.values()), "by_class_us": per,
                                      "floor_us": nbytes / COPY_RATE * 1e6 + launches * BOUNDARY_US, "cost_bytes": nbytes, "launches": launches}), flush=True)
            for T in a.prefill:
                ids = rng.integers(0, cfg.vocab_size, T).astype(np.int32)
                if a.prefill_mode in ("rows", "both"):
                    p = profiled(lm, ids, 1, PREFILL_CLASSES)
                    print(json.dumps({"kind": "prefill", "weights": dtype, "positions": T, "kernel_us": sum(p.get(c, 0.0) for c in PREFILL_CLASSES), "wall_us": wall(lm, ids, 1),
                                      "by_class_us": {c.replace("_prefill", ""): p.get(c, 0.0) for c in PREFILL_CLASSES}}), flush=True)
                if a.prefill_mode in ("gemm", "both"):
                    lm.generate(input_ids=ids[:70], max_new_tokens=1, prefill="gemm")        # warm-up of this arm's code objects
                    p = profiled(lm, ids, 1, GEMM_CLASSES + CLASSES, prefill="gemm")
                    flops, nbytes, launches = lm.prefill_cost([T])
                    print(json.dumps({"kind": "prefill_gemm", "weights": dtype, "positions": T, "kernel_us": sum(p.get(c, 0.0) for c in GEMM_CLASSES + CLASSES),
                                      "wall_us": wall(lm, ids, 1, "gemm"), "by_class_us": {c: p.get(c, 0.0) for c in GEMM_CLASSES + CLASSES},
                                      "floor_us": max(flops / F32_MATRIX_PEAK, nbytes / COPY_RATE) * 1e6, "cost_flops": flops, "cost_bytes": nbytes, "launches": launches}), flush=True)


def torch_child(a):
    """In a process of its own: torch brings its own HIP runtime."""
    import torch
    cfg = vl.CausalLMConfig(max_positions=4096, **CFG)
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        for C in a.cache:
            for n in a.seqs:
                print(json.dumps({"kind": "torch_eager", "weights": name, "seqs": n, "cache": C, "step_us": torch_step_us(cfg, n, C, dt, a.steps)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=1)
    ap.add_argument("--seqs", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--cache", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--prefill", type=int, nargs="+", default=[1024])
    ap.add_argument("--prefill-mode", choices=["rows", "gemm", "both"], default="rows")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--torch-child", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        torch_child(a)
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
                key = (d["kind"], d["weights"], d.get("seqs"), d.get("cache", d.get("positions")))
                rows.setdefault(key, []).append(d)
        if r.wait() != 0:
            sys.exit(r.returncode)
    stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}   # noqa: E731
    for key, ds in rows.items():
        out = {"kind": key[0], "weights": key[1], "seqs": key[2], "cache_or_positions": key[3], "processes": len(ds)}
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
