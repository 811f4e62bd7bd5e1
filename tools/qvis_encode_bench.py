"""Speed of the Qwen2-VL and Qwen2.5-VL vision towers (qvis_host.cc, qvis_misc.hip) at the configuration the two towers are understood to have -- no
checkpoint has been seen here --: depth 32, width 1280, 16 heads (head size 80), patch 14, temporal 2, merge 2; qwen2: MLP 5120 with quick_gelu, out 1536; qwen2_5:
gated MLP 3420 with silu, out 2048, window 112 (64-patch windows), full attention at blocks 7, 15, 23 and 31; and `qwen2_5_full`, the same model with every block
made full-attention, which shows what the windows save.  Random weights (one block's matrices serve every block: the library uploads each block's own copy), one
image per call at grids 36 x 36 (1296 patches) and 72 x 70 (5040).

Per tower and grid: the kernel time of one `encode` by profiler class (event intervals, no gaps), the host wall clock of the call with the profiler off, and the
floor from oar_qvis_cost: flops / 157.3 TFLOP/s (the f32 matrix peak) and bytes / 6.29 TB/s (the measured copy rate), whichever is larger.  As the outside yardstick
torch-ROCm runs the same layer stacks (f32, scaled_dot_product_attention per segment, the rotation as element-wise ops) in a process of its own.  `--processes 3`
runs three fresh processes of each and prints medians with min .. max.  No number here is a pass criterion.

Usage: python tools/qvis_encode_bench.py [--processes 3] [--grids 36x36 72x70] [--reps 3] [--layers 32] [--towers qwen2 qwen2_5 qwen2_5_full] [--no-torch]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api, vl                      # noqa: E402
from oar_ocr_amd.synth.qwen_vision_reference import window_plan   # noqa: E402

COMMON = dict(embed_dim=1280, num_heads=16, patch_size=14, temporal_patch_size=2, spatial_merge_size=2)
TOWERS = {"qwen2": dict(kind="qwen2", intermediate_size=5120, hidden_act="quick_gelu", out_hidden_size=1536),
          "qwen2_5": dict(kind="qwen2_5", intermediate_size=3420, hidden_act="silu", out_hidden_size=2048, window_size=112, fullatt_block_indexes=[7, 15, 23, 31]),
          "qwen2_5_full": dict(kind="qwen2_5", intermediate_size=3420, hidden_act="silu", out_hidden_size=2048, window_size=112, fullatt_block_indexes=None)}
F32_PEAK, COPY_RATE = 157.3e12, 6.29e12


def tower_cfg(name, layers, max_tokens):
    d = dict(TOWERS[name])
    full = d.pop("fullatt_block_indexes", [])
    if d["kind"] == "qwen2_5":
        d["fullatt_block_indexes"] = list(range(layers)) if full is None else [i for i in full if i < layers]
    return vl.QwenVisionConfig(depth=layers, max_tokens=max_tokens, max_images=1, **COMMON, **d)


def weights(cfg, rng):
    D, F, m2, OH, q5 = cfg.embed_dim, cfg.intermediate_size, cfg.spatial_merge_size ** 2, cfg.out_hidden_size, cfg.kind == "qwen2_5"
    mat = lambda n, k: (rng.standard_normal((n, k), dtype=np.float32) / np.float32(np.sqrt(k)))   # noqa: E731
    one, zero = lambda n: np.ones(n, np.float32), lambda n: np.zeros(n, np.float32)               # noqa: E731
    w = {"visual.patch_embed.proj.weight": mat(D, cfg.patch_dim), "visual.merger.ln_q.weight": one(D), "visual.merger.mlp.0.weight": mat(m2 * D, m2 * D),
         "visual.merger.mlp.0.bias": zero(m2 * D), "visual.merger.mlp.2.weight": mat(OH, m2 * D), "visual.merger.mlp.2.bias": zero(OH)}
    block = {"norm1.weight": one(D), "norm2.weight": one(D), "attn.qkv.weight": mat(3 * D, D), "attn.qkv.bias": zero(3 * D), "attn.proj.weight": mat(D, D), "attn.proj.bias": zero(D)}
    if q5:
        block.update({"mlp.gate_proj.weight": mat(F, D), "mlp.gate_proj.bias": zero(F), "mlp.up_proj.weight": mat(F, D), "mlp.up_proj.bias": zero(F),
                      "mlp.down_proj.weight": mat(D, F), "mlp.down_proj.bias": zero(D)})
    else:
        w["visual.merger.ln_q.bias"] = zero(D)
        block.update({"norm1.bias": zero(D), "norm2.bias": zero(D), "mlp.fc1.weight": mat(F, D), "mlp.fc1.bias": zero(F), "mlp.fc2.weight": mat(D, F), "mlp.fc2.bias": zero(D)})
    for i in range(cfg.depth):
        for k, v in block.items():
            w[f"visual.blocks.{i}.{k}"] = v
    return w


def grid_of(text):
    h, w = text.lower().split("x")
    return int(h), int(w)


def child(a):
    grids = [grid_of(g) for g in a.grids]
    for name in a.towers:
        cfg = tower_cfg(name, a.layers, max(h * w for h, w in grids))
        rng = np.random.default_rng(0)
        with vl.QwenVisionEncoder.from_state_dict(cfg, weights(cfg, rng)) as enc:
            for h, w in grids:
                px = rng.uniform(-1, 1, (h * w, cfg.patch_dim)).astype(np.float32)
                enc.encode(px, [(h, w)])                                                 # warm-up: code objects
                walls = []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    enc.encode(px, [(h, w)])
                    walls.append((time.perf_counter() - t) * 1e3)
                api.prof_reset()
                api.prof_enable(True)
                try:
                    enc.encode(px, [(h, w)])
                    by = {e["name"]: (e["total_ms"], e["launches"]) for e in api.prof_snapshot() if e["launches"]}
                finally:
                    api.prof_enable(False)
                flops, nbytes, launches = enc.cost([(h, w)])
                print(json.dumps({"kind": name, "grid": f"{h}x{w}", "patches": h * w, "kernel_ms": sum(v[0] for v in by.values()), "wall_ms": float(np.median(walls)),
                                  "by_class_ms": {k: v[0] for k, v in by.items()}, "launches_by_class": {k: v[1] for k, v in by.items()}, "launches": launches,
                                  "floor_ms": max(flops / F32_PEAK, nbytes / COPY_RATE) * 1e3, "cost_gflop": flops / 1e9, "cost_mb": nbytes / 1e6}), flush=True)


def torch_child(a):
    """In a process of its own: torch brings its own HIP runtime.  The layer stack only (no patch Linear, no merger), windows as a loop over segments of equal length."""
    import torch
    import torch.nn.functional as Fn
    dev, D, nh, L = "cuda", COMMON["embed_dim"], COMMON["num_heads"], a.layers
    dh = D // nh
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g) / s[-1] ** 0.5   # noqa: E731
    one, zero = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    rot = lambda x: torch.cat([-x[..., dh // 2:], x[..., :dh // 2]], -1)       # noqa: E731
    for name in a.towers:
        cfg = tower_cfg(name, L, 1 << 20)
        F, q5 = cfg.intermediate_size, cfg.kind == "qwen2_5"
        W = dict(qkv=rnd(3 * D, D), o=rnd(D, D), f1=rnd(2 * F if q5 else F, D), f2=rnd(D, F))
        for h, w in [grid_of(t) for t in a.grids]:
            T = h * w
            x0 = torch.randn(T, D, device=dev, generator=g)
            cos, sin = torch.randn(1, T, dh, device=dev, generator=g), torch.randn(1, T, dh, device=dev, generator=g)
            segs = window_plan([(h, w)], 2, 14, 112)[2] if q5 else []
            by_len = {}
            for s, n in segs:
                by_len.setdefault(n, []).append(s)
            groups = [(n, torch.tensor([list(range(s, s + n)) for s in ss], device=dev)) for n, ss in by_len.items()]   # windows of one length as one batched call

            def attend(q, k, v, full):
                if full:
                    return Fn.scaled_dot_product_attention(q[None], k[None], v[None])[0].transpose(0, 1).reshape(T, D)
                out = torch.empty(T, D, device=dev)
                for n, idx in groups:                                                  # q [nh, T, dh] -> [windows, nh, n, dh]
                    o = Fn.scaled_dot_product_attention(q[:, idx].transpose(0, 1), k[:, idx].transpose(0, 1), v[:, idx].transpose(0, 1))
                    out[idx.reshape(-1)] = o.transpose(1, 2).reshape(-1, D)
                return out

            def norm(x):
                return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * one if q5 else Fn.layer_norm(x, (D,), one, zero, 1e-6)

            def run():
                x = x0
                for i in range(L):
                    q, k, v = (norm(x) @ W["qkv"].T).view(T, 3, nh, dh).permute(1, 2, 0, 3)
                    q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
                    x = x + attend(q, k, v, not q5 or i in cfg.fullatt_block_indexes) @ W["o"].T
                    y = norm(x) @ W["f1"].T
                    y = Fn.silu(y[:, :F]) * y[:, F:] if q5 else y * torch.sigmoid(1.702 * y)
                    x = x + y @ W["f2"].T
                return x
            with torch.no_grad():
                run()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    run()
                e1.record()
                torch.cuda.synchronize()
            print(json.dumps({"kind": "torch_f32_layers_" + name, "grid": f"{h}x{w}", "patches": T, "gpu_ms": e0.elapsed_time(e1) / a.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=1)
    ap.add_argument("--grids", nargs="+", default=["36x36", "72x70"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--towers", nargs="+", default=list(TOWERS), choices=list(TOWERS))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--torch-child", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        return torch_child(a)
    if a.child:
        return child(a)
    rows = {}
    runs = [["--child"]] * a.processes + ([] if a.no_torch else [["--torch-child"]] * a.processes)
    for mode in runs:                                                                # fresh processes, one after the other
        r = subprocess.Popen([sys.executable, __file__] + mode + sys.argv[1:], stdout=subprocess.PIPE, text=True)
        for line in r.stdout:
            sys.stderr.write(line)
            sys.stderr.flush()
            if line.startswith("{"):
                d = json.loads(line)
                rows.setdefault((d["kind"], d["grid"]), []).append(d)
        if r.wait() != 0:
            sys.exit(r.returncode)
    stat = lambda v: {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}   # noqa: E731
    for (kind, grid), ds in rows.items():
        out = {"kind": kind, "grid": grid, "patches": ds[0]["patches"], "processes": len(ds)}
        for f in ("kernel_ms", "wall_ms", "gpu_ms"):
            if f in ds[0]:
                out[f] = stat([d[f] for d in ds])
        if "by_class_ms" in ds[0]:
            out["by_class_ms"] = {c: round(float(np.median([d["by_class_ms"].get(c, 0.0) for d in ds])), 2) for c in ds[0]["by_class_ms"]}
            out["launches_by_class"] = ds[0]["launches_by_class"]
            out["floor_ms"], out["cost_gflop"], out["cost_mb"] = round(ds[0]["floor_ms"], 2), round(ds[0]["cost_gflop"], 1), round(ds[0]["cost_mb"], 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
