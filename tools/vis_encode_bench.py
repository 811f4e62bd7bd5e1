"""Speed of the vision encoder and projector (vis_attention.hip, vis_host.cc) at the SigLIP-so400m-shaped configuration PaddleOCR-VL is understood to
use (hidden 1152, 27 layers, 16 heads -- head size 72 --, MLP 4304, patch 14, a 27 x 27 position table, merge 2, text hidden 1024), random weights, one image per
call at grids 36 x 36 (1296 patches) and 72 x 70 (5040).

Per grid: the kernel time of one `encode` by profiler class (event intervals, no gaps), the host wall clock of the call with the profiler off, and the floor from
oar_vis_cost: flops / 157.3 TFLOP/s (the f32 matrix peak) and bytes / 6.29 TB/s (the measured copy rate), whichever is larger.  As the only outside yardstick, torch-ROCm runs
the same layer stack (f32, scaled_dot_product_attention, the rotation as element-wise ops) in a process of its own.  `--processes 3` runs three fresh processes of each and
prints medians with min .. max.  No number here is a pass criterion.

Usage: python tools/vis_encode_bench.py [--processes 3] [--grids 36x36 72x70] [--reps 3] [--layers 27] [--no-torch]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api, vl                      # noqa: E402

CFG = dict(hidden_size=1152, num_attention_heads=16, intermediate_size=4304, patch_size=14, text_hidden=1024, pos_grid=27, spatial_merge_size=2)
F32_PEAK, COPY_RATE = 157.3e12, 6.29e12


def weights(cfg, rng):
    D, F, p, m2, TH = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size, cfg.spatial_merge_size ** 2, cfg.text_hidden
    mat = lambda n, k: (rng.standard_normal((n, k), dtype=np.float32) / np.float32(np.sqrt(k)))   # noqa: E731
    one, zero = lambda n: np.ones(n, np.float32), lambda n: np.zeros(n, np.float32)               # noqa: E731
    vm = "visual.vision_model."
    w = {vm + "embeddings.patch_embedding.weight": mat(D, 3 * p * p).reshape(D, 3, p, p), vm + "embeddings.patch_embedding.bias": zero(D),
         vm + "embeddings.position_embedding.weight": rng.standard_normal((cfg.pos_grid ** 2, D), dtype=np.float32),
         vm + "post_layernorm.weight": one(D), vm + "post_layernorm.bias": zero(D), "mlp_AR.pre_norm.weight": one(D), "mlp_AR.pre_norm.bias": zero(D),
         "mlp_AR.linear_1.weight": mat(m2 * D, m2 * D), "mlp_AR.linear_1.bias": zero(m2 * D), "mlp_AR.linear_2.weight": mat(TH, m2 * D), "mlp_AR.linear_2.bias": zero(TH)}
    for i in range(cfg.num_hidden_layers):
        pre = vm + f"encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            w[pre + ln + ".weight"], w[pre + ln + ".bias"] = one(D), zero(D)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            w[pre + f"self_attn.{n}.weight"], w[pre + f"self_attn.{n}.bias"] = mat(D, D), zero(D)
        w[pre + "mlp.fc1.weight"], w[pre + "mlp.fc1.bias"], w[pre + "mlp.fc2.weight"], w[pre + "mlp.fc2.bias"] = mat(F, D), zero(F), mat(D, F), zero(D)
    return w


def grid_of(text):
    h, w = text.lower().split("x")
    return int(h), int(w)


def child(a):
    grids = [grid_of(g) for g in a.grids]
    cfg = vl.VisionConfig(num_hidden_layers=a.layers, max_tokens=max(h * w for h, w in grids), max_images=1, **CFG)
    rng = np.random.default_rng(0)
    with vl.VisionEncoder.from_state_dict(cfg, weights(cfg, rng)) as enc:
        for h, w in grids:
            px = rng.uniform(-1, 1, (h * w, 3 * cfg.patch_size ** 2)).astype(np.float32)
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
                by = {e["name"]: (e["total_ms"], e["launches"]) for e in api.prof_snapshot()}
            finally:
                api.prof_enable(False)
            flops, nbytes, launches = enc.cost([(h, w)])
            print(json.dumps({"kind": "encode", "grid": f"{h}x{w}", "patches": h * w, "kernel_ms": sum(v[0] for v in by.values()), "wall_ms": float(np.median(walls)),
                              "by_class_ms": {k: v[0] for k, v in by.items()}, "launches_by_class": {k: v[1] for k, v in by.items()}, "launches": launches,
                              "floor_ms": max(flops / F32_PEAK, nbytes / COPY_RATE) * 1e3, "cost_gflop": flops / 1e9, "cost_mb": nbytes / 1e6}), flush=True)


def torch_child(a):
    """In a process of its own: torch brings its own HIP runtime."""
    import torch
    import torch.nn.functional as Fn
    dev, D, nh, F, L = "cuda", CFG["hidden_size"], CFG["num_attention_heads"], CFG["intermediate_size"], a.layers
    dh = D // nh
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g) / s[-1] ** 0.5   # noqa: E731
    layers = [dict(qkv=rnd(3 * D, D), o=rnd(D, D), f1=rnd(F, D), f2=rnd(D, F)) for _ in range(L)]
    one, zero = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    rot = lambda x: torch.cat([-x[..., dh // 2:], x[..., :dh // 2]], -1)       # noqa: E731
    for h, w in [grid_of(t) for t in a.grids]:
        T = h * w
        x0 = torch.randn(T, D, device=dev, generator=g)
        cos, sin = torch.randn(1, T, dh, device=dev, generator=g), torch.randn(1, T, dh, device=dev, generator=g)

        def run():
            x = x0
            for W in layers:
                q, k, v = (Fn.layer_norm(x, (D,), one, zero, 1e-6) @ W["qkv"].T).view(T, 3, nh, dh).permute(1, 2, 0, 3)
                q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
                att = Fn.scaled_dot_product_attention(q[None], k[None], v[None])[0].transpose(0, 1).reshape(T, D)
                x = x + att @ W["o"].T
                x = x + Fn.gelu(Fn.layer_norm(x, (D,), one, zero, 1e-6) @ W["f1"].T, approximate="tanh") @ W["f2"].T
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
        print(json.dumps({"kind": "torch_f32_layers", "grid": f"{h}x{w}", "patches": T, "gpu_ms": e0.elapsed_time(e1) / a.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=1)
    ap.add_argument("--grids", nargs="+", default=["36x36", "72x70"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=27)
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
