"""Speed of the Vary / SAM ViT-shaped encoder with and without the RelPosAttention rewrite: event time per `infer` of
synth.models.build_vary_vit at the -L shape (768 x 768 input, 48 x 48 tokens, width 768, 12 heads of 64, depth 12, 14 x 14 windows, global blocks 2, 5, 8, 11).
OAR_FUSE_RELPOS_ATTENTION is read when the graph is loaded, so one process times one arm: run the arms in alternating processes on one saved graph and
compare their spread.  Prints one JSON line: the median and every repetition of the profiler's summed event time over all classes, the launches per infer,
those of class relpos_attention with that class's time and achieved TFLOP/s (4 N^2 dh + 2 (h + w) N dh flops per (image, key set, head), against the 155 TF
f32-matrix peak), the largest classes, and the wall time of an unprofiled infer.
Usage: OAR_FUSE_RELPOS_ATTENTION=0|1 python tools/vit_encoder_bench.py [--reps 5] [--batch 1] [--small] [--save graph.onnx | --load graph.onnx] [--lib other.so]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api                      # noqa: E402
from oar_ocr_amd.synth import models             # noqa: E402

L_SHAPE = dict(image_shape=(768, 768), C=768, nh=12, depth=12, ws=14, global_blocks=(2, 5, 8, 11), mlp_ratio=4, neck=256, D=512)
SMALL = dict(image_shape=(256, 256), C=128, nh=2, depth=4, ws=14, global_blocks=(1, 3), mlp_ratio=4, neck=64, D=128)   # a quick look, not the table's shape


def relpos_flops(cfg, batch):
    """the flops of the RelPosAttention launches of one infer: both products and the rel terms"""
    H, W = cfg["image_shape"][0] // 16, cfg["image_shape"][1] // 16
    dh, ws, total = cfg["C"] // cfg["nh"], cfg["ws"], 0.0
    for i in range(cfg["depth"]):
        if i in cfg["global_blocks"]:
            sets, h, w = 1, H, W
        else:
            sets, h, w = -(-H // ws) * -(-W // ws), ws, ws
        N = h * w
        total += batch * sets * cfg["nh"] * N * (4.0 * N * dh + 2.0 * (h + w) * dh)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="a small encoder instead of the -L shape")
    ap.add_argument("--save", default=None)
    ap.add_argument("--load", default=None)
    ap.add_argument("--lib", default=None, help="time this build of the library instead of the tree's own")
    a = ap.parse_args()
    cfg = SMALL if a.small else L_SHAPE
    if a.lib:
        api.LIB_PATH = Path(a.lib).resolve()
    if a.load:
        model = Path(a.load).read_bytes()
    else:
        model, _ = models.build_vary_vit(seed=0, **cfg)
    if a.save:
        Path(a.save).write_bytes(model)
    x = np.random.default_rng(0).standard_normal((a.batch, 1) + tuple(cfg["image_shape"])).astype(np.float32)
    eng = api.OrtInfer(model, profile=True)
    try:
        eng.infer(x)
        eng.infer(x)
        ev, wall, launches, rp, rp_us = [], [], 0, 0, []
        for _ in range(a.reps):
            api.prof_reset()
            api.prof_enable(True)
            eng.infer(x)
            snap = api.prof_snapshot()
            api.prof_enable(False)
            ev.append(sum(e["total_ms"] for e in snap) * 1e3)
            launches = sum(e["launches"] for e in snap)
            rp = sum(e["launches"] for e in snap if e["name"] == "relpos_attention")
            rp_us.append(sum(e["total_ms"] for e in snap if e["name"] == "relpos_attention") * 1e3)
            t0 = time.perf_counter()
            eng.infer(x)
            wall.append((time.perf_counter() - t0) * 1e6)
        top = sorted(snap, key=lambda e: -e["total_ms"])[:8]
        us = float(np.median(rp_us))
        print(json.dumps({"fuse_relpos_attention": os.environ.get("OAR_FUSE_RELPOS_ATTENTION", "default"), "lib": a.lib or "tree", "batch": a.batch, "shape": "small" if a.small else "L",
                          "event_us_per_infer": round(float(np.median(ev)), 1), "event_us_reps": [round(v, 1) for v in ev], "wall_us_per_infer": round(float(np.median(wall)), 1),
                          "launches_per_infer": launches, "relpos_attention_launches": rp, "relpos_attention_us": round(us, 1),
                          "relpos_attention_tflops": round(relpos_flops(cfg, a.batch) / us / 1e6, 2) if rp else None,
                          "top_classes_us": {e["name"]: round(e["total_ms"] * 1e3, 1) for e in top}}), flush=True)
    finally:
        api.prof_enable(False)
        eng.close()


if __name__ == "__main__":
    main()
