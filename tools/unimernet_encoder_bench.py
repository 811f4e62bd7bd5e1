"""Speed of the UniMERNet-shaped encoder with and without the WindowAttention rewrite: event time per `infer` of
synth.models.build_unimernet(encoder_only=True) at the preprocessor's target (672, 192).  OAR_FUSE_WINDOW_ATTENTION is read when the graph is loaded, so one
process times one arm: run the two arms in alternating processes and compare their spread.  Prints one JSON line: the median and every repetition of the
profiler's summed event time over all classes, the launches per infer, those of class window_attention, and the wall time of an unprofiled infer.
--ws 7 makes every stage pad (48 x 168 and 24 x 84 tokens are no multiples of 7) and --shifted makes the odd blocks roll and mask.
Usage: OAR_FUSE_WINDOW_ATTENTION=0|1 python tools/unimernet_encoder_bench.py [--reps 7] [--batch 1] [--ws 6] [--shifted] [--save graph.onnx | --load graph.onnx] [--lib other.so]"""
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

WIDTHS = dict(C=96, heads=(3, 6), depths=(2, 2), mlp_ratio=4)            # UniMERNet-like: 48 x 168 tokens at width 96, then 24 x 84 at 192; head size 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--ws", type=int, default=6, help="window side (6: N = 36; 12: N = 144; both divide 24 and 84.  7, Swin's own: the blocks pad)")
    ap.add_argument("--shifted", action="store_true", help="odd blocks shift by ws // 2 and add the shifted-window mask")
    ap.add_argument("--save", default=None)
    ap.add_argument("--load", default=None)
    ap.add_argument("--lib", default=None, help="time this build of the library instead of the tree's own")
    a = ap.parse_args()
    if a.lib:
        api.LIB_PATH = Path(a.lib).resolve()
    if a.load:
        model = Path(a.load).read_bytes()
    else:
        model, _ = models.build_unimernet(image_shape=(192, 672), encoder_only=True, seed=0, ws=a.ws, shifted=a.shifted, **WIDTHS)
    if a.save:
        Path(a.save).write_bytes(model)
    x = np.random.default_rng(0).random((a.batch, 1, 192, 672)).astype(np.float32)
    eng = api.OrtInfer(model, profile=True)
    try:
        eng.infer(x)
        eng.infer(x)
        ev, wall, launches, wa = [], [], 0, 0
        for _ in range(a.reps):
            api.prof_reset()
            api.prof_enable(True)
            eng.infer(x)
            snap = api.prof_snapshot()
            api.prof_enable(False)
            ev.append(sum(e["total_ms"] for e in snap) * 1e3)
            launches = sum(e["launches"] for e in snap)
            wa = sum(e["launches"] for e in snap if e["name"] == "window_attention")
            t0 = time.perf_counter()
            eng.infer(x)
            wall.append((time.perf_counter() - t0) * 1e6)
        top = sorted(snap, key=lambda e: -e["total_ms"])[:6]
        print(json.dumps({"fuse_window_attention": os.environ.get("OAR_FUSE_WINDOW_ATTENTION", "default"), "lib": a.lib or "tree", "batch": a.batch, "ws": a.ws, "shifted": a.shifted, "widths": {k: list(v) if isinstance(v, tuple) else v for k, v in WIDTHS.items()},
                          "event_us_per_infer": round(float(np.median(ev)), 1), "event_us_reps": [round(v, 1) for v in ev], "wall_us_per_infer": round(float(np.median(wall)), 1),
                          "launches_per_infer": launches, "window_attention_launches": wa, "top_classes_us": {e["name"]: round(e["total_ms"] * 1e3, 1) for e in top}}), flush=True)
    finally:
        api.prof_enable(False)
        eng.close()


if __name__ == "__main__":
    main()
