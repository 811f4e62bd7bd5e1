"""Speed of the MultiHeadAttention launch against the launches it replaces.  OAR_FUSE_MHA_ATTENTION is read when a graph is loaded, so the script
loads every graph twice -- once with the rewrite, once with the knob at 0 -- and alternates the two engines in ONE process; all times are the profiler's event
intervals.  The deformable-attention rewrite is on in both arms.

  mha300 / mha400   synth.models.build_mha at Tq = Tk = 300 and 400, 8 heads of 32: the block on its own
  decoder           synth.models.build_rtdetr_decoder at RT-DETR-L's shape: D = 256, 8 heads, 4 points, 300 queries, levels 80^2 / 40^2 / 20^2, six layers
  aifi20 / aifi25   synth.models.build_aifi_layer at 20 x 20 and 25 x 25 tokens, D = 256, 8 heads, F = 1024

Everything outside the block is common to the arms, so  (op-by-op total) - (fused total - mha_attention)  is the replaced launches' time; adjacent repetitions
are paired.  Prints one JSON line per (graph, batch): medians and the min .. max spread over the repetitions, launches per infer of each arm, whether the fused
arm's range lies entirely below the op-by-op arm's (the rule that decides the knob's default), the largest |difference| of the two arms' outputs, and the
kernel's achieved TFLOP/s against the 155 TF f32-matrix peak, for information.
Usage: python tools/mha_attention_bench.py [--batch 1 8] [--reps 30] [--warmup 5] [--graphs mha300 mha400 decoder aifi20 aifi25] [--lib other.so]"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api                      # noqa: E402
from oar_ocr_amd.synth import models             # noqa: E402

KNOB = "OAR_FUSE_MHA_ATTENTION"
D, NH, P, Q, LEVELS, LAYERS, F = 256, 8, 4, 300, ((80, 80), (40, 40), (20, 20)), 6, 1024
PEAK_TF = 155.0


def load(model, fuse):
    old = {k: os.environ.get(k) for k in (KNOB, "OAR_FUSE_DEFORMABLE_ATTENTION")}
    os.environ[KNOB] = "1" if fuse else "0"
    os.environ["OAR_FUSE_DEFORMABLE_ATTENTION"] = "1"
    try:
        return api.OrtInfer(model, profile=True)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def timed(eng, feeds):
    api.prof_reset()
    api.prof_enable(True)
    outs = eng.infer(feeds)
    snap = api.prof_snapshot()
    api.prof_enable(False)
    ma = [e for e in snap if e["name"] == "mha_attention"]
    return {"total_us": sum(e["total_ms"] for e in snap) * 1e3, "launches": sum(e["launches"] for e in snap), "ma_us": sum(e["total_ms"] for e in ma) * 1e3,
            "ma_launches": sum(e["launches"] for e in ma), "classes": {e["name"]: (e["launches"], e["total_ms"] * 1e3) for e in snap}}, outs


def stat(v):
    return {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}


def run(name, model, feeds, blocks, flops, reps, warmup, batch):
    arms = {"fused": load(model, True), "op_by_op": load(model, False)}
    try:
        for _ in range(warmup):
            for eng in arms.values():
                eng.infer(feeds)
        rec = {k: [] for k in arms}
        outs = {}
        for _ in range(reps):
            for k, eng in arms.items():                                  # alternating: fused, op by op, fused, ...
                r, outs[k] = timed(eng, feeds)
                rec[k].append(r)
        f, p = rec["fused"], rec["op_by_op"]
        assert all(r["ma_launches"] == blocks for r in f) and all(r["ma_launches"] == 0 for r in p), "the rewrite did not take (or took with the knob at 0)"
        fused_us = [r["ma_us"] for r in f]
        replaced_us = [b["total_us"] - (a["total_us"] - a["ma_us"]) for a, b in zip(f, p)]
        tf, tp = [r["total_us"] for r in f], [r["total_us"] for r in p]
        diff = max(float(np.abs(np.asarray(a[1], np.float64) - np.asarray(b[1], np.float64)).max()) for a, b in zip(outs["fused"], outs["op_by_op"]))
        top = sorted(p[-1]["classes"].items(), key=lambda kv: -kv[1][1])[:6]
        print(json.dumps({"graph": name, "batch": batch, "blocks": blocks, "reps": reps, "launches_per_infer": {"fused": f[-1]["launches"], "op_by_op": p[-1]["launches"]},
                          "total_us_per_infer": {"fused": stat(tf), "op_by_op": stat(tp)}, "fused_range_entirely_below": bool(max(tf) < min(tp)),
                          "fused_us_per_infer": stat(fused_us), "replaced_us_per_infer": stat(replaced_us),
                          "ratio_of_medians": round(float(np.median(fused_us) / np.median(replaced_us)), 3),
                          "launches_per_block": {"fused": 1, "op_by_op": (p[-1]["launches"] - (f[-1]["launches"] - blocks)) / blocks},
                          "kernel_TFLOPs": round(flops / (np.median(fused_us) * 1e-6) / 1e12, 2), "kernel_fraction_of_f32_matrix_peak": round(flops / (np.median(fused_us) * 1e-6) / 1e12 / PEAK_TF, 4),
                          "max_abs_output_difference": diff, "op_by_op_top_classes": {k: {"launches": v[0], "us": round(v[1], 1)} for k, v in top}}), flush=True)
    finally:
        api.prof_enable(False)
        for eng in arms.values():
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", nargs="+", default=["mha300", "mha400", "decoder", "aifi20", "aifi25"])
    ap.add_argument("--lib", default=None, help="time this build of the library instead of the tree's own")
    a = ap.parse_args()
    if a.lib:
        api.LIB_PATH = Path(a.lib).resolve()
    Lv = sum(h * w for h, w in LEVELS)
    core = lambda n, T: 4.0 * n * NH * T * T * (D // NH)                  # the two products of one block, multiply and add counted apart
    for n in a.batch:
        rng = np.random.default_rng(n)
        for T in (300, 400):
            if f"mha{T}" in a.graphs:
                model, _ = models.build_mha(n, T, T, NH, D // NH, seed=0)
                run(f"mha{T}", model, [("x", rng.standard_normal((n, T, D)).astype(np.float32))], 1, core(n, T), a.reps, a.warmup, n)
        if "decoder" in a.graphs:
            model, _ = models.build_rtdetr_decoder(D=D, nh=NH, levels=LEVELS, P=P, layers=LAYERS, Q=Q, n_classes=80, seed=0)
            feeds = [("memory", rng.standard_normal((n, Lv, D)).astype(np.float32)), ("tgt", rng.standard_normal((n, Q, D)).astype(np.float32)),
                     ("ref_logit", rng.uniform(-1.5, 1.5, (n, Q, 4)).astype(np.float32))]
            run("decoder", model, feeds, LAYERS, LAYERS * core(n, Q), a.reps, a.warmup, n)
        for side in (20, 25):
            if f"aifi{side}" in a.graphs:
                model, _ = models.build_aifi_layer(side, side, D, NH, F, seed=0)
                run(f"aifi{side}", model, [("src", rng.standard_normal((n, side * side, D)).astype(np.float32))], 1, core(n, side * side), a.reps, a.warmup, n)


if __name__ == "__main__":
    main()
