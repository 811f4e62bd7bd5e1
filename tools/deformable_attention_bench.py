"""Speed of the DeformableAttention launch against the launches it replaces, at RT-DETR-L's decoder shape: D = 256, 8 heads, 4 points, 300 queries,
levels 80^2 / 40^2 / 20^2 (a 640^2 input), six layers.  OAR_FUSE_DEFORMABLE_ATTENTION is read when a graph is loaded, so the script loads every graph twice --
once with the rewrite, once with the knob at 0 -- and alternates the two engines in ONE process; all times are the profiler's event intervals.

  core     synth.models.build_deformable_attention: the op-by-op arm consists of exactly the launches the fused one replaces
  decoder  synth.models.build_rtdetr_decoder: everything else in the graph is common to the arms, so  (op-by-op total) - (fused total - deformable_attention)
           is the replaced launches' time; adjacent repetitions are paired

Prints one JSON line per (graph, batch): medians and the min .. max spread over the repetitions, launches per layer of each arm, the largest |difference| of the
two arms' outputs at the timed size, and the kernel's achieved bytes / s over the bytes its taps, locations, weights and output need (k::deformable_attention's
own count).  Usage: python tools/deformable_attention_bench.py [--batch 1 8] [--reps 30] [--warmup 5] [--layers 6]"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api                      # noqa: E402
from oar_ocr_amd.synth import models             # noqa: E402

KNOB = "OAR_FUSE_DEFORMABLE_ATTENTION"
D, NH, P, Q, LEVELS = 256, 8, 4, 300, ((80, 80), (40, 40), (20, 20))


def load(model, fuse):
    old = os.environ.get(KNOB)
    os.environ[KNOB] = "1" if fuse else "0"
    try:
        return api.OrtInfer(model, profile=True)
    finally:
        if old is None:
            del os.environ[KNOB]
        else:
            os.environ[KNOB] = old


def timed(eng, feeds):
    api.prof_reset()
    api.prof_enable(True)
    outs = eng.infer(feeds)
    snap = api.prof_snapshot()
    api.prof_enable(False)
    da = [e for e in snap if e["name"] == "deformable_attention"]
    return {"total_us": sum(e["total_ms"] for e in snap) * 1e3, "launches": sum(e["launches"] for e in snap), "da_us": sum(e["total_ms"] for e in da) * 1e3,
            "da_launches": sum(e["launches"] for e in da), "da_bytes": sum(e["alg_bytes"] for e in da), "classes": {e["name"]: (e["launches"], e["total_ms"] * 1e3) for e in snap}}, outs


def stat(v):
    return {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}


def run(name, model, feeds, layers, reps, warmup, batch):
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
        assert all(r["da_launches"] == layers for r in f) and all(r["da_launches"] == 0 for r in p), "the rewrite did not take (or took with the knob at 0)"
        fused_us = [r["da_us"] for r in f]
        replaced_us = [b["total_us"] - (a["total_us"] - a["da_us"]) for a, b in zip(f, p)]
        diff = max(float(np.abs(np.asarray(a[1], np.float64) - np.asarray(b[1], np.float64)).max()) for a, b in zip(outs["fused"], outs["op_by_op"]))
        top = sorted(p[-1]["classes"].items(), key=lambda kv: -kv[1][1])[:6]
        print(json.dumps({"graph": name, "batch": batch, "layers": layers, "reps": reps, "fused_us_per_infer": stat(fused_us), "replaced_us_per_infer": stat(replaced_us),
                          "ratio_of_medians": round(float(np.median(fused_us) / np.median(replaced_us)), 3),
                          "launches_per_layer": {"fused": 1, "op_by_op": (p[-1]["launches"] - (f[-1]["launches"] - layers)) / layers},
                          "launches_per_infer": {"fused": f[-1]["launches"], "op_by_op": p[-1]["launches"]},
                          "total_us_per_infer": {"fused": stat([r["total_us"] for r in f]), "op_by_op": stat([r["total_us"] for r in p])},
                          "kernel_GBps": round(f[-1]["da_bytes"] / (np.median(fused_us) * 1e-6) / 1e9, 1), "kernel_bytes_per_infer": f[-1]["da_bytes"],
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
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--graphs", nargs="+", default=["core", "decoder"])
    a = ap.parse_args()
    Lv, L = sum(h * w for h, w in LEVELS), len(LEVELS)
    core, _ = models.build_deformable_attention(1, Q, NH, D // NH, LEVELS, P)
    dec, _ = models.build_rtdetr_decoder(D=D, nh=NH, levels=LEVELS, P=P, layers=a.layers, Q=Q, n_classes=80, seed=0)
    for n in a.batch:
        rng = np.random.default_rng(n)
        if "core" in a.graphs:   # sampling points scattered around a reference point inside the image, as a decoder's are
            centre = rng.uniform(0.1, 0.9, (n, Q, 1, 1, 1, 2))
            loc = (centre + 0.08 * rng.standard_normal((n, Q, NH, L, P, 2))).astype(np.float32)
            feeds = [("value", rng.standard_normal((n, Lv, D)).astype(np.float32)), ("loc", loc), ("logit", rng.standard_normal((n, Q, NH * L * P)).astype(np.float32))]
            run("core", core, feeds, 1, a.reps, a.warmup, n)
        if "decoder" in a.graphs:
            feeds = [("memory", rng.standard_normal((n, Lv, D)).astype(np.float32)), ("tgt", rng.standard_normal((n, Q, D)).astype(np.float32)),
                     ("ref_logit", rng.uniform(-1.5, 1.5, (n, Q, 4)).astype(np.float32))]
            run("decoder", dec, feeds, a.layers, a.reps, a.warmup, n)


if __name__ == "__main__":
    main()
