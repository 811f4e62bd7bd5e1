"""Speed of the FormulaDecode operator on PP-FormulaNet-S- and -L-shaped heads: microseconds per decode step from the profiler's event intervals of
class `formula_decode`, the weight bytes a step streams over that time, and the same math as an eager torch loop on the same card in the same process
(alternating runs, medians).  Usage: python tools/formula_decode_bench.py [--reps 5] [--steps 64] [--heads S,L,U] [--squeeze r]
Head U is UniMERNet's MBart decoder (D 1024, 16 heads, F 4096, 8 layers, V 50000) with squeeze attention r = 2; --squeeze r overrides a
head's own r (1 for S and L).

--stop adds the stop token of `OrtInfer.set_decode_stop` (one more JSON line per head, batch and mode, the modes alternating inside every repetition):
  off      the setting off: all M steps run (the only mode of a build that has no stop token: `--lib` / a copy of this file in an older tree)
  never    on, with a token the torch loop never emits: all M steps run and every poll point is paid -- the cost of the feature where it gains nothing
  eighth   on, with the token of the torch loop's own output whose last first occurrence over the rows lies nearest M / 8
  all      the three of them
Per line: microseconds per step of class `formula_decode` (its total over M, and over the steps that did work), every repetition's figure, the wall time of an
unprofiled `infer`, steps_executed and steps_enqueued.  --lib times another build of the library (e.g. one compiled with another -DOAR_FD_LOOKAHEAD)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api                      # noqa: E402
from oar_ocr_amd.synth import models             # noqa: E402

HEADS = {"S": dict(D=384, nh=16, F=1536, Ld=2, V=50000, S=144), "L": dict(D=512, nh=16, F=2048, Ld=8, V=50000, S=144),
         "U": dict(D=1024, nh=16, F=4096, Ld=8, V=50000, S=144, r=2)}


def torch_loop(w, mem, M):
    """formula_reference.formula_head_reference on the device in f32, the arg max fed back without leaving the device; returns a closure that runs all M steps"""
    import torch
    import torch.nn.functional as Fn
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in w.items() if isinstance(v, np.ndarray)}
    mem = torch.from_numpy(mem).to(dev)
    B, S, D = mem.shape
    nh, Ld, eps = int(w["nh"]), int(w["Ld"]), float(w["eps"])
    dh, dq = D // nh, w["l0_wq"].shape[0] // nh
    s_emb, qs, cqs, c_pos = float(w["s_emb"]), float(w["q_scale"]), float(w.get("cq_scale", w["q_scale"])), int(w["c_pos"])
    ln = lambda x, nm: Fn.layer_norm(x, (D,), t[nm + "_g"], t[nm + "_b"], eps)
    lin = lambda x, wn, bn: Fn.linear(x, t[wn], t[bn])

    def run():
        with torch.no_grad():
            KmT = [lin(mem, f"l{l}_wck", f"l{l}_bck").reshape(B, S, nh, dh).permute(0, 2, 3, 1) for l in range(Ld)]
            Vm = [lin(mem, f"l{l}_wcv", f"l{l}_bcv").reshape(B, S, nh, dh).permute(0, 2, 1, 3) for l in range(Ld)]
            K = [torch.zeros(B, nh, M, dq, device=dev) for _ in range(Ld)]
            Vc = [torch.zeros(B, nh, M, dh, device=dev) for _ in range(Ld)]
            tok = torch.zeros(B, dtype=torch.long, device=dev)
            toks = []
            for i in range(M):
                x = ln(t["e_tok"][tok] * s_emb + t["e_pos"][i + c_pos], "lne")
                for l in range(Ld):
                    p = f"l{l}_"
                    y = ln(x, p + "ln1")
                    q = (lin(y, p + "wq", p + "bq") * qs).reshape(B, nh, 1, dq)
                    K[l][:, :, i] = lin(y, p + "wk", p + "bk").reshape(B, nh, dq)
                    Vc[l][:, :, i] = lin(y, p + "wv", p + "bv").reshape(B, nh, dh)
                    o = (torch.softmax(q @ K[l][:, :, :i + 1].transpose(2, 3), -1) @ Vc[l][:, :, :i + 1]).reshape(B, D)
                    x = x + lin(o, p + "wo", p + "bo")
                    y = ln(x, p + "ln2")
                    qc = (lin(y, p + "wcq", p + "bcq") * cqs).reshape(B, nh, 1, dh)
                    x = x + lin((torch.softmax(qc @ KmT[l], -1) @ Vm[l]).reshape(B, D), p + "wco", p + "bco")
                    x = x + lin(Fn.gelu(lin(ln(x, p + "ln3"), p + "w1", p + "b1")), p + "w2", p + "b2")
                tok = torch.argmax(lin(ln(x, "lnf"), "w_lm", "b_lm"), 1)
                toks.append(tok)
            return torch.stack(toks, 1)
    return run


def pick_stop(tokens, V, where):
    """(token, the step after which a chunk holding all rows ends) -- `never`: the lowest id that occurs nowhere; `eighth`: see the module docstring"""
    B, M = tokens.shape
    if where == "never":
        return int(np.setdiff1d(np.arange(V), tokens.ravel())[0]), M - 1
    best = None
    for e in np.unique(tokens):
        t_stop = max(int(np.nonzero(r == e)[0][0]) if np.any(r == e) else M - 1 for r in tokens)
        if best is None or abs(t_stop - M // 8) < abs(best[1] - M // 8):
            best = (int(e), t_stop)
    return best


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--heads", default="S,L")
    ap.add_argument("--squeeze", type=int, default=None, help="squeeze attention: Wq / Wk project to D / r (default: the head's own, 1 for S and L)")
    ap.add_argument("--stop", choices=["off", "never", "eighth", "all"], default=None)
    ap.add_argument("--lib", default=None, help="time this build of the library instead of the tree's own")
    a = ap.parse_args()
    if a.lib:
        api.LIB_PATH = Path(a.lib).resolve()
    M = a.steps
    has_stop = hasattr(api.OrtInfer, "set_decode_stop")
    modes = [] if a.stop is None else ["off", "never", "eighth"] if a.stop == "all" else [a.stop]
    if not has_stop:
        modes = [m for m in modes if m == "off"]
    for name in a.heads.split(","):
        h = HEADS[name]
        r = a.squeeze if a.squeeze is not None else h.get("r", 1)
        w = models.formula_weights(h["D"], h["nh"], h["F"], h["V"], h["Ld"], M + 2, 0) if r == 1 else models.formula_weights(h["D"], h["nh"], h["F"], h["V"], h["Ld"], M + 2, 0, qk_squeeze=r)
        model, _ = models.build_formulanet(D=h["D"], nh=h["nh"], F=h["F"], V=h["V"], Ld=h["Ld"], M=M, head_only=True, weights=w)
        eng = api.OrtInfer(model, profile=True)
        D, F, Ld, V = h["D"], h["F"], h["Ld"], h["V"]
        weight_bytes = 4.0 * (Ld * ((4 + 2.0 / r) * D * D + 2 * F * D) + V * D)
        for B in (1, 8):
            mem = np.random.default_rng(B).standard_normal((B, h["S"], D)).astype(np.float32)
            loop = torch_loop(w, mem, M)
            ids = dict(eng.infer(mem))["token_ids"]
            torch_ids = loop().cpu().numpy()
            same = bool(np.array_equal(ids, torch_ids))
            ours, wall, theirs = [], [], []
            for _ in range(a.reps):
                api.prof_reset()
                api.prof_enable(True)
                t0 = time.perf_counter()
                eng.infer(mem)
                wall.append((time.perf_counter() - t0) * 1e6 / M)
                snap = {e["name"]: e for e in api.prof_snapshot()}
                api.prof_enable(False)
                ours.append(snap["formula_decode"]["total_ms"] * 1e3 / M)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loop()
                e1.record()
                torch.cuda.synchronize()
                theirs.append(e0.elapsed_time(e1) * 1e3 / M)
            us = float(np.median(ours))
            print(json.dumps({"head": name, "squeeze": r, "B": B, "M": M, "us_per_step_kernels": round(us, 1), "us_per_step_wall_profiled": round(float(np.median(wall)), 1),
                              "weight_MB_per_step": round(weight_bytes / 1e6, 1), "share_of_8TBps": round(weight_bytes / (us * 1e-6) / 8e12, 3),
                              "torch_eager_us_per_step": round(float(np.median(theirs)), 1), "tokens_equal_torch_f32": same}), flush=True)
            if not modes:
                continue
            stops = {m: (None, M - 1) if m == "off" else pick_stop(torch_ids, V, m) for m in modes}
            rec = {m: dict(us=[], wall=[], executed=[], enqueued=[]) for m in modes}
            for _ in range(a.reps):
                for m in modes:                                    # alternating: every repetition visits every mode
                    if has_stop:
                        eng.set_decode_stop(-1 if m == "off" else stops[m][0])
                    api.prof_reset()
                    api.prof_enable(True)
                    eng.infer(mem)
                    snap = {e["name"]: e for e in api.prof_snapshot()}
                    api.prof_enable(False)
                    rec[m]["us"].append(snap["formula_decode"]["total_ms"] * 1e3)
                    t0 = time.perf_counter()
                    eng.infer(mem)                                 # unprofiled: the wall time a caller sees
                    rec[m]["wall"].append((time.perf_counter() - t0) * 1e3)
                    st = eng.decode_stats() if has_stop else None
                    rec[m]["executed"].append(st.steps_executed if st else M)
                    rec[m]["enqueued"].append(st.steps_enqueued if st else M)
            for m in modes:
                r = rec[m]
                tot = float(np.median(r["us"]))
                print(json.dumps({"head": name, "B": B, "M": M, "mode": m, "stop_token": stops[m][0], "t_stop_expected": stops[m][1],
                                  "us_per_step_kernels": round(tot / M, 2), "us_per_step_kernels_reps": [round(v / M, 2) for v in r["us"]],
                                  "us_per_executed_step": round(tot / max(int(np.median(r["executed"])), 1), 2),
                                  "formula_decode_ms": round(tot / 1e3, 3), "wall_ms": round(float(np.median(r["wall"])), 3), "wall_ms_reps": [round(v, 3) for v in r["wall"]],
                                  "steps_executed": int(np.median(r["executed"])), "steps_enqueued": int(np.median(r["enqueued"])),
                                  "lookahead": int(st.lookahead) if st else None}), flush=True)
            if has_stop:
                eng.set_decode_stop(-1)
        eng.close()


if __name__ == "__main__":
    main()
