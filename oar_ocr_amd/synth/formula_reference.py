"""The formula head (synth.models.build_formulanet's Loop, with the cross-attention keys / values the graph computes before it) restated in torch on the
CPU, in f64 and f32: the reference the GPU tests hold the decode kernels to, and the measure of how much f32 rounding alone moves the result (`noise`)."""
from __future__ import annotations

import numpy as np


def formula_head_reference(w, memory, M, dtype="float64", sos=0):
    """w: the arrays and scalars of synth.models.formula_weights (info["weights"] of build_formulanet; its "q_scale_pos" says on which side of the bias Add
    the query scale stands, default "after"; with squeeze attention Wq / Wk have nh dq < D rows and "cq_scale" is the cross-attention's own scale);
    memory [B, S, D].  Returns logits [B, M, V] and tokens
    [B, M] (arg max, first index among equals) as numpy arrays."""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    with torch.no_grad():
        t = {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in w.items() if isinstance(v, np.ndarray)}
        mem = torch.from_numpy(np.asarray(memory)).to(dt)
        B, S, D = mem.shape
        nh, Ld, eps = int(w["nh"]), int(w["Ld"]), float(w["eps"])
        dh, dq, dc = D // nh, t["l0_wq"].shape[0] // nh, t["l0_wcq"].shape[0] // nh     # value / self q.k / cross q.k head sizes
        cqs = torch.tensor(np.float32(w.get("cq_scale", w["q_scale"]))).to(dt)
        s_emb, qs, c_pos = torch.tensor(np.float32(w["s_emb"])).to(dt), torch.tensor(np.float32(w["q_scale"])).to(dt), int(w["c_pos"])
        ln = lambda x, nm: Fn.layer_norm(x, (D,), t[nm + "_g"], t[nm + "_b"], eps)
        lin = lambda x, wn, bn: x @ t[wn].T + t[bn]
        if w.get("q_scale_pos", "after") == "before":            # the graph scales the product and adds the bias afterwards
            qlin = lambda x, wn, bn, s=qs: (x @ t[wn].T) * s + t[bn]
        else:
            qlin = lambda x, wn, bn, s=qs: lin(x, wn, bn) * s
        KmT = [lin(mem, f"l{l}_wck", f"l{l}_bck").reshape(B, S, nh, dc).permute(0, 2, 3, 1) for l in range(Ld)]
        Vm = [lin(mem, f"l{l}_wcv", f"l{l}_bcv").reshape(B, S, nh, dh).permute(0, 2, 1, 3) for l in range(Ld)]
        K = [torch.zeros(B, nh, 0, dq, dtype=dt) for _ in range(Ld)]
        Vc = [torch.zeros(B, nh, 0, dh, dtype=dt) for _ in range(Ld)]
        tok = torch.full((B,), int(sos), dtype=torch.long)
        logits, toks = [], []
        for i in range(M):
            x = ln(t["e_tok"][tok] * s_emb + t["e_pos"][i + c_pos], "lne")
            for l in range(Ld):
                p = f"l{l}_"
                y = ln(x, p + "ln1")
                q = qlin(y, p + "wq", p + "bq").reshape(B, nh, 1, dq)
                K[l] = torch.cat([K[l], lin(y, p + "wk", p + "bk").reshape(B, nh, 1, dq)], 2)
                Vc[l] = torch.cat([Vc[l], lin(y, p + "wv", p + "bv").reshape(B, nh, 1, dh)], 2)
                o = (torch.softmax(q @ K[l].transpose(2, 3), -1) @ Vc[l]).reshape(B, D)
                x = x + lin(o, p + "wo", p + "bo")
                y = ln(x, p + "ln2")
                qc = qlin(y, p + "wcq", p + "bcq", cqs).reshape(B, nh, 1, dc)
                oc = (torch.softmax(qc @ KmT[l], -1) @ Vm[l]).reshape(B, D)
                x = x + lin(oc, p + "wco", p + "bco")
                y = ln(x, p + "ln3")
                x = x + lin(Fn.gelu(lin(y, p + "w1", p + "b1")), p + "w2", p + "b2")
            lg = lin(ln(x, "lnf"), "w_lm", "b_lm")
            tok = torch.from_numpy(np.argmax(lg.numpy(), 1))                                # numpy: the first maximum, documented
            logits.append(lg); toks.append(tok)
        return {"logits": torch.stack(logits, 1).numpy(), "tokens": torch.stack(toks, 1).numpy()}


def formula_memory_reference(w, x, dtype="float64"):
    """build_formulanet's backbone in torch: x [B, 1, H, W] -> memory [B, (H / 8) (W / 8), D] (patch convolution, hard-swish, 1 x 1 convolution)"""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    with torch.no_grad():
        c = lambda k: torch.from_numpy(np.asarray(w[k])).to(dt)
        t = Fn.conv2d(torch.from_numpy(np.asarray(x)).to(dt), c("bb_w1"), c("bb_b1"), stride=8)
        t = t * torch.clamp(t / 6.0 + 0.5, 0.0, 1.0)
        t = Fn.conv2d(t, c("bb_w2"), c("bb_b2"))
        return t.reshape(t.shape[0], t.shape[1], -1).transpose(1, 2).contiguous().numpy()


def formula_reference_bundle(w, memory, M, sos=0):
    """f64 reference, the f32 run of the same math, and what separates them:
      noise: max |f32 - f64| of the logits over all steps
      tol = max(16 noise, 2^-19): 16 covers a different reduction order and the device's exp / erf, each a few ulp, feeding the cache every later step reads
      gap: the smallest difference between the two largest f64 logits of any step (how close the greedy path comes to forking)
      changes: how often the emitted token differs from the previous one"""
    r64, r32 = formula_head_reference(w, memory, M, "float64", sos), formula_head_reference(w, memory, M, "float32", sos)
    noise = float(np.abs(r32["logits"].astype(np.float64) - r64["logits"]).max())
    top2 = np.partition(r64["logits"], -2, axis=2)[..., -2:]
    return {"f64": r64, "f32": r32, "tokens": r64["tokens"], "logits": r64["logits"], "noise": noise, "tol": max(16 * noise, 2.0 ** -19),
            "gap": float((top2[..., 1] - top2[..., 0]).min()), "changes": int((r64["tokens"][:, 1:] != r64["tokens"][:, :-1]).sum())}
