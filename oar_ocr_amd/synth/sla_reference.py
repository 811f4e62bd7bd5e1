"""The SLA head (synth.models.build_slanet's Loop) restated in torch on the CPU, in f64 and f32: the reference the GPU tests hold the fused
decode kernel to, and the measure of how much f32 rounding alone moves the result (`noise`)."""
from __future__ import annotations

import numpy as np


def sla_head_reference(w, fea, M, dtype="float64", h0=None, pre0=None):
    """w: the arrays of synth.models.sla_weights; fea [B, HW, C].  Returns logits [B, M, V], probs (softmax of the logits), loc [B, M, L],
    tokens [B, M] (arg max, first index among equals) and the last hidden state h [B, H], as numpy arrays of `dtype`."""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        w = {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in w.items()}
        fea = torch.from_numpy(np.asarray(fea)).to(dt)
        B = fea.shape[0]
        H, V = w["h2h_w"].shape[0], w["s2w"].shape[0]
        proj = fea @ w["i2h"].T
        h = torch.zeros(B, H, dtype=dt) if h0 is None else torch.from_numpy(np.asarray(h0)).to(dt)
        pre = torch.zeros(B, dtype=torch.long) if pre0 is None else torch.from_numpy(np.asarray(pre0)).long()
        logits, locs, toks = [], [], []
        for _ in range(M):
            hp = h @ w["h2h_w"].T + w["h2h_b"]
            e = torch.tanh(proj + hp[:, None, :]) @ w["score"].T                    # [B, HW, 1]
            ctx = (torch.softmax(e, 1).transpose(1, 2) @ fea)[:, 0]                   # [B, C]
            x = torch.cat([ctx, torch.nn.functional.one_hot(pre, V).to(dt)], 1)
            xr, xz, xc = (x @ w["wih"].T + w["bih"]).chunk(3, 1)
            hr, hz, hc = (h @ w["whh"].T + w["bhh"]).chunk(3, 1)
            r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
            c = torch.tanh(xc + r * hc)
            h = (h - c) * z + c
            s = (h @ w["s1w"].T + w["s1b"]) @ w["s2w"].T + w["s2b"]
            l = torch.sigmoid((h @ w["l1w"].T + w["l1b"]) @ w["l2w"].T + w["l2b"])
            pre = torch.from_numpy(np.argmax(s.numpy(), 1))                           # numpy: the first maximum, documented
            logits.append(s); locs.append(l); toks.append(pre)
        lg = torch.stack(logits, 1)
        return {"logits": lg.numpy(), "probs": torch.softmax(lg, 2).numpy(), "loc": torch.stack(locs, 1).numpy(), "tokens": torch.stack(toks, 1).numpy(),
                "h": h.numpy()}


def sla_reference_bundle(w, fea, M):
    """f64 reference, the f32 run of the same math, and what separates them:
      noise / noise_loc / noise_h: max |f32 - f64| of the probabilities / locations (all steps) / last hidden state
      tol = max(16 noise, 2^-19), tol_loc likewise: 16 covers a different reduction order and the device's exp / tanh, each a few ulp, feeding a
            recurrent state; the floor is 16 ulp of 1.0
      gap: the smallest difference between the two largest f64 probabilities of any step (how close the greedy path comes to forking)"""
    r64, r32 = sla_head_reference(w, fea, M, "float64"), sla_head_reference(w, fea, M, "float32")
    noise = float(np.abs(r32["probs"].astype(np.float64) - r64["probs"]).max())
    noise_loc = float(np.abs(r32["loc"].astype(np.float64) - r64["loc"]).max())
    noise_h = float(np.abs(r32["h"].astype(np.float64) - r64["h"]).max())
    top2 = np.sort(r64["probs"], axis=2)[..., -2:]
    floor = 2.0 ** -19
    return {"f64": r64, "f32": r32, "noise": noise, "noise_loc": noise_loc, "noise_h": noise_h, "tol": max(16 * noise, floor), "tol_loc": max(16 * noise_loc, floor),
            "gap": float((top2[..., 1] - top2[..., 0]).min()), "changes": int((r64["tokens"][:, 1:] != r64["tokens"][:, :-1]).sum())}
