"""The SAM / Vary ViT block of synth.models.build_vit_block and the encoder of build_vary_vit restated in torch on the CPU, in f64 and f32, from the
formulas (F.pad, the window partition, einsum for the decomposed relative-position bias q . Rh[qy, ky] + q . Rw[qx, kx], soft-max, projection, window
reverse, crop), not by evaluating the graph.  `variant` names one of the WRONG readings tests/test_vit_relpos_cpu.py tells apart from the right one."""
from __future__ import annotations

import numpy as np

from .unimernet_reference import _t, reference_bundle  # noqa: F401  (reference_bundle: the one bundle rule of the project)

VARIANTS = ("no rw", "swapped", "rel from scaled q", "pad keys masked", "zero pad keys")


def _attention(t, p, x, H, W, nh, ws, scale, rel_from="q", variant=None):
    import torch
    import torch.nn.functional as Fn
    B, L, C = x.shape
    dh = C // nh
    hb, wb = (-(-H // ws), -(-W // ws)) if ws else (1, 1)
    Hp, Wp = (hb * ws, wb * ws) if ws else (H, W)
    h, w = (ws, ws) if ws else (H, W)
    y = Fn.layer_norm(x, (C,), t[p + "ln1_g"], t[p + "ln1_b"], 1e-5).reshape(B, H, W, C)
    real = torch.ones(1, H, W, 1, dtype=torch.bool)
    if ws:
        y = Fn.pad(y, (0, 0, 0, Wp - W, 0, Hp - H))                                                # zeros, in front of the fused Linear
        real = Fn.pad(real, (0, 0, 0, Wp - W, 0, Hp - H))
        part = lambda a: a.reshape(a.shape[0], hb, ws, wb, ws, a.shape[-1]).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, a.shape[-1])
        y, real = part(y), part(real)
    else:
        y, real = y.reshape(B, H * W, C), real.reshape(1, H * W, 1)
    real = real[:, :, 0].repeat(B, 1)                                                             # [G', h w]: False for a padding token
    qkv = y @ t[p + "wqkv"].T + t[p + "bqkv"]                                                      # a padding token: the bias row
    if variant == "zero pad keys":
        qkv = qkv * real[:, :, None].to(qkv.dtype)
    qkv = qkv.reshape(-1, h * w, 3, nh, dh).permute(2, 0, 3, 1, 4).reshape(3, -1, h * w, dh)
    q, k, v = qkv[0], qkv[1], qkv[2]                                                              # [G, h w, dh], G = G' nh
    c = torch.tensor(np.float32(dh ** -0.5)).to(x.dtype)                                           # the graph's constant is the f32 dh^-0.5
    s = (q * c) @ k.transpose(1, 2) if scale == "pre" else (q @ k.transpose(1, 2)) * c
    rq = (q * c if rel_from == "scaled" or variant == "rel from scaled q" else q).reshape(-1, h, w, dh)
    Rh, Rw = t[p + "rh"], t[p + "rw"]
    if variant == "swapped":
        Rh, Rw = Rw, Rh                                                                           # (h = w only)
    rh = torch.einsum("ghwd,hkd->ghwk", rq, Rh)
    rw = torch.einsum("ghwd,wkd->ghwk", rq, Rw)
    if variant == "no rw":
        rw = torch.zeros_like(rw)
    s = (s.reshape(-1, h, w, h, w) + rh[..., None] + rw[..., None, :]).reshape(-1, h * w, h * w)
    if variant == "pad keys masked":
        s = s.masked_fill(~real.repeat_interleave(nh, 0)[:, None, :], float("-inf"))
    a = torch.softmax(s, -1)
    o = (a @ v).reshape(-1, nh, h, w, dh).permute(0, 2, 3, 1, 4).reshape(-1, h * w, C) @ t[p + "wp"].T + t[p + "bp"]
    if ws:
        o = o.reshape(-1, hb, wb, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, Hp, Wp, C)[:, :H, :W]
    return x + o.reshape(B, H * W, C)


def _block(t, p, x, H, W, nh, ws, scale, rel_from="q", variant=None):
    import torch.nn.functional as Fn
    C = x.shape[-1]
    x = _attention(t, p, x, H, W, nh, ws, scale, rel_from, variant)
    y = Fn.layer_norm(x, (C,), t[p + "ln2_g"], t[p + "ln2_b"], 1e-5)
    return x + (Fn.gelu(y @ t[p + "w1"].T + t[p + "b1"]) @ t[p + "w2"].T + t[p + "b2"])


def vit_block_reference(info, x, dtype="float64", variant=None):
    """build_vit_block's graph: x [B, H W, C] -> y"""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        t = _t(info["weights"], dt)
        f = _block if info["whole"] else _attention
        return f(t, "", torch.from_numpy(np.asarray(x)).to(dt), info["H"], info["W"], info["nh"], info["ws"], info["scale"], info.get("rel_from", "q"), variant).numpy()


def vary_vit_reference(we, x, dtype="float64", scale="pre", variant=None):
    """build_vary_vit's graph: x [B, 1, Hi, Wi] -> memory [B, S, D]; we: info["encoder"]"""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    with torch.no_grad():
        t = _t(we, dt)
        C, nh, ws = int(we["C"]), int(we["nh"]), int(we["ws"])
        h = Fn.conv2d(torch.from_numpy(np.asarray(x)).to(dt), t["pe_w"], t["pe_b"], stride=16)
        B, _, H, W = h.shape
        h = h.reshape(B, C, -1).transpose(1, 2) + t["pos"]
        for i in range(int(we["depth"])):
            h = _block(t, f"b{i}_", h, H, W, nh, 0 if i in we["global_blocks"] else ws, scale, "q", variant)
        m = h.transpose(1, 2).reshape(B, C, H, W)
        m = Fn.conv2d(Fn.conv2d(m, t["n1_w"], t["n1_b"]), t["n2_w"], t["n2_b"], stride=2, padding=1)
        m = m.reshape(B, m.shape[1], -1).transpose(1, 2)
        return (m @ t["fc_w"].T + t["fc_b"]).contiguous().numpy()
