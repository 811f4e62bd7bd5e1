"""The UniMERNet-shaped encoder of synth.models.build_unimernet restated in torch on the CPU, in f64 and f32: the stem, the Swin blocks (plain, padded,
shifted and masked windows: F.pad, torch.roll, the mask added per window, the crop; window partition, per-window multi-head attention with the additive relative-position bias, projection, window reverse; the depthwise "conv
enhance"; the MLP), patch merging and the final LayerNorm.  The decoder's reference is synth/formula_reference.py (it handles squeeze attention)."""
from __future__ import annotations

import numpy as np


def _t(w, dt):
    import torch
    return {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in w.items() if isinstance(v, np.ndarray)}


def _attention(t, p, x, H, W, nh, ws, scale, shift=0, mask=None, pad_value=0.0, unroll=None):
    """shift: an int, or (rows, columns); unroll: the reverse roll (default: the forward one); mask: None or [nW, N, N]; pad_value: what LN1's output is
    padded with at the bottom / right, in front of the Linears, where H or W is no multiple of ws"""
    import torch
    import torch.nn.functional as Fn
    B, L, C = x.shape
    N, dh = ws * ws, C // nh
    hb, wb = -(-H // ws), -(-W // ws)
    Hp, Wp = hb * ws, wb * ws
    sy, sx = shift if isinstance(shift, (tuple, list)) else (shift, shift)
    uy, ux = (sy, sx) if unroll is None else unroll if isinstance(unroll, (tuple, list)) else (unroll, unroll)
    y = Fn.layer_norm(x, (C,), t[p + "ln1_g"], t[p + "ln1_b"], 1e-5).reshape(B, H, W, C)
    y = Fn.pad(y, (0, 0, 0, Wp - W, 0, Hp - H), value=float(pad_value))
    y = torch.roll(y, (-sy, -sx), (1, 2))
    win = y.reshape(B, hb, ws, wb, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, C)
    heads = lambda nm: (win @ t[p + "w" + nm].T + t[p + "b" + nm]).reshape(-1, N, nh, dh).permute(0, 2, 1, 3)
    q, k, v = heads("q"), heads("k"), heads("v")
    s = q @ k.transpose(2, 3)
    if scale == "div":
        s = s / torch.tensor(np.float32(np.sqrt(dh))).to(x.dtype)                        # the graph's constant is the f32 sqrt(dh)
    else:
        s = s * torch.tensor(np.float32(dh ** -0.5)).to(x.dtype)
    s = s + t[p + "bias"][None]
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask, np.float32)).to(x.dtype)        # [nW, N, N]: the same for every image and head
        s = (s.reshape(B, -1, nh, N, N) + m[None, :, None]).reshape(-1, nh, N, N)
    a = torch.softmax(s, -1)
    o = (a @ v).permute(0, 2, 1, 3).reshape(-1, N, C) @ t[p + "wp"].T + t[p + "bp"]
    r = o.reshape(-1, hb, wb, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, Hp, Wp, C)
    r = torch.roll(r, (uy, ux), (1, 2))[:, :H, :W]
    return x + r.reshape(B, H * W, C)


def _block(t, p, x, H, W, nh, ws, scale, shift=0, mask=None, pad_value=0.0, unroll=None):
    import torch.nn.functional as Fn
    B, L, C = x.shape
    x = _attention(t, p, x, H, W, nh, ws, scale, shift, mask, pad_value, unroll)
    img = Fn.conv2d(x.transpose(1, 2).reshape(B, C, H, W), t[p + "ce_w"], t[p + "ce_b"], padding=1, groups=C)
    x = x + img.reshape(B, C, -1).transpose(1, 2)
    y = Fn.layer_norm(x, (C,), t[p + "ln2_g"], t[p + "ln2_b"], 1e-5)
    return x + (Fn.gelu(y @ t[p + "w1"].T + t[p + "b1"]) @ t[p + "w2"].T + t[p + "b2"])


def swin_block_reference(info, x, dtype="float64"):
    """build_swin_block's graph: x [B, H W, C] -> y; info's shift / unroll / mask / pad_value, where present, are the block's"""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        t = _t(info["weights"], dt)
        f = _block if info["whole"] else _attention
        return f(t, "", torch.from_numpy(np.asarray(x)).to(dt), info["H"], info["W"], info["nh"], info["ws"], info["scale"],
                 info.get("shift", 0), info.get("mask"), info.get("pad_value", 0.0), info.get("unroll")).numpy()


def unimernet_encoder_reference(we, x, dtype="float64", scale="div"):
    """build_unimernet's encoder: x [B, 1, H, W] -> memory [B, S, D]; we: info["encoder"]"""
    import torch
    import torch.nn.functional as Fn
    dt = getattr(torch, dtype)
    with torch.no_grad():
        t = _t(we, dt)
        from .models import swin_shift_mask
        C, heads, depths, ws = int(we["C"]), we["heads"], we["depths"], int(we["ws"])
        h = Fn.gelu(Fn.conv2d(torch.from_numpy(np.asarray(x)).to(dt), t["st_w1"], t["st_b1"], stride=2, padding=1))
        h = Fn.gelu(Fn.conv2d(h, t["st_w2"], t["st_b2"], stride=2, padding=1))
        B, _, H, W = h.shape
        h = h.reshape(B, C, -1).transpose(1, 2)
        for si in range(len(depths)):
            Cs = C << si
            for bi in range(depths[si]):
                sh = ws // 2 if we.get("shifted") and bi % 2 else 0                       # the odd blocks of a shifted encoder
                h = _block(t, f"s{si}b{bi}_", h, H, W, heads[si], ws, scale, sh, swin_shift_mask(H, W, ws, sh) if sh else None)
            if si + 1 < len(depths):
                h = h.reshape(B, H // 2, 2, W // 2, 2, Cs).permute(0, 1, 3, 2, 4, 5).reshape(B, -1, 4 * Cs)
                h = Fn.layer_norm(h, (4 * Cs,), t[f"m{si}_ln_g"], t[f"m{si}_ln_b"], 1e-5) @ t[f"m{si}_w"].T
                H, W = H // 2, W // 2
        D = C << (len(depths) - 1)
        return Fn.layer_norm(h, (D,), t["lnf_g"], t["lnf_b"], 1e-5).contiguous().numpy()


def reference_bundle(run, *args, **kw):
    """f64 reference, the f32 run of the same math, noise = max |f32 - f64| and tol = max(16 noise, 2^-19) (16: another reduction order and the device's
    exp / erf, each a few ulp)"""
    r64, r32 = run(*args, dtype="float64", **kw), run(*args, dtype="float32", **kw)
    noise = float(np.abs(r32.astype(np.float64) - r64).max())
    return {"f64": r64, "f32": r32, "noise": noise, "tol": max(16 * noise, 2.0 ** -19)}
