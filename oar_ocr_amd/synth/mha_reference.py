"""Multi-head attention with separate q / k / v sources, the AIFI layer of RT-DETR's hybrid encoder and the graphs of synth.models that hold them
(build_mha, build_aifi_layer, build_table_cell_det(encoder_layers > 0)) restated in torch on the CPU, in f64 and f32, from the formulas:
o[n, t, h] = softmax_s(q[n, t, h] . k[n, s, h] * dh^-0.5) v[n, s, h], with einsum over named axes rather than the exported Reshape / Transpose list.
Used through unimernet_reference.reference_bundle: noise = max |f32 - f64|, tol = max(16 noise, 2^-19).

`variant` names a wrong reading of the block; tests/test_mha_attention_cpu.py shows that the inputs tell each from the right one."""
from __future__ import annotations

import numpy as np

from .unimernet_reference import reference_bundle  # noqa: F401  (re-exported for the tests)

VARIANTS = ("v from x + pos", "k without pos", "no scale", "heads merged in the wrong order", "softmax over the queries")


def _t(w, dt):
    import torch
    return {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in w.items() if isinstance(v, np.ndarray)}


def _attend(w, xq, xk, xv, nh, scale="post", mask=None, variant=None):
    """xq [N, Tq, D], xk and xv [N, Tk, D] (torch tensors of one dtype), w: torch weights q / k / v / o -> [N, Tq, D]"""
    import torch
    dt = xq.dtype
    N, Tq, D = xq.shape
    Tk, dh = xk.shape[1], D // nh
    lin = lambda t, nm: t @ w[nm + "_w"] + w[nm + "_b"]
    q, k, v = lin(xq, "q").reshape(N, Tq, nh, dh), lin(xk, "k").reshape(N, Tk, nh, dh), lin(xv, "v").reshape(N, Tk, nh, dh)
    c = torch.tensor(np.float32(dh ** -0.5)).to(dt)                                       # the graph's constant is the f32 dh^-0.5
    if variant == "no scale":
        s = torch.einsum("nthd,nshd->nhts", q, k)
    elif scale == "pre":
        s = torch.einsum("nthd,nshd->nhts", q * c, k)
    else:
        s = torch.einsum("nthd,nshd->nhts", q, k) * c
    if mask is not None:
        s = s + torch.from_numpy(np.ascontiguousarray(mask, np.float32)).to(dt)
    a = torch.softmax(s, -2 if variant == "softmax over the queries" else -1)
    if variant == "heads merged in the wrong order":
        o = torch.einsum("nhts,nshd->ntdh", a, v).reshape(N, Tq, D)
    else:
        o = torch.einsum("nhts,nshd->nthd", a, v).reshape(N, Tq, D)
    return lin(o, "o")


def _block(w, x, mem, pos, nh, self_attn, scale="post", mask=None, variant=None):
    """self-attention: q = k = x + pos, v = x; cross-attention: q = x + pos, k = v = mem"""
    xq = x if pos is None else x + pos
    if self_attn:
        return _attend(w, xq, x if variant == "k without pos" else xq, xq if variant == "v from x + pos" else x, nh, scale, mask, variant)
    return _attend(w, xq, mem, mem, nh, scale, mask, variant)


def mha_reference(info, x, mem=None, dtype="float64", variant=None):
    """build_mha's graph: -> y [N, Tq, D]"""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        w = _t(info["weights"], dt)
        xs = torch.from_numpy(np.asarray(x)).to(dt)
        ms = None if mem is None else torch.from_numpy(np.asarray(mem)).to(dt)
        pos = None if info["pos"] is None else torch.from_numpy(info["pos"]).to(dt)
        return _block(w, xs, ms, pos, info["nh"], info["self"], info["scale"], info.get("mask"), variant).contiguous().numpy()


def _aifi(w, src, H, W, D, nh, variant=None):
    import torch
    import torch.nn.functional as Fn
    from .models import sincos_2d
    lin = lambda t, nm: t @ w[nm + "_w"] + w[nm + "_b"]
    lnorm = lambda t, nm: Fn.layer_norm(t, (D,), w[nm + "_g"], w[nm + "_b"], 1e-5)
    pos = torch.from_numpy(sincos_2d(H, W, D)).to(src.dtype)                               # (the graph's table is f32)
    src = lnorm(src + _block(w, src, None, pos, nh, True, "post", None, variant), "ln1")
    return lnorm(src + lin(Fn.gelu(lin(src, "ffn1")), "ffn2"), "ln2")


def aifi_layer_reference(info, src, dtype="float64", variant=None):
    """build_aifi_layer's graph: src [N, H W, D] -> y"""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        return _aifi(_t(info["weights"], dt), torch.from_numpy(np.asarray(src)).to(dt), info["H"], info["W"], info["D"], info["nh"], variant).contiguous().numpy()


def aifi_stack_reference(aifi, src, dtype="float64"):
    """the AIFI layers of build_table_cell_det(encoder_layers > 0): aifi = info["aifi"], src = the tensor named aifi["in"] -> the tensor named aifi["out"]"""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        t = torch.from_numpy(np.asarray(src)).to(dt)
        for w in aifi["layers"]:
            t = _aifi(_t(w, dt), t, aifi["H"], aifi["W"], aifi["D"], aifi["nh"])
        return t.contiguous().numpy()
