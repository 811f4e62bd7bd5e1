"""Multi-scale deformable attention and the RT-DETR-shaped decoder of synth.models (build_deformable_attention, build_rtdetr_decoder) restated in torch on
the CPU, in f64 and f32.  The core follows PaddleDetection's deformable_attention_core_func: per level the value is viewed as [N nh, c, h, w], sampled with
grid_sample(bilinear, zeros, align_corners = False) at 2 loc - 1, and the L P samples are summed with the (softmax) weights.  Used through
unimernet_reference.reference_bundle: noise = max |f32 - f64|, tol = max(16 noise, 2^-19)."""
from __future__ import annotations

import numpy as np


def _t(w, dt):
    import torch
    return {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in w.items() if isinstance(v, np.ndarray)}


def _core(value, loc, logit, nh, levels, P, weights="softmax", align_corners=0):
    """value [N, Lv, nh c], loc [N, Q, nh, L, P, 2], logit [N, Q, nh L P] (torch tensors of one dtype) -> [N, Q, nh c]"""
    import torch
    import torch.nn.functional as Fn
    N, Lv, D = value.shape
    Q, L, c = loc.shape[1], len(levels), D // nh
    w = logit.reshape(N, Q, nh, L * P)
    if weights == "softmax":
        w = torch.softmax(w, -1)
    w = w.permute(0, 2, 1, 3).reshape(N * nh, 1, Q, L * P)
    grid = 2 * loc - 1
    samples, start = [], 0
    for l, (h, wd) in enumerate(levels):
        v = value[:, start:start + h * wd].reshape(N, h * wd, nh * c).permute(0, 2, 1).reshape(N * nh, c, h, wd)
        gl = grid[:, :, :, l].permute(0, 2, 1, 3, 4).reshape(N * nh, Q, P, 2)
        samples.append(Fn.grid_sample(v, gl, mode="bilinear", padding_mode="zeros", align_corners=bool(align_corners)))
        start += h * wd
    s = torch.stack(samples, 3).reshape(N * nh, c, Q, L * P)
    return (s * w).sum(-1).reshape(N, nh * c, Q).permute(0, 2, 1)


def deformable_attention_inputs(info, seed=0):
    """value ~ N(0, 1); logit ~ 3 N(0, 1), a peaked softmax, so that a tap taken from another level, point or head moves the output by O(1) (weights = "input":
    that softmax itself, in f32); loc ~ U(-0.3, 1.3) with every 17th coordinate set to 0, 0.5 or 1 in turn: about a third of the coordinates lie outside the
    image, and the borders and the centre are hit exactly"""
    rng = np.random.default_rng(seed)
    N, Q, nh, c, L, P = info["N"], info["Q"], info["nh"], info["c"], len(info["levels"]), info["P"]
    Lv = sum(h * w for h, w in info["levels"])
    value = rng.standard_normal((N, Lv, nh * c)).astype(np.float32)
    logit = (3.0 * rng.standard_normal((N, Q, nh * L * P))).astype(np.float32)
    loc = rng.uniform(-0.3, 1.3, (N, Q, nh, L, P, 2)).astype(np.float32)
    flat = loc.reshape(-1)
    flat[::17] = np.resize(np.array([0.0, 0.5, 1.0], np.float32), flat[::17].shape)
    if info["weights"] == "input":
        z = logit.reshape(N, Q, nh, L * P)
        e = np.exp(z - z.max(-1, keepdims=True))
        logit = (e / e.sum(-1, keepdims=True)).astype(np.float32).reshape(N, Q, nh * L * P)
    return value, loc, logit


def deformable_attention_reference(info, value, loc, logit, dtype="float64"):
    """build_deformable_attention's graph: -> y [N, Q, nh c]"""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        a = [torch.from_numpy(np.asarray(x)).to(dt) for x in (value, loc, logit)]
        return _core(*a, info["nh"], info["levels"], info["P"], info["weights"], info.get("align_corners", 0)).contiguous().numpy()


def rtdetr_decoder_layers(w, memory, tgt, ref_logit, D, nh, levels, P, layers):
    """_rtdetr_decoder's layers on torch tensors: -> [(out, ref_logit)] per layer.  w: torch weights (rtdetr_decoder_weights through _t)"""
    import torch
    import torch.nn.functional as Fn
    dt = tgt.dtype
    N, Q, _ = tgt.shape
    dh, L = D // nh, len(levels)
    f32c = lambda v: torch.tensor(np.float32(v)).to(dt)                                  # the graph's constants are f32
    lin = lambda t, nm: t @ w[nm + "_w"] + w[nm + "_b"]
    lnorm = lambda t, nm: Fn.layer_norm(t, (D,), w[nm + "_g"], w[nm + "_b"], 1e-5)
    heads = lambda t: t.reshape(N, Q, nh, dh).permute(0, 2, 1, 3)
    outs = []
    for i in range(layers):
        p = f"l{i}_"
        ref = torch.sigmoid(ref_logit)
        pos = lin(torch.relu(lin(ref, "pos1")), "pos2")
        qk = tgt + pos
        sc = (heads(lin(qk, p + "sa_q")) @ heads(lin(qk, p + "sa_k")).transpose(2, 3)) * f32c(dh ** -0.5)
        sa = lin((torch.softmax(sc, -1) @ heads(lin(tgt, p + "sa_v"))).permute(0, 2, 1, 3).reshape(N, Q, D), p + "sa_o")
        tgt = lnorm(tgt + sa, p + "ln1")
        query = tgt + pos
        value = lin(memory, p + "value")
        offs = lin(query, p + "offs").reshape(N, Q, nh, L, P, 2)
        logit = lin(query, p + "attw")
        xy, wh = ref[:, :, None, None, None, 0:2], ref[:, :, None, None, None, 2:4]
        loc = xy + offs / f32c(float(P)) * wh * f32c(0.5)
        tgt = lnorm(tgt + lin(_core(value, loc, logit, nh, levels, P), p + "out"), p + "ln2")
        tgt = lnorm(tgt + lin(torch.relu(lin(tgt, p + "ffn1")), p + "ffn2"), p + "ln3")
        ref_logit = lin(torch.relu(lin(tgt, p + "box1")), p + "box2") + ref_logit
        outs.append((tgt, ref_logit))
    return outs


def rtdetr_decoder_reference(info, memory, tgt, ref_logit, dtype="float64", want="boxes"):
    """build_rtdetr_decoder's graph: -> the output named `want` ("boxes", "logits", "out<i>", "ref<i>")"""
    import torch
    dt = getattr(torch, dtype)
    with torch.no_grad():
        w = _t(info["weights"], dt)
        m, t, r = (torch.from_numpy(np.asarray(x)).to(dt) for x in (memory, tgt, ref_logit))
        outs = rtdetr_decoder_layers(w, m, t, r, info["D"], info["nh"], info["levels"], info["P"], info["layers"])
        if want == "boxes":
            y = torch.sigmoid(outs[-1][1])
        elif want == "logits":
            y = outs[-1][0] @ w["cls_w"] + w["cls_b"]
        elif want.startswith("out"):
            y = outs[int(want[3:])][0]
        elif want.startswith("ref"):
            y = torch.sigmoid(outs[int(want[3:])][1])
        else:
            raise ValueError(want)
        return y.contiguous().numpy()
