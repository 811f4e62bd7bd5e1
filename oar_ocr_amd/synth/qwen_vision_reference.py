"""Reference for the Qwen2-VL and Qwen2.5-VL vision towers (qvis_host.cc, qvis_misc.hip), in numpy from the formulas, in f32 and f64.

Patches arrive in MERGE-GROUPED order (hb, wb, mi, mj) -- the m x m patches of a merge unit lie next to each other -- and a patch's values in (c, tp, dy, dx)
order.  x = patches W^T (no bias, no position table).  Rotary tables as in vision_reference (inv_freq[j] = theta^(-2 j / (dh / 2)), j < dh / 4; angle =
position x frequency; [row part | column part]), but the position of a row is the patch's own (row, column) in that merge-grouped order.
Block, kind "qwen2":   x += proj(attention(qkv(LN(x))));  x += fc2(act(fc1(LN(x))))        LayerNorm eps 1e-6, act quick_gelu by default
Block, kind "qwen2_5": x += proj(attention(qkv(RMS(x)))); x += down(act(gate(RMS(x))) up(RMS(x)))   RMSNorm eps 1e-6, act silu by default; the merge units are
    permuted into window order first (window_plan), the rotary tables with them; blocks in `fullatt` attend over one segment per image, the others over the windows.
Merger: ln_q (LayerNorm / RMSNorm), m^2 consecutive rows as one, mlp.0 + erf GELU, mlp.2; for qwen2_5 the merged rows go back to raster order (reverse_index).
The features are the last block's output in the caller's order.  hidden_act: "quick_gelu" x sigmoid(1.702 x); "gelu", "gelu_new", "gelu_pytorch_tanh" all the
ERF GELU (as the reference implementation maps them); "silu".

qvision_bundle: the project's rule, tol = max(16 noise, 2^-19) with noise = max |f32 - f64| of this model on the same case.  FAULTS: wrong readings, each
named for the case that tells it apart (tests/test_qwen_vision_reference_cpu.py: by more than 4 tol)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from .vision_reference import rotate, smart_resize_ref, vis_attention_core  # noqa: F401

ERF_NAMES = ("gelu", "gelu_new", "gelu_pytorch_tanh")
ACTS = ("quick_gelu", "silu") + ERF_NAMES

FAULTS = {   # fault -> the case named for it
    "raster rotary positions": "A2",
    "rotary positions not permuted with the windows": "W5",
    "no reverse permutation": "W5",
    "window segments in a full-attention block": "W5",
    "full attention in a windowed block": "W5",
    "full attention across the whole call": "A2",
    "LayerNorm where RMSNorm belongs": "W5",
    "gate and up exchanged": "X5",
    "quick_gelu and erf GELU exchanged": "A2",
    "the second temporal frame zero": "A2",
}


EPS_FAULT = "eps inside the mean's divisor"      # not in FAULTS: it shows only on rows whose mean(x^2) is near eps (the cases' pixels scaled by EPS_FAULT_SCALE)
EPS_FAULT_SCALE = 1e-3


@dataclass(frozen=True)
class QvisCase:
    name: str
    kind: str                      # "qwen2" | "qwen2_5"
    D: int
    heads: int
    F: int
    L: int
    grids: Tuple[Tuple[int, int], ...]
    act: str = "quick_gelu"
    out_hidden: int = 48
    patch: int = 2
    temporal: int = 2
    channels: int = 3
    merge: int = 2
    window_size: int = 0
    fullatt: Tuple[int, ...] = ()
    seed: int = 5

    @property
    def dh(self):
        return self.D // self.heads

    @property
    def K(self):
        return self.channels * self.temporal * self.patch ** 2

    @property
    def tokens(self):
        return sum(h * w for h, w in self.grids)


QVIS_CASES = {c.name: c for c in (
    QvisCase("A2", "qwen2", 160, 2, 320, 2, ((2, 2), (6, 10), (10, 14))),                                   # the real head size 80; T = 4, 60, 140
    QvisCase("B2", "qwen2", 24, 3, 36, 1, ((4, 8), (6, 6)), act="gelu"),                                   # dh 8; the erf GELU in fc1's epilogue
    QvisCase("K2", "qwen2", 72, 1, 144, 1, ((2, 4),), act="silu", patch=14),                               # the real patch Linear, K = 1176
    QvisCase("W5", "qwen2_5", 160, 2, 200, 3, ((14, 14), (16, 16), (4, 4)), act="silu", window_size=16, fullatt=(1,)),   # window side 4 units: 64-patch windows
    QvisCase("X5", "qwen2_5", 24, 3, 40, 2, ((4, 36), (6, 6)), act="silu", window_size=8),                 # 16-patch windows, an elongated grid with a partial last window
)}


def make_qvision(case: QvisCase, seed: int = None, prefix: str = "visual.") -> Dict[str, np.ndarray]:
    """Random f32 weights under the checkpoint's names.  Matrices N(0, 1) / sqrt(K); q and k rows at gain 2 so the soft-max is far from uniform; norm weights
    around 1; the patch weight 5-D, as a checkpoint has it."""
    rng = np.random.default_rng([case.seed if seed is None else seed, case.D, case.heads, case.L, len(case.name)])
    f = lambda a: np.ascontiguousarray(a, np.float32)   # noqa: E731
    mat = lambda n, k, gain=1.0: f(rng.standard_normal((n, k)) * gain / np.sqrt(k))   # noqa: E731
    vec = lambda n, s=0.1: f(rng.standard_normal(n) * s)   # noqa: E731
    D, F, m2, q5 = case.D, case.F, case.merge ** 2, case.kind == "qwen2_5"
    w = {prefix + "patch_embed.proj.weight": mat(D, case.K).reshape(D, case.channels, case.temporal, case.patch, case.patch)}

    def norm(name):
        w[name + ".weight"] = f(1.0 + 0.1 * rng.standard_normal(D))
        if not q5:
            w[name + ".bias"] = vec(D)
    for i in range(case.L):
        pre = prefix + f"blocks.{i}."
        norm(pre + "norm1"); norm(pre + "norm2")
        qkv = mat(3 * D, D)
        qkv[:2 * D] *= 2.0
        w[pre + "attn.qkv.weight"], w[pre + "attn.qkv.bias"] = qkv, vec(3 * D)
        w[pre + "attn.proj.weight"], w[pre + "attn.proj.bias"] = mat(D, D), vec(D)
        if q5:
            w[pre + "mlp.gate_proj.weight"], w[pre + "mlp.gate_proj.bias"] = mat(F, D, 2.0), vec(F)
            w[pre + "mlp.up_proj.weight"], w[pre + "mlp.up_proj.bias"] = mat(F, D, 2.0), vec(F)
            w[pre + "mlp.down_proj.weight"], w[pre + "mlp.down_proj.bias"] = mat(D, F), vec(D)
        else:
            w[pre + "mlp.fc1.weight"], w[pre + "mlp.fc1.bias"] = mat(F, D, 2.0), vec(F)
            w[pre + "mlp.fc2.weight"], w[pre + "mlp.fc2.bias"] = mat(D, F), vec(D)
    norm(prefix + "merger.ln_q")
    w[prefix + "merger.mlp.0.weight"], w[prefix + "merger.mlp.0.bias"] = mat(m2 * D, m2 * D, 2.0), vec(m2 * D)
    w[prefix + "merger.mlp.2.weight"], w[prefix + "merger.mlp.2.bias"] = mat(case.out_hidden, m2 * D), vec(case.out_hidden)
    return w


def make_qpixels(case: QvisCase, seed: int = None, grids=None) -> np.ndarray:
    """[T, K] f32 in [-1, 1), the two temporal frames equal (what preprocess_images_qwen yields for one image)"""
    grids = case.grids if grids is None else grids
    T = sum(h * w for h, w in grids)
    one = np.random.default_rng([case.seed if seed is None else seed, 77, T]).uniform(-1.0, 1.0, (T, case.channels, 1, case.patch ** 2)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(one, case.temporal, 2)).reshape(T, case.K)


# ------------------------------------------------------------------------------------------------ the window plan and the positions
def window_plan(grids, merge, patch, window_size):
    """-> (window_index, reverse_index, segments [(start, len)] in patches).  window_side = window_size / (merge patch) merge units; every image is cut into
    windows of that side, each dimension padded up (partial windows at the lower and right edge); a window without a unit gives no segment; the units of an image
    are offset by those of the images in front of it.  grids: (h, w) or (t, h, w) with t = 1."""
    unit = merge * patch
    if merge <= 0 or patch <= 0 or window_size <= 0 or window_size % unit:
        raise ValueError(f"window_size ({window_size}) must be a positive multiple of merge * patch ({unit})")
    side, m2 = window_size // unit, merge * merge
    index, segs, base, at = [], [], 0, 0
    for g in grids:
        h, w = g[-2], g[-1]
        uh, uw = h // merge, w // merge
        for wh in range(-(-uh // side)):
            for ww in range(-(-uw // side)):
                rows = range(wh * side, min((wh + 1) * side, uh))
                cols = range(ww * side, min((ww + 1) * side, uw))
                ids = [base + r * uw + c for r in rows for c in cols]
                if ids:
                    index += ids
                    segs.append((at, len(ids) * m2))
                    at += len(ids) * m2
        base += uh * uw
    index = np.asarray(index, np.int64)
    reverse = np.empty_like(index)
    reverse[index] = np.arange(index.size)
    return index, reverse, segs


def vision_position_ids(t, h, w, merge):
    """(row, column) of every patch in merge-grouped order (hb, wb, mi, mj), by the naive loop"""
    hp, wp = [], []
    for _ in range(t):
        for hb in range(h // merge):
            for wb in range(w // merge):
                for mi in range(merge):
                    for mj in range(merge):
                        hp.append(hb * merge + mi); wp.append(wb * merge + mj)
    return hp, wp


def qrotary_tables(grids, merge, dh, theta=10000.0, dtype="float32", window_index=None, fault=None):
    """-> cos, sin [T, dh / 2] in `dtype` (position and frequency rounded to it first), rows in the order the tokens run through the blocks"""
    dt = np.dtype(dtype)
    q = dh // 4
    inv = (1.0 / (np.float64(theta) ** (2.0 * np.arange(q, dtype=np.float64) / (dh // 2)))).astype(dt)
    hp, wp = [], []
    for h, w in grids:
        if fault == "raster rotary positions":
            a, b = [i // w for i in range(h * w)], [i % w for i in range(h * w)]
        else:
            a, b = vision_position_ids(1, h, w, merge)
        hp += a; wp += b
    hp, wp = np.asarray(hp), np.asarray(wp)
    if window_index is not None and fault != "rotary positions not permuted with the windows":
        m2 = merge * merge
        order = (np.asarray(window_index)[:, None] * m2 + np.arange(m2)[None, :]).reshape(-1)
        hp, wp = hp[order], wp[order]
    ang = np.concatenate([hp.astype(dt)[:, None] * inv[None, :], wp.astype(dt)[:, None] * inv[None, :]], 1).astype(dt)
    return np.cos(ang).astype(dt), np.sin(ang).astype(dt)


# ------------------------------------------------------------------------------------------------ the towers
def _erf(x):
    import torch
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def act_fn(name, x):
    """in x's dtype"""
    dt = x.dtype
    if name == "quick_gelu":
        return (x / (1.0 + np.exp(-(dt.type(1.702) * x)))).astype(dt)
    if name == "silu":
        return (x / (1.0 + np.exp(-x))).astype(dt)
    if name in ERF_NAMES:
        return (dt.type(0.5) * x * (1.0 + _erf(x * dt.type(math.sqrt(0.5))))).astype(dt)
    raise ValueError(f"unsupported vision hidden_act {name!r}")


def layer_norm(x, g, b, eps=1e-6):
    dt = x.dtype
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + dt.type(eps)) * g
    return (y + b if b is not None else y).astype(dt)


def rms_norm(x, g, eps=1e-6, eps_in_divisor=False):
    """eps_in_divisor: the wrong reading (sum(x^2) + eps) / D"""
    dt = x.dtype
    ms = ((x * x).sum(-1, keepdims=True) + dt.type(eps)) / dt.type(x.shape[-1]) if eps_in_divisor else (x * x).mean(-1, keepdims=True) + dt.type(eps)
    return (x / np.sqrt(ms) * g).astype(dt)


def qvision_forward(case: QvisCase, weights, pixels, dtype="float64", fault=None, grids=None, prefix="visual."):
    """-> (features [T, D] in the caller's order, embeds [T / m^2, out_hidden] in raster order of the merged grids), numpy arrays of `dtype`"""
    dt = np.dtype(dtype)
    W = {k[len(prefix):]: np.asarray(v, np.float32).astype(dt) for k, v in weights.items() if k.startswith(prefix)}
    grids = tuple(case.grids if grids is None else grids)
    D, nh, dh, m2, q5 = case.D, case.heads, case.dh, case.merge ** 2, case.kind == "qwen2_5"
    lens = [h * w for h, w in grids]
    T = sum(lens)
    lin = lambda v, name: (v @ W[name + ".weight"].T + W[name + ".bias"]).astype(dt)   # noqa: E731
    px = np.asarray(pixels, np.float32).astype(dt).reshape(T, -1)
    if fault == "the second temporal frame zero":
        px = px.reshape(T, case.channels, case.temporal, -1).copy()
        px[:, :, 1:] = 0
        px = px.reshape(T, -1)
    x = (px @ W["patch_embed.proj.weight"].reshape(D, -1).T).astype(dt)
    index = reverse = None
    win_lens = None
    if q5:
        index, reverse, segs = window_plan(grids, case.merge, case.patch, case.window_size)
        win_lens = [n for _, n in segs]
        x = x.reshape(T // m2, m2, D)[index].reshape(T, D)
    cos, sin = qrotary_tables(grids, case.merge, dh, dtype=dtype, window_index=index, fault=fault)
    act = case.act
    if fault == "quick_gelu and erf GELU exchanged":
        act = "gelu" if act == "quick_gelu" else "quick_gelu"
    use_ln = not q5 or fault == "LayerNorm where RMSNorm belongs"

    def norm(v, name):
        if use_ln:
            return layer_norm(v, W[name + ".weight"], W.get(name + ".bias"))
        return rms_norm(v, W[name + ".weight"], eps_in_divisor=fault == EPS_FAULT)
    for i in range(case.L):
        pre = f"blocks.{i}."
        full = not q5 or i in case.fullatt
        if fault == "window segments in a full-attention block" and q5 and full:
            full = False
        elif fault == "full attention in a windowed block" and q5 and not full:
            full = True
        seg = lens if full else win_lens
        if fault == "full attention across the whole call" and full:
            seg = [T]
        qkv = lin(norm(x, pre + "norm1"), pre + "attn.qkv")
        x = x + lin(vis_attention_core(qkv, cos, sin, seg, nh, dh, dtype=dtype), pre + "attn.proj")
        y = norm(x, pre + "norm2")
        if q5:
            g, u = ("up_proj", "gate_proj") if fault == "gate and up exchanged" else ("gate_proj", "up_proj")
            x = x + lin(act_fn(act, lin(y, pre + "mlp." + g)) * lin(y, pre + "mlp." + u), pre + "mlp.down_proj")
        else:
            x = x + lin(act_fn(act, lin(y, pre + "mlp.fc1")), pre + "mlp.fc2")
    feat = x
    if q5:
        feat = np.empty_like(x).reshape(T // m2, m2, D)
        feat[index] = x.reshape(T // m2, m2, D)
        feat = feat.reshape(T, D)
    mg = norm(x, "merger.ln_q").reshape(T // m2, m2 * D)
    emb = lin(act_fn("gelu", lin(mg, "merger.mlp.0")), "merger.mlp.2")
    if q5 and fault != "no reverse permutation":
        emb = emb[reverse]
    return feat, emb


def qvision_bundle(case: QvisCase, weights, pixels, grids=None):
    """the project's rule, separately for the features and the embeddings: {feat, emb} -> {f64, f32, noise, tol}"""
    f64, e64 = qvision_forward(case, weights, pixels, "float64", grids=grids)
    f32, e32 = qvision_forward(case, weights, pixels, "float32", grids=grids)
    out = {}
    for key, a, b in (("feat", f64, f32), ("emb", e64, e32)):
        noise = float(np.abs(b.astype(np.float64) - a).max())
        out[key] = {"f64": a, "f32": b, "noise": noise, "tol": max(16 * noise, 2.0 ** -19)}
    return out


# ------------------------------------------------------------------------------------------------ preprocessing, in plain loops
def patchify_qwen_ref(img_u8, patch, merge, temporal, rescale, mean, std, second_frame=None):
    """[H, W, 3] u8 -> [H/p W/p, 3 temporal p p] f32 by the naive loop: patches in (hb, wb, mi, mj) order, a patch's values in (c, tp, dy, dx) order; v * rescale,
    then (v - mean) / std, in f32; the one frame repeated `temporal` times"""
    H, W, _ = img_u8.shape
    gh, gw = H // patch, W // patch
    out = np.zeros((gh * gw, 3 * temporal * patch * patch), np.float32)
    i = 0
    for hb in range(gh // merge):
        for wb in range(gw // merge):
            for mi in range(merge):
                for mj in range(merge):
                    gy, gx, n = hb * merge + mi, wb * merge + mj, 0
                    for c in range(3):
                        for tp in range(temporal):
                            for dy in range(patch):
                                for dx in range(patch):
                                    v = np.float32(img_u8[gy * patch + dy, gx * patch + dx, c]) * np.float32(rescale)
                                    out[i, n] = (v - np.float32(mean[c])) / np.float32(std[c])
                                    n += 1
                    i += 1
    return out


# ------------------------------------------------------------------------------------------------ composite cases: a tower in front of a Qwen2-style decoder
# MA: the qwen2 tower, NA: the qwen2_5 tower, each in front of a small decoder with q / k / v biases and an M-RoPE section.  Three u8 images (patch 2, no resize),
# ids = prefix + image tokens + suffix.  The seeds are the first (of 0, 1, 2, ...) at which the f64 run alone keeps a greedy margin above 2 tol at every step
# and, for MA under no_repeat_ngram_size = 3, a margin above 4 r tol with at least one token per sequence changed by the ban (composite_conditions;
# tests/test_qwen_vision_reference_cpu.py asserts them).
COMPOSITE_IDS = dict(image=91, start=90, end=92, prefix=(3, 90), suffix=(92, 7, 8))    # inside the decoder's vocabulary of 97
COMPOSITE_STEPS = 24
COMPOSITE_NGRAM = 3
COMPOSITES = {
    "MA": (QvisCase("MA", "qwen2", 80, 2, 160, 2, ((6, 10), (2, 2), (4, 8)), out_hidden=64), 0),
    "NA": (QvisCase("NA", "qwen2_5", 80, 2, 96, 2, ((6, 10), (4, 4), (8, 6)), act="silu", out_hidden=64, window_size=8, fullatt=(1,)), 0),
}
_COMPOSITE = {}


def composite_lm_case():
    from . import lm_reference as lr
    return lr.LmCase("QA", 64, 2, 4, 2, 16, 96, 97, (2, 3, 3), qkv_bias=True)


def composite_reference(name: str, seed: int = None):
    """-> dict(vis_case, lm_case, weights, images, runs [(tokens, logits64, ids, pos)], ngram_runs (MA: lm_logits_cases._generate_rows' dicts), noise, tol, margins):
    the f64 greedy run of COMPOSITE_STEPS tokens per image, the f32 run teacher-forced with them, noise and tol over the logits (DESIGN 4.41's composite rule)"""
    vc, default_seed = COMPOSITES[name]
    seed = default_seed if seed is None else seed
    if (name, seed) in _COMPOSITE:
        return _COMPOSITE[(name, seed)]
    import torch
    from . import lm_logits_cases as ll
    from . import lm_reference as lr
    from .vision_reference import _gen, rope_index_ref
    lc = composite_lm_case()
    w = {**make_qvision(vc, seed), **lr.make_lm(lc, seed)}
    rng = np.random.default_rng([seed, 4243, len(name)])
    images = [rng.integers(0, 256, (h * vc.patch, wd * vc.patch, 3), dtype=np.uint8) for h, wd in vc.grids]
    px = np.concatenate([patchify_qwen_ref(im, vc.patch, vc.merge, vc.temporal, 1.0 / 255.0, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)) for im in images])
    embs = {dt: qvision_forward(vc, w, px, dt)[1] for dt in ("float64", "float32")}
    r64, r32 = lr.RefLM(lc, w, torch.float64), lr.RefLM(lc, w, torch.float32)
    runs, ngram_runs, noise, margins, off = [], [], 0.0, [], 0
    n_pre = len(COMPOSITE_IDS["prefix"])
    for grid in vc.grids:
        n_img = grid[0] * grid[1] // vc.merge ** 2
        ids = list(COMPOSITE_IDS["prefix"]) + [COMPOSITE_IDS["image"]] * n_img + list(COMPOSITE_IDS["suffix"])
        pos, _ = rope_index_ref(ids, [grid], COMPOSITE_IDS["image"], COMPOSITE_IDS["start"], vc.merge)
        xs = []
        for dt, lm in (("float64", r64), ("float32", r32)):
            x = lm.embed(ids).clone()
            x[n_pre:n_pre + n_img] = torch.from_numpy(embs[dt][off:off + n_img]).to(x.dtype)
            xs.append(x)
        off += n_img
        t64, l64 = _gen(r64, xs[0], pos, None)
        _, l32 = _gen(r32, xs[1], pos, t64)
        noise = max(noise, float((l32.double() - l64).abs().max()))
        top = torch.topk(l64, 2, dim=-1).values
        margins.append((top[:, 0] - top[:, 1]).numpy())
        runs.append((t64, l64.numpy(), ids, pos))
        if name == "MA":
            ngram_runs.append(ll._generate_rows(r64, xs[0], pos, ids, COMPOSITE_STEPS, 1.0, COMPOSITE_NGRAM))
    out = dict(vis_case=vc, lm_case=lc, weights=w, images=images, runs=runs, ngram_runs=ngram_runs, noise=noise, tol=max(16.0 * noise, 2.0 ** -19), margins=np.stack(margins))
    _COMPOSITE[(name, seed)] = out
    return out


def composite_conditions(ref) -> dict:
    """least greedy margin / (2 tol) (must exceed 1); with the n-gram runs: least processed margin / (4 r tol), r = 1 (must exceed 1) and the fewest tokens of a
    sequence that the ban changed (must be at least 1)"""
    out = dict(margin_ratio=float(ref["margins"].min()) / (2.0 * ref["tol"]))
    if ref["ngram_runs"]:
        out["ngram_margin_ratio"] = min(float(g["margin"].min()) for g in ref["ngram_runs"]) / (4.0 * ref["tol"])
        out["least_changed"] = min(int((g["tokens"] != g["raw_argmax"]).sum()) for g in ref["ngram_runs"])
    return out
