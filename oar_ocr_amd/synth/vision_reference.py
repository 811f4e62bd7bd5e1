"""Reference for the attention of the PaddleOCR-VL vision encoder (vis_attention.hip), in plain numpy from the formulas, not from any source.

The patches of several images are packed back to back: image i has grid (h_i, w_i) and takes h_i w_i rows, patch idx of an image sits at row = idx // w,
col = idx % w.  2-D rotary embedding with dh the head size:
    inv_freq[j] = theta^(-2 j / (dh / 2))  for j < dh / 4,
    angle[c]    = row inv_freq[c] for c < dh / 4,  col inv_freq[c - dh / 4] for dh / 4 <= c < dh / 2,
    x'[c] = x[c] cos(angle[c]) - x[c + dh/2] sin(angle[c]),   x'[c + dh/2] = x[c + dh/2] cos(angle[c]) + x[c] sin(angle[c])      (rotate_half),
then per (image, head)  o = softmax(dh^-0.5 (q' k'^T)) v  over the keys of the query's own image.

`vis_attention_core` is used through reference_bundle: noise = max |f32 - f64| of this very computation on the same inputs, tol = max(16 noise, 2^-19).
FAULTS names wrong readings of the attention; tests/test_vision_reference_cpu.py shows that the cases tell each from the right one by more than 100 tol.

The second half of the module is the whole vision stage in torch on the CPU, f64 and f32: patch Linear + bilinearly resampled position table, the pre-LN
layers, post_layernorm (the features), and the projector (LayerNorm eps 1e-5, 2 x 2 merge in the order (hb, wb, mi, mj, d), linear_1 + erf-GELU, linear_2: the
embeddings); ENCODER_CASES, make_vision (random weights under the checkpoint's names), ENCODER_FAULTS, and smart_resize / patchify / rope_index in plain loops."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from .unimernet_reference import reference_bundle  # noqa: F401  (the one bundle rule of the project, re-exported for the tests)

FAULTS = ("row and column swapped", "interleaved rotate_half", "frequencies over dh", "1-D rotary", "no block-diagonal", "scale applied twice")
HEAD_SIZES = (8, 24, 40, 56, 72, 80)                       # DH16 = 1, 2, 3, 4, 5 (partial), 5 (full)
SEGMENT_SETS = ((1,), (31, 32, 33), (64, 65), (4, 140))    # one token; the key-block edge; the query-tile edge; a partial tile, then three tiles with a 12-key tail


def grid_of(n):
    """(h, w) with h w = n and h the largest divisor of n not above sqrt(n): 140 -> (10, 14), 31 -> (1, 31)"""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def rotary_tables(grids, dh, theta=10000.0, dtype="float32", fault=None):
    """-> cos, sin [sum h w, dh / 2] in `dtype`: position and frequency are rounded to `dtype` first, and the angle, cos and sin are formed in it (float32: what
    the reference implementation does)."""
    assert dh % 8 == 0, dh
    dt = np.dtype(dtype)
    q = dh // 4
    denom = dh if fault == "frequencies over dh" else dh // 2
    inv = (1.0 / (np.float64(theta) ** (2.0 * np.arange(q, dtype=np.float64) / denom))).astype(dt)
    cs, sn = [], []
    for h, w in grids:
        idx = np.arange(h * w)
        row, col = (idx // w).astype(dt), (idx % w).astype(dt)
        if fault == "row and column swapped":
            row, col = col, row
        if fault == "1-D rotary":
            row = col = idx.astype(dt)
        ang = np.concatenate([row[:, None] * inv[None, :], col[:, None] * inv[None, :]], 1).astype(dt)
        cs.append(np.cos(ang).astype(dt)); sn.append(np.sin(ang).astype(dt))
    return np.concatenate(cs), np.concatenate(sn)


def rotate(x, cos, sin, fault=None):
    """x [T, nh, dh], cos / sin [T, dh / 2], in x's dtype"""
    h2 = x.shape[-1] // 2
    c, s = cos[:, None, :], sin[:, None, :]
    if fault == "interleaved rotate_half":                  # pairs (2 c, 2 c + 1) instead of (c, c + dh / 2)
        a, b = x[..., 0::2], x[..., 1::2]
        out = np.empty_like(x)
        out[..., 0::2], out[..., 1::2] = a * c - b * s, b * c + a * s
        return out
    a, b = x[..., :h2], x[..., h2:]
    return np.concatenate([a * c - b * s, b * c + a * s], -1)


def vis_attention_core(qkv, cos, sin, lens, nh, dh, dtype="float64", fault=None):
    """qkv [T, 3, nh, dh] (any array of T 3 nh dh numbers), cos / sin [T, dh / 2], lens: the images' token counts -> o [T, nh dh].  The tables are inputs: the
    kernel takes them in f32, so they are cast to the working dtype, not recomputed."""
    dt = np.dtype(dtype)
    T = int(sum(lens))
    qkv = np.asarray(qkv).astype(dt).reshape(T, 3, nh, dh)
    cos, sin = np.asarray(cos).astype(dt).reshape(T, dh // 2), np.asarray(sin).astype(dt).reshape(T, dh // 2)
    q, k, v = rotate(qkv[:, 0], cos, sin, fault), rotate(qkv[:, 1], cos, sin, fault), qkv[:, 2]
    scale = np.float32(dh ** -0.5).astype(dt)
    o = np.empty((T, nh * dh), dt)
    spans = [(0, T)] if fault == "no block-diagonal" else [(int(sum(lens[:i])), int(sum(lens[:i + 1]))) for i in range(len(lens))]
    for a, b in spans:
        s = np.einsum("qhd,khd->hqk", q[a:b], k[a:b]) * scale
        if fault == "scale applied twice":
            s = s * scale
        e = np.exp(s - s.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        o[a:b] = np.einsum("hqk,khd->qhd", p, v[a:b]).reshape(b - a, nh * dh)
    return o


def attention_case(dh, lens, nh=2, seed=0, fault=None):
    """The inputs of one direct kernel case -> dict(qkv [T, 3, nh, dh] f32, cos, sin f32, lens, grids, nh, dh): N(0, 1) projections with q and k at gain 2 (so
    the soft-max is far from uniform and a wrong angle shows), the rotary tables of grids with h w = len formed in f32."""
    rng = np.random.default_rng([seed, dh, nh] + list(lens))
    T = int(sum(lens))
    qkv = rng.standard_normal((T, 3, nh, dh))
    qkv[:, :2] *= 2.0
    grids = [grid_of(n) for n in lens]
    cos, sin = rotary_tables(grids, dh, dtype="float32", fault=fault)
    return dict(qkv=qkv.astype(np.float32), cos=cos, sin=sin, lens=tuple(lens), grids=grids, nh=nh, dh=dh)


def packed_layout(case, pad=0, off=0):
    """-> (buf, qkv_off, ld): the rows of qkv [T][3 nh dh] at a stride of ld = 3 nh dh + pad floats from float `off` on; with pad or off, every float outside
    the rows is a quiet NaN -- a value read from a gap makes the output non-finite"""
    T, D3 = case["qkv"].shape[0], 3 * case["nh"] * case["dh"]
    ld = D3 + pad
    buf = np.full(off + (T - 1) * ld + D3 + (16 if pad or off else 0), np.nan, np.float32)
    np.lib.stride_tricks.as_strided(buf[off:], (T, D3), (4 * ld, 4))[...] = case["qkv"].reshape(T, D3)
    return buf, off, ld


# ================================================================================== the whole vision stage
ENCODER_FAULTS = FAULTS + ("align_corners=True", "no clamp", "merge without permute", "pre_norm after merge", "erf and tanh exchanged")


@dataclass(frozen=True)
class VisCase:
    name: str
    D: int
    heads: int
    F: int
    L: int
    patch: int
    G: int
    text_hidden: int
    grids: Tuple[Tuple[int, int], ...]
    merge: int = 2
    act: str = "gelu_pytorch_tanh"
    eps: float = 1e-6
    seed: int = 5

    @property
    def dh(self):
        return self.D // self.heads

    @property
    def tokens(self):
        return sum(h * w for h, w in self.grids)


ENCODER_CASES = {c.name: c for c in (
    VisCase("P", 144, 2, 160, 2, 2, 5, 64, ((2, 2), (6, 10), (10, 14))),    # the real head size 72 (DH16 = 5, 8 idle components); T = 4, 60, 140; table up- and down-sampled, h != w
    VisCase("Q", 160, 2, 96, 1, 2, 3, 48, ((8, 8), (2, 34))),               # DH16 = 5 full; T = 64 exactly and 68
    VisCase("R", 24, 3, 40, 1, 2, 4, 40, ((4, 8), (6, 6), (4, 4))),         # DH16 = 1, dh / 4 = 2; T = 32, 36; h = w = G: the identity interpolation
    VisCase("S", 80, 2, 96, 1, 4, 3, 48, ((2, 34), (8, 8))),                # DH16 = 3 partial, dh / 4 = 10: a row / column boundary inside a float4; K = 48
    VisCase("K", 72, 1, 100, 1, 14, 2, 40, ((2, 4),)),                      # the real patch Linear, K = 588
    # The exchange of the erf and the tanh GELU differs by at most 4.7e-4 per element and moves the five cases above by at most 27 tol; small sums and a seed
    # picked for it (2, out of 0..11) make it 160 tol here.
    VisCase("G", 16, 1, 16, 1, 2, 2, 8, ((2, 2),), seed=2),
)}


def make_vision(case: VisCase, seed: int = None) -> Dict[str, np.ndarray]:
    """Random f32 weights under the checkpoint's names.  Matrices N(0, 1) / sqrt(K); q and k at gain 2 so the soft-max is far from uniform; LayerNorm weights
    around 1; the position table N(0, 1) so that a wrong resampling shows."""
    rng = np.random.default_rng([case.seed if seed is None else seed, case.D, case.heads, case.L])
    f = lambda a: np.ascontiguousarray(a, np.float32)   # noqa: E731
    mat = lambda n, k, gain=1.0: f(rng.standard_normal((n, k)) * gain / np.sqrt(k))   # noqa: E731
    vec = lambda n, s=0.1: f(rng.standard_normal(n) * s)   # noqa: E731
    D, F, p, m2 = case.D, case.F, case.patch, case.merge ** 2
    vm = "visual.vision_model."
    w = {vm + "embeddings.patch_embedding.weight": mat(D, 3 * p * p).reshape(D, 3, p, p), vm + "embeddings.patch_embedding.bias": vec(D),
         vm + "embeddings.position_embedding.weight": f(rng.standard_normal((case.G * case.G, D)))}
    for i in range(case.L):
        pre = vm + f"encoder.layers.{i}."
        for ln in ("layer_norm1", "layer_norm2"):
            w[pre + ln + ".weight"], w[pre + ln + ".bias"] = f(1.0 + 0.1 * rng.standard_normal(D)), vec(D)
        for name, gain in (("q_proj", 2.0), ("k_proj", 2.0), ("v_proj", 1.0), ("out_proj", 1.0)):
            w[pre + f"self_attn.{name}.weight"], w[pre + f"self_attn.{name}.bias"] = mat(D, D, gain), vec(D)
        w[pre + "mlp.fc1.weight"], w[pre + "mlp.fc1.bias"] = mat(F, D, 2.0), vec(F)
        w[pre + "mlp.fc2.weight"], w[pre + "mlp.fc2.bias"] = mat(D, F), vec(D)
    w[vm + "post_layernorm.weight"], w[vm + "post_layernorm.bias"] = f(1.0 + 0.1 * rng.standard_normal(D)), vec(D)
    w["mlp_AR.pre_norm.weight"], w["mlp_AR.pre_norm.bias"] = f(1.0 + 0.1 * rng.standard_normal(D)), vec(D)
    w["mlp_AR.linear_1.weight"], w["mlp_AR.linear_1.bias"] = mat(m2 * D, m2 * D, 2.0), vec(m2 * D)
    w["mlp_AR.linear_2.weight"], w["mlp_AR.linear_2.bias"] = mat(case.text_hidden, m2 * D), vec(case.text_hidden)
    return w


def make_pixels(case: VisCase, seed: int = None) -> np.ndarray:
    """[T, 3 p p] f32 in [-1, 1): what preprocess_images yields for mean = std = 0.5"""
    return np.random.default_rng([case.seed if seed is None else seed, 77, case.tokens]).uniform(-1.0, 1.0, (case.tokens, 3 * case.patch ** 2)).astype(np.float32)


def resample_table(table, G, h, w, fault=None):
    """table [G G, D] (torch) -> [h w, D]: bilinear, align_corners = false, source coordinate clamped to [0, G - 1]; plain loops"""
    t = table.reshape(G, G, -1)

    def axis(o, out):
        c = (o * (G - 1) / (out - 1) if out > 1 else 0.0) if fault == "align_corners=True" else (o + 0.5) * G / out - 0.5
        if fault != "no clamp":
            c = min(max(c, 0.0), G - 1.0)
        i0 = min(max(math.floor(c), 0), max(G - 2, 0))     # (without the clamp the weight c - i0 leaves [0, 1]: the border rows are extrapolated)
        return i0, c - i0
    rows = []
    for oy in range(h):
        y0, wy = axis(oy, h)
        for ox in range(w):
            x0, wx = axis(ox, w)
            y1, x1 = min(y0 + 1, G - 1), min(x0 + 1, G - 1)
            rows.append(t[y0, x0] * ((1 - wy) * (1 - wx)) + t[y0, x1] * ((1 - wy) * wx) + t[y1, x0] * (wy * (1 - wx)) + t[y1, x1] * (wy * wx))
    import torch
    return torch.stack(rows)


def vision_forward(case: VisCase, weights, pixels, dtype="float64", fault=None, grids=None):
    """-> (features [T, D], embeds [T / merge^2, text_hidden]) as numpy arrays of `dtype`.  grids: another composition than the case's (pixels must match it)."""
    import torch
    import torch.nn.functional as Fn
    td = torch.float64 if dtype == "float64" else torch.float32
    W = {k: torch.from_numpy(np.asarray(v, np.float32)).to(td) for k, v in weights.items()}
    grids = tuple(case.grids if grids is None else grids)
    vm = "visual.vision_model."
    D, nh, dh, m = case.D, case.heads, case.dh, case.merge
    lens = [h * w for h, w in grids]
    T = sum(lens)
    x = torch.from_numpy(np.asarray(pixels, np.float32)).to(td).reshape(T, -1)
    lin = lambda v, name: v @ W[name + ".weight"].reshape(W[name + ".weight"].shape[0], -1).T + W[name + ".bias"]   # noqa: E731
    ln = lambda v, name, eps: Fn.layer_norm(v, (v.shape[-1],), W[name + ".weight"], W[name + ".bias"], eps)          # noqa: E731
    gelu = {"tanh": lambda v: Fn.gelu(v, approximate="tanh"), "erf": lambda v: Fn.gelu(v)}
    enc_act, proj_act = ("tanh" if case.act != "gelu" else "erf"), "erf"
    if fault == "erf and tanh exchanged":
        enc_act, proj_act = ("erf" if enc_act == "tanh" else "tanh"), "tanh"
    pos = torch.cat([resample_table(W[vm + "embeddings.position_embedding.weight"], case.G, h, w, fault) for h, w in grids])
    x = lin(x, vm + "embeddings.patch_embedding") + pos
    table_fault = fault if fault in ("row and column swapped", "frequencies over dh", "1-D rotary") else None
    core_fault = fault if fault in ("interleaved rotate_half", "no block-diagonal", "scale applied twice") else None
    cos, sin = rotary_tables(grids, dh, dtype=dtype, fault=table_fault)
    for i in range(case.L):
        pre = vm + f"encoder.layers.{i}."
        y = ln(x, pre + "layer_norm1", case.eps)
        qkv = torch.stack([lin(y, pre + "self_attn." + n) for n in ("q_proj", "k_proj", "v_proj")], 1).reshape(T, 3, nh, dh)
        att = torch.from_numpy(vis_attention_core(qkv.numpy(), cos, sin, lens, nh, dh, dtype=dtype, fault=core_fault)).to(td)
        x = x + lin(att, pre + "self_attn.out_proj")
        y = ln(x, pre + "layer_norm2", case.eps)
        x = x + lin(gelu[enc_act](lin(y, pre + "mlp.fc1")), pre + "mlp.fc2")
    feat = ln(x, vm + "post_layernorm", case.eps)

    def merge(v):
        out, start = [], 0
        for h, w in grids:
            g = v[start:start + h * w].reshape(h // m, m, w // m, m, -1)
            if fault == "merge without permute":
                out.append(g.reshape(h * w // (m * m), -1))                   # (hb, mi, wb, mj) taken as it lies
            else:
                out.append(g.permute(0, 2, 1, 3, 4).reshape(h * w // (m * m), -1))
            start += h * w
        return torch.cat(out)
    if fault == "pre_norm after merge":
        g = merge(feat)                                                      # the norm over the merged row of m^2 D, weight and bias repeated
        mu, var = g.mean(-1, keepdim=True), g.var(-1, unbiased=False, keepdim=True)
        mg = (g - mu) / torch.sqrt(var + 1e-5) * W["mlp_AR.pre_norm.weight"].repeat(m * m) + W["mlp_AR.pre_norm.bias"].repeat(m * m)
    else:
        mg = merge(ln(feat, "mlp_AR.pre_norm", 1e-5))
    emb = lin(gelu[proj_act](lin(mg, "mlp_AR.linear_1")), "mlp_AR.linear_2")
    return feat.numpy(), emb.numpy()


def vision_bundle(case: VisCase, weights, pixels, grids=None):
    """the project's rule, separately for the features and the embeddings: {feat, emb} -> {f64, f32, noise, tol}"""
    f64, e64 = vision_forward(case, weights, pixels, "float64", grids=grids)
    f32, e32 = vision_forward(case, weights, pixels, "float32", grids=grids)
    out = {}
    for key, a, b in (("feat", f64, f32), ("emb", e64, e32)):
        noise = float(np.abs(b.astype(np.float64) - a).max())
        out[key] = {"f64": a, "f32": b, "noise": noise, "tol": max(16 * noise, 2.0 ** -19)}
    return out


# ------------------------------------------------------------------------------------------------ preprocessing and positions, in plain loops
def smart_resize_ref(height, width, factor, min_pixels, max_pixels):
    """A second spelling in exact arithmetic where the other uses f64 tricks: rounding to the factor by integer arithmetic on twice the value (half away from
    zero), floor and ceil of a / (f b) by comparing squares of integers -- floor(h / (beta f)) with beta^2 = h w / max is the largest n with n^2 f^2 h w <= h^2 max.
    Errors as ValueError.  (The f64 square root can differ from this only where the quotient is an integer to within an ulp; no such size is among the tests.)"""
    h, w, f = int(height), int(width), int(factor)
    if max(h, w) > 200 * min(h, w):
        raise ValueError("aspect ratio")
    hb, wb = ((2 * h + f) // (2 * f)) * f, ((2 * w + f) // (2 * f)) * f
    if hb * wb > max_pixels:
        def down(side):                                    # floor(side / (beta f)), beta^2 = h w / max_pixels
            n = 0
            while (n + 1) ** 2 * f * f * h * w <= side * side * max_pixels:
                n += 1
            return max(n, 1) * f
        hb, wb = down(h), down(w)
        if hb * wb < min_pixels:
            raise ValueError("cannot satisfy")
    elif hb * wb < min_pixels:
        def up(side):                                      # ceil(side beta / f), beta^2 = min_pixels / (h w)
            n = 0
            while n * n * f * f * h * w < side * side * min_pixels:
                n += 1
            return max(n, 1) * f
        hb, wb = up(h), up(w)
        if hb * wb > max_pixels:
            raise ValueError("cannot satisfy")
    return hb, wb


def patchify_ref(img_u8, patch, rescale, mean, std):
    """[H, W, 3] u8 -> [H/p W/p, 3 p p] f32 by the naive loop over (patch, c, dy, dx): v * rescale, then (v - mean) / std, in f32"""
    H, W, _ = img_u8.shape
    gh, gw = H // patch, W // patch
    out = np.zeros((gh * gw, 3 * patch * patch), np.float32)
    for i in range(gh * gw):
        gy, gx = divmod(i, gw)
        n = 0
        for c in range(3):
            for dy in range(patch):
                for dx in range(patch):
                    v = np.float32(img_u8[gy * patch + dy, gx * patch + dx, c]) * np.float32(rescale)
                    out[i, n] = (v - np.float32(mean[c])) / np.float32(std[c])
                    n += 1
    return out


def rope_index_ref(ids, grids, image_id, start_id, merge):
    """positions [3, T] and the delta, token by token: a counter `nxt` = largest position so far + 1; a text token takes (nxt, nxt, nxt); the n-th image token
    run takes (base, base + hh, base + ww) over its merged grid with base = nxt at its first token"""
    pairs = sum(1 for a, b in zip(ids[:-1], ids[1:]) if a == start_id and b == image_id)
    if pairs != len(grids):
        raise ValueError("image count mismatch")
    pos, big, i, n = [], -1, 0, 0
    while i < len(ids):
        if ids[i] == image_id and n < len(grids):
            lh, lw = grids[n][0] // merge, grids[n][1] // merge
            base = big + 1
            for k in range(lh * lw):
                pos.append((base, base + k // lw, base + k % lw))
            big = max(big, base + max(lh, lw) - 1)
            i += lh * lw
            n += 1
        else:
            pos.append((big + 1,) * 3)
            big += 1
            i += 1
    return np.asarray(pos, np.int64).T, big + 1 - len(ids)


# ------------------------------------------------------------------------------------------------ composite case PA: vision case P in front of LM case A
PA_SEED = 0                      # (the first seed tried: every free-running step's f64 margin exceeds 4 tol)
PA_IDS = dict(image=91, start=90, end=92, prefix=(3, 90), suffix=(92, 7, 8))    # inside LM case A's vocabulary of 97
PA_GRIDS = ((6, 10), (2, 2))     # 15 and 1 image tokens
PA_STEPS = 24
_PA = {}


def composite_reference():
    """Two sequences, one image each (u8 images of 12 x 20 and 4 x 4 pixels, patch 2, no resize), through vision case P's encoder and projector (one image at a
    time, as the reference implementation runs them) into LM case A's geometry: ids = prefix + image tokens + suffix, the embedding rows with the image span
    replaced, positions from rope_index_ref; the f64 greedy run of PA_STEPS tokens, the f32 run teacher-forced with them, noise and tol over the logits.
    -> dict(vis_case, lm_case, weights, images, runs [(tokens, logits64)], noise, tol, margins)"""
    if _PA:
        return _PA
    import torch
    from . import lm_reference as lr
    vc = VisCase("PA", 144, 2, 160, 2, 2, 5, 64, PA_GRIDS, seed=PA_SEED)
    lc = lr.CASES["A"]
    w = {**make_vision(vc), **lr.make_lm(lc, PA_SEED)}
    rng = np.random.default_rng([PA_SEED, 4242])
    images = [rng.integers(0, 256, (h * 2, wd * 2, 3), dtype=np.uint8) for h, wd in PA_GRIDS]
    r64, r32 = lr.RefLM(lc, w, torch.float64), lr.RefLM(lc, w, torch.float32)
    runs, noise, margins = [], 0.0, []
    for img, grid in zip(images, PA_GRIDS):
        px = patchify_ref(img, 2, 1.0 / 255.0, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        n_img = grid[0] * grid[1] // 4
        ids = list(PA_IDS["prefix"]) + [PA_IDS["image"]] * n_img + list(PA_IDS["suffix"])
        pos, _ = rope_index_ref(ids, [grid], PA_IDS["image"], PA_IDS["start"], 2)
        outs = []
        for dtype, lm in (("float64", r64), ("float32", r32)):
            _, emb = vision_forward(vc, w, px, dtype, grids=(grid,))
            x = lm.embed(ids).clone()
            x[2:2 + n_img] = torch.from_numpy(emb).to(x.dtype)
            outs.append(x)
        t64, l64 = _gen(r64, outs[0], pos, None)
        _, l32 = _gen(r32, outs[1], pos, t64)
        noise = max(noise, float((l32.double() - l64).abs().max()))
        top = torch.topk(l64, 2, dim=-1).values
        margins.append((top[:, 0] - top[:, 1]).numpy())
        runs.append((t64, l64.numpy(), ids, pos))
    _PA.update(vis_case=vc, lm_case=lc, weights=w, images=images, runs=runs, noise=noise, tol=max(16.0 * noise, 2.0 ** -19), margins=np.stack(margins))
    return _PA


def _gen(lm, x, pos, forced):
    """RefLM.generate on embeddings kept in the model's own dtype (its inputs_embeds argument goes through f32)"""
    import torch
    T = x.shape[0]
    pos3 = torch.as_tensor(np.asarray(pos, np.int64))
    nxt = int(pos3.max()) + 1
    cache = [None] * lm.c.L
    h = lm.forward_chunk(x, pos3, cache)[-1:]
    toks, logs = [], []
    for i in range(PA_STEPS):
        lg = lm.logits_of(h)[0]
        logs.append(lg)
        tok = int((lg == lg.max()).nonzero()[0, 0])
        toks.append(tok)
        if i + 1 == PA_STEPS:
            break
        feed = tok if forced is None else int(forced[i])
        h = lm.forward_chunk(lm.embed([feed]), torch.full((3, 1), nxt + i, dtype=torch.int64), cache)
    assert T == pos3.shape[1]
    return np.asarray(toks, np.int64), torch.stack(logs)
