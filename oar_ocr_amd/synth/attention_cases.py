"""References, input families and layouts for the direct tests of the two flash-attention kernels (mha_attention.hip, relpos_attention.hip).

`mha_core` and `relpos_core` are the attention alone, in plain numpy from the formulas in kernels.h: every score of a key set exists as one array and the
soft-max is taken over it at once -- no key blocks, no running maximum.  Used through reference_bundle: noise = max |f32 - f64|, tol = max(16 noise, 2^-19).

`flash_emulate` is the opposite: the kernels' key loop restated in f32 numpy (32-key blocks, a key past the end reads the last key, running maximum and
sum) on the same flat buffer / offsets / row strides the kernel entry point takes, with switches that break it one way each.
tests/test_flash_attention_cases_cpu.py uses it to show that the input families below tell each broken loop from the right one."""
from __future__ import annotations

import numpy as np

from .unimernet_reference import reference_bundle  # noqa: F401  (the one bundle rule of the project, re-exported for the tests)

FAMILIES = ("normal", "rising", "falling", "equal")
LAYOUTS = ("dense", "qk_fused", "qkv_fused", "padded")
FAULTS = ("no tail mask", "sum not rescaled", "maximum frozen", "row stride ignored", "image stride ignored")
RAMP = 200.0     # the scaled score of `rising` / `falling` runs from -RAMP to +RAMP over the keys; f32 expf overflows at 89


def scale_of(dh):
    """the graph's constant: dh^-0.5 rounded to f32"""
    return np.float32(dh ** -0.5)


def _softmax(s):
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def mha_core(q, k, v, scale, scale_pre, dtype="float64"):
    """q [N, Tq, nh, dh], k and v [N, Tk, nh, dh] -> o [N, Tq, nh dh] = softmax_s(scaled q . k_s) v_s per (image, head).  scale: the f32 constant, cast to
    the working dtype; scale_pre: it multiplies q in front of the product, otherwise the scores."""
    dt = np.dtype(dtype)
    q, k, v = (np.asarray(a).astype(dt) for a in (q, k, v))
    c = np.float32(scale).astype(dt)
    q, k, v = (a.transpose(0, 2, 1, 3) for a in (q, k, v))                                                    # [N, nh, T, dh]
    s = (q * c) @ k.transpose(0, 1, 3, 2) if scale_pre else (q @ k.transpose(0, 1, 3, 2)) * c                 # [N, nh, Tq, Tk]
    N, nh, Tq, dh = q.shape
    return np.ascontiguousarray((_softmax(s) @ v).transpose(0, 2, 1, 3).reshape(N, Tq, nh * dh))


def relpos_core(qkv, rh, rw, bqkv, B, H, W, ws, nh, dh, scale, scale_pre, dtype="float64"):
    """qkv [B H W, 3, nh, dh] (tokens in image order), rh [gh, dh, gh], rw [gw, dh, gw] (query row / column, component, key row / column) with (gh, gw) =
    (ws, ws) or (H, W), bqkv [3, nh, dh] or None -> o [B H W, nh dh].  ws > 0: the grid is padded at the bottom / right to multiples of ws and cut into
    ws x ws windows; a padding token is a key with bqkv's k / v rows (None: zeros) that takes part in the soft-max, and as a query it has no output row.
    score[(qy, qx), (ky, kx)] = scaled q . k + q . rh[qy, :, ky] + q . rw[qx, :, kx], the UNSCALED q in both bias terms."""
    dt = np.dtype(dtype)
    gh, gw = (ws, ws) if ws else (H, W)
    hb, wb = -(-H // gh), -(-W // gw)
    Hp, Wp = hb * gh, wb * gw
    rh, rw = np.asarray(rh).astype(dt).reshape(gh, dh, gh), np.asarray(rw).astype(dt).reshape(gw, dh, gw)
    grid = np.zeros((B, Hp, Wp, 3, nh, dh), dt)
    if bqkv is not None:
        grid[...] = np.asarray(bqkv).astype(dt).reshape(3, nh, dh)
    grid[:, :H, :W] = np.asarray(qkv).astype(dt).reshape(B, H, W, 3, nh, dh)
    win = grid.reshape(B, hb, gh, wb, gw, 3, nh, dh).transpose(0, 1, 3, 2, 4, 5, 6, 7).reshape(-1, gh, gw, 3, nh, dh)     # [G, gh, gw, 3, nh, dh]
    G, T = win.shape[0], gh * gw
    q, k, v = (win[:, :, :, i].reshape(G, T, nh, dh).transpose(0, 2, 1, 3) for i in range(3))               # [G, nh, T, dh], token t = y gw + x
    c = np.float32(scale).astype(dt)
    s = (q * c) @ k.transpose(0, 1, 3, 2) if scale_pre else (q @ k.transpose(0, 1, 3, 2)) * c                 # [G, nh, T, T]
    q5 = q.reshape(G, nh, gh, gw, dh)
    bh, bw = np.einsum("ghyxd,ydv->ghyxv", q5, rh), np.einsum("ghyxd,xdu->ghyxu", q5, rw)                     # q . rh[qy, :, ky], q . rw[qx, :, kx]
    s = (s.reshape(G, nh, gh, gw, gh, gw) + bh[..., :, None] + bw[..., None, :]).reshape(G, nh, T, T)
    o = (_softmax(s) @ v).transpose(0, 2, 1, 3).reshape(B, hb, wb, gh, gw, nh * dh).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, nh * dh)
    return np.ascontiguousarray(o[:, :H, :W].reshape(B * H * W, nh * dh))


# ------------------------------------------------------------------------------------------------ input families (all f32, seeded)
def _unit(rng, *shape):
    u = rng.standard_normal(shape)
    return u / np.linalg.norm(u, axis=-1, keepdims=True)


def _ramp(n):
    """-1 .. +1 over n keys (a single key: -1)"""
    return 2.0 * np.arange(n) / max(n - 1, 1) - 1.0


def mha_inputs(family, N, Tq, Tk, nh, dh, seed=0):
    """-> q [N, Tq, nh, dh], k, v [N, Tk, nh, dh].
    normal: all N(0, 1).  rising: per head a unit vector u, q = 0.25 N(0,1) + sqrt(dh) u and k_s = 0.25 N(0,1) + RAMP (2 s / (Tk - 1) - 1) u, so the scaled
    score climbs from about -RAMP to +RAMP with the key index and every block raises the running maximum.  falling: the ramp reversed -- the first keys
    dominate and later blocks underflow to 0.  equal: k = 0, so the soft-max is uniform and o is the mean of v over exactly Tk keys."""
    assert family in FAMILIES, family
    rng = np.random.default_rng([seed, N, Tq, Tk, nh, dh, FAMILIES.index(family)])
    q, k, v = rng.standard_normal((N, Tq, nh, dh)), rng.standard_normal((N, Tk, nh, dh)), rng.standard_normal((N, Tk, nh, dh))
    if family in ("rising", "falling"):
        u = _unit(rng, nh, dh)
        ramp = _ramp(Tk) * (RAMP if family == "rising" else -RAMP)
        q = 0.25 * q + np.sqrt(dh) * u
        k = 0.25 * k + ramp[None, :, None, None] * u[None, None]
    elif family == "equal":
        k = np.zeros_like(k)
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def relpos_inputs(family, B, H, W, nh, dh, ws, seed=0, bias=True):
    """-> qkv [B H W, 3, nh, dh], rh [gh, dh, gh], rw [gw, dh, gw], bqkv [3, nh, dh] (None without `bias`).
    normal: qkv and bqkv N(0, 1), the tables N(0, 1) / sqrt(dh) (each bias term is O(1) like the scaled product).  rising: one unit vector u (the tables
    have no head axis), q = 0.25 N(0,1) + sqrt(dh) u, k = 0.25 N(0,1) and rh[qy, :, ky] = RAMP (2 ky / (gh - 1) - 1) / sqrt(dh) u: the bias term
    q . rh climbs from about -RAMP to +RAMP with the key row -- the ramp goes through the bias path."""
    assert family in ("normal", "rising"), family
    rng = np.random.default_rng([seed, B, H, W, nh, dh, ws, FAMILIES.index(family)])
    gh, gw = (ws, ws) if ws else (H, W)
    qkv = rng.standard_normal((B * H * W, 3, nh, dh))
    rh, rw = rng.standard_normal((gh, dh, gh)) / np.sqrt(dh), rng.standard_normal((gw, dh, gw)) / np.sqrt(dh)
    bqkv = rng.standard_normal((3, nh, dh))
    if family == "rising":
        u = _unit(rng, dh)
        qkv[:, 0] = 0.25 * qkv[:, 0] + np.sqrt(dh) * u
        qkv[:, 1] *= 0.25
        rh = np.broadcast_to((RAMP / np.sqrt(dh)) * u[None, :, None] * _ramp(gh)[None, None, :], (gh, dh, gh)).copy()
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(qkv), f(rh), f(rw), (f(bqkv) if bias else None)


# ------------------------------------------------------------------------------------------------ layouts of q / k / v in one flat buffer
def mha_layout(layout, q, k, v):
    """-> dict(buf, q_off, k_off, v_off, ldq, ldk, ldv): the views the kernel entry point takes.  dense: three contiguous tensors back to back.  qk_fused:
    q and k are the halves of one [N, T, 2 D] block (ld = 2 D), v follows.  qkv_fused: one [N, T, 3 D] block.  padded: ldq = D + 4, ldk = D + 8, ldv =
    D + 12, non-zero offsets, and every float outside the three views is a quiet NaN -- a value read from a gap makes the output non-finite."""
    assert layout in LAYOUTS, layout
    N, Tq, nh, dh = q.shape
    Tk, D = k.shape[1], nh * dh
    q2, k2, v2 = q.reshape(N * Tq, D), k.reshape(N * Tk, D), v.reshape(N * Tk, D)
    if layout == "dense":
        return dict(buf=np.concatenate([q2.ravel(), k2.ravel(), v2.ravel()]), q_off=0, k_off=q2.size, v_off=q2.size + k2.size, ldq=D, ldk=D, ldv=D)
    if layout == "qk_fused":
        assert Tq == Tk
        return dict(buf=np.concatenate([np.concatenate([q2, k2], 1).ravel(), v2.ravel()]), q_off=0, k_off=D, v_off=2 * q2.size, ldq=2 * D, ldk=2 * D, ldv=D)
    if layout == "qkv_fused":
        assert Tq == Tk
        return dict(buf=np.concatenate([q2, k2, v2], 1).ravel(), q_off=0, k_off=D, v_off=2 * D, ldq=3 * D, ldk=3 * D, ldv=3 * D)
    ldq, ldk, ldv = D + 4, D + 8, D + 12
    q_off = 8
    k_off = q_off + (N * Tq - 1) * ldq + D + 12
    v_off = k_off + (N * Tk - 1) * ldk + D + 12
    buf = np.full(v_off + (N * Tk - 1) * ldv + D + 16, np.nan, np.float32)
    for a, off, ld in ((q2, q_off, ldq), (k2, k_off, ldk), (v2, v_off, ldv)):
        rows = a.shape[0]
        np.lib.stride_tricks.as_strided(buf[off:], (rows, D), (4 * ld, 4))[...] = a
    return dict(buf=buf, q_off=q_off, k_off=k_off, v_off=v_off, ldq=ldq, ldk=ldk, ldv=ldv)


# ------------------------------------------------------------------------------------------------ the key loop, in f32 numpy, with fault switches
def flash_emulate(buf, q_off, k_off, v_off, ldq, ldk, ldv, N, Tq, Tk, nh, dh, scale, scale_pre, fault=None, block=32):
    """The kernels' key loop on the entry point's own arguments -> o [N, Tq, nh dh] f32.  Per (image, head): keys in blocks of `block`, a key past the end
    reads the last key and its score is -inf, m = running maximum, l = running sum, both rescaled by exp(m_old - m_new) per block.  fault (FAULTS):
    'no tail mask' keeps the scores of the keys past the end; 'sum not rescaled' adds a block's sum to l as it is; 'maximum frozen' keeps the first
    block's maximum; 'row stride ignored' reads the rows of k and v at ld = nh dh; 'image stride ignored' starts image b of k and v at b Tk nh dh."""
    assert fault is None or fault in FAULTS, fault
    f32 = np.float32
    buf = np.asarray(buf, f32).reshape(-1)
    D = nh * dh
    c = f32(scale)
    post = f32(1.0) if scale_pre else c
    o = np.zeros((N, Tq, D), f32)

    def rows(off, ld, T, b, head, idx, kv):
        row_ld = D if (kv and fault == "row stride ignored") else ld
        img = b * T * (D if (kv and fault == "image stride ignored") else ld)
        at = off + img + idx[:, None] * row_ld + head * dh + np.arange(dh)[None, :]
        return buf[at]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for b in range(N):
            for head in range(nh):
                q = rows(q_off, ldq, Tq, b, head, np.arange(Tq), False)
                if scale_pre:
                    q = q * c
                m = np.full(Tq, -np.inf, f32)
                l = np.zeros(Tq, f32)
                acc = np.zeros((Tq, dh), f32)
                for kb in range(-(-Tk // block)):
                    n = kb * block + np.arange(block)
                    idx = np.minimum(n, Tk - 1)
                    s = (q @ rows(k_off, ldk, Tk, b, head, idx, True).T).astype(f32) * post
                    if fault != "no tail mask":
                        s[:, n >= Tk] = -np.inf
                    m_new = np.maximum(m, s.max(1)) if (kb == 0 or fault != "maximum frozen") else m
                    alpha = np.exp(m - m_new).astype(f32)
                    p = np.exp(s - m_new[:, None]).astype(f32)
                    l = (l if fault == "sum not rescaled" else l * alpha) + p.sum(1, dtype=f32)
                    acc = acc * alpha[:, None] + (p @ rows(v_off, ldv, Tk, b, head, idx, True)).astype(f32)
                    m = m_new
                o[b, :, head * dh:(head + 1) * dh] = acc / l[:, None]
    return o
