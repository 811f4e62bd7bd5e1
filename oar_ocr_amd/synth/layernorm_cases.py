"""Residual add + LayerNorm (csrc/add_layernorm.hip): input families, the f64 reference and an f32 numpy restatement of the kernel's row
routine with switches that break it one way each, for tests/test_layernorm_cases_cpu.py (no GPU) and tests/test_gpu_add_layernorm_kernel.py.

The operation: a [rows, C], b [b_rows, C] with b_rows | rows, s = f32(a + b[r % b_rows]), y = (s - mean) / sqrt(var + eps) * gamma + beta over each row.
The reference takes the f32 sum as given (it is what the kernel stores and what a separate Add would have written) and normalises it in f64.
Tolerance, as elsewhere in the project: noise = max |f32 numpy - f64| on the same inputs, tol = max(16 noise, 2^-19)."""
from __future__ import annotations

import numpy as np

FAMILIES = ("normal", "offset", "cancel", "periodic")
FAULTS = ("residual ignored", "b row not modulo", "padded lanes counted", "rows reduced together", "sum written after", "eps dropped")
#          rows C  b_rows      (4 | C <= 1024: the half-wave form; C = 30, 65, 1028: the one-wave form)
SHAPES = [(7, 32, 7), (15, 132, 5), (9, 260, 1), (17, 384, 17), (8, 1024, 4), (6, 30, 3), (5, 65, 5), (4, 1028, 2)]


def inputs(family, rows, C, b_rows, seed=0):
    """-> a [rows, C], b [b_rows, C], gamma [C], beta [C], all f32.
      normal    a, b ~ N(0, 1)
      offset    every row of a sits at about 50 with unit spread (a mean over the wrong count, or a sum stored after the normalisation, shows)
      cancel    b = -a (its first b_rows rows) + 1e-3 N(0, 1): the sum is tiny next to either operand, so an ignored residual and a dropped eps
                (the variance is about 1e-6) both show
      periodic  the rows of b differ in scale (row i: (1 + i) N(0, 1)), so reading another row of b shows"""
    if family not in FAMILIES:
        raise ValueError(family)
    if rows % b_rows:
        raise ValueError("b_rows must divide rows")
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((rows, C))
    b = rng.standard_normal((b_rows, C))
    if family == "offset":
        a = a + 50.0 + rng.standard_normal((rows, 1))
        b = 0.5 * b
    elif family == "cancel":
        b = -a[:b_rows].astype(np.float32).astype(np.float64) + 1e-3 * b
    elif family == "periodic":
        b = b * (1.0 + np.arange(b_rows))[:, None]
    gamma = 1.0 + 0.3 * rng.standard_normal(C)
    beta = 0.2 * rng.standard_normal(C)
    return tuple(np.ascontiguousarray(v, np.float32) for v in (a, b, gamma, beta))


def f32_sum(a, b, b_rows):
    """what the kernel stores as the sum: a + b[r % b_rows] in f32"""
    rows = a.shape[0]
    return (a.astype(np.float32) + b.astype(np.float32)[np.arange(rows) % b_rows]).astype(np.float32)


def ln_of_sum(a, b, b_rows, gamma, beta, eps, dtype="float64"):
    """LN(f32(a + b)) gamma + beta in `dtype` (numpy's own reductions); gamma / beta may be None"""
    s = f32_sum(a, b, b_rows).astype(dtype)
    d = s - s.mean(-1, keepdims=True)
    y = d / np.sqrt((d * d).mean(-1, keepdims=True) + np.asarray(eps, dtype))
    if gamma is not None:
        y = y * gamma.astype(dtype)
    if beta is not None:
        y = y + beta.astype(dtype)
    return y


def reference_bundle(a, b, b_rows, gamma, beta, eps):
    r64, r32 = ln_of_sum(a, b, b_rows, gamma, beta, eps), ln_of_sum(a, b, b_rows, gamma, beta, eps, "float32")
    noise = float(np.abs(r32.astype(np.float64) - r64).max())
    return {"f64": r64, "f32": r32, "sum": f32_sum(a, b, b_rows), "noise": noise, "tol": max(16 * noise, 2.0 ** -19)}


def takes_v4(C, offsets=()):
    """the half-wave form: 4 | C <= 1024 and every pointer on 16 bytes (offsets in floats)"""
    return C % 4 == 0 and C <= 1024 and all(o % 4 == 0 for o in offsets)


def _butterfly(v, width):
    """v [rows, lanes] f32 -> after xor-shuffles of width/2 .. 1 every lane of a group of `width` holds the group's sum, in the kernel's order"""
    lanes = v.shape[1]
    idx = np.arange(lanes)
    o = width // 2
    while o > 0:
        v = (v + v[:, idx ^ o]).astype(np.float32)
        o //= 2
    return v


def emulate(a, b, b_rows, gamma, beta, eps, fault=None, v4=None):
    """-> (y, s) as the kernel computes them, in f32 with its order of operations.  v4 (default: takes_v4(C)): the half-wave form -- lane l of 32 holds the
    float4s l, l + 32, ..; per lane (x + y) + (z + w) accumulated over them; a 32-lane butterfly; mean = sum * (1 / C); the centred squares the same way;
    inv = 1 / sqrt(q * (1 / C) + eps).  Otherwise the one-wave form: lane l of 64 takes the elements l, l + 64, .. one at a time; a 64-lane butterfly;
    mean = sum / C.  fault: one of FAULTS ("padded lanes counted" and "rows reduced together" only exist in the half-wave form)."""
    if fault is not None and fault not in FAULTS:
        raise ValueError(fault)
    f32 = np.float32
    rows, C = a.shape
    v4 = takes_v4(C) if v4 is None else v4
    r = np.arange(rows)
    brow = np.minimum(r, b_rows - 1) if fault == "b row not modulo" else r % b_rows
    s = a.astype(f32) if fault == "residual ignored" else (a.astype(f32) + b.astype(f32)[brow]).astype(f32)
    e = f32(0.0 if fault == "eps dropped" else eps)
    if v4:
        nv = (C // 4 + 31) // 32
        nv = nv if nv <= 4 else 8
        pad = np.zeros((rows, nv * 128), f32)
        pad[:, :C] = s
        q4 = pad.reshape(rows, nv, 32, 4)                                  # [row][i][lane][component]
        live = (np.arange(nv * 128) < C).reshape(nv, 32, 4)[None, :, :, 0]   # float4 j = lane + 32 i exists
        count = nv * 128 if fault == "padded lanes counted" else C
        inv_c = f32(1.0) / f32(count)

        def lanes_sum(t, masked):
            acc = np.zeros((rows, 32), f32)
            for i in range(nv):
                part = ((t[:, i, :, 0] + t[:, i, :, 1]).astype(f32) + (t[:, i, :, 2] + t[:, i, :, 3]).astype(f32)).astype(f32)
                acc = np.where(live[:, i] | (not masked), (acc + part).astype(f32), acc)
            if fault == "rows reduced together":                            # the butterfly runs over the 64 lanes of the wave: rows 2k and 2k + 1 (a missing partner adds 0)
                both = np.zeros((rows + rows % 2, 32), f32)
                both[:rows] = acc
                pair = _butterfly(both.reshape(-1, 64), 64)
                return pair.reshape(-1, 32)[:rows, 0]
            return _butterfly(acc, 32)[:, 0]
        mean = (lanes_sum(q4, False) * inv_c).astype(f32)
        d = (q4 - mean[:, None, None, None]).astype(f32)
        if fault == "padded lanes counted":
            sq = (d * d).astype(f32)                                        # the padding lanes' (0 - mean)^2 counted too
            var = (lanes_sum(sq, False) * inv_c).astype(f32)
        else:
            var = (lanes_sum((d * d).astype(f32), True) * inv_c).astype(f32)
        inv = (f32(1.0) / np.sqrt((var + e).astype(f32)).astype(f32)).astype(f32)
        y = (d * inv[:, None, None, None]).astype(f32).reshape(rows, nv * 128)[:, :C]
    else:
        n = (C + 63) // 64
        pad = np.zeros((rows, n * 64), f32)
        pad[:, :C] = s
        live = (np.arange(n * 64) < C).reshape(n, 64)

        def lanes_sum(t):
            acc = np.zeros((rows, 64), f32)
            t = t.reshape(rows, n, 64)
            for i in range(n):
                acc = np.where(live[i][None], (acc + t[:, i]).astype(f32), acc)
            return _butterfly(acc, 64)[:, 0]
        mean = (lanes_sum(pad) / f32(C)).astype(f32)
        d = (pad - mean[:, None]).astype(f32)
        var = (lanes_sum((d * d).astype(f32)) / f32(C)).astype(f32)
        inv = (f32(1.0) / np.sqrt((var + e).astype(f32)).astype(f32)).astype(f32)
        y = (d * inv[:, None]).astype(f32)[:, :C]
    if gamma is not None:
        y = (y * gamma.astype(f32)).astype(f32)
    if beta is not None:
        y = (y + beta.astype(f32)).astype(f32)
    return y, (y.copy() if fault == "sum written after" else s)


def error(y, s, ref):
    """the larger of max |y - f64| and max |s - the f32 sum| (the sum has to be exact); inf for a non-finite output"""
    if not (np.isfinite(y).all() and np.isfinite(s).all()):
        return float("inf")
    return max(float(np.abs(y.astype(np.float64) - ref["f64"]).max()), float(np.abs(s.astype(np.float64) - ref["sum"].astype(np.float64)).max()))
