"""The engine's f32 reduction kernels of csrc/kernels.hip -- soft-max, LayerNorm, the small batched GEMM, the pools, the squeeze-excite gate and the SVTR
attention -- as six families of one- or two-node graphs.  Per family: a case table, seeded input families, a float64 reference in plain
numpy, `form` (the launcher's selection rule restated: the profiler name the launch must carry with OAR_PROF_DETAIL=1), `emulate` (the kernel restated in
f32 numpy in its own order of operations, with switches that break it one way each) and `bundle` (the tolerance, by the project's two existing rules).

  soft-max, LayerNorm, pool means, se, attention   noise = max |f32 numpy - f64|, tol = max(16 noise, 2^-19); soft-max probabilities
                                                    relative to the float64 value, element by element, every other output in absolute terms
  gemm                                             f32_cases' S-normalised rule: S = the operation on absolute values (|bias| and |residual| included),
                                                    noise_S over two honest f32 evaluations, tol_S = 4 noise_S, applied in front of the activation
  MaxPool                                          exact: a maximum has no rounding

tests/test_row_cases_cpu.py holds the tables to their own claims without a GPU (every form has a case, the fault-free emulation is inside the tolerance
everywhere, every fault is outside it somewhere); tests/test_gpu_row_kernels.py holds the kernels to the same tolerances.

CPU only: numpy."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import attention_cases as A
from . import layernorm_cases as LN
from .f32_cases import err_S
from .layernorm_cases import _butterfly
from .models import decomposed_layernorm
from .onnx_writer import GraphBuilder

F32 = np.float32
FAMILIES = ("softmax", "layernorm", "gemm", "pool", "se", "attention")
FLOOR = 2.0 ** -19
FLT_MAX = F32(3.402823466e38)
# one child process per group (the switches are read once per process); every group runs with OAR_PROF_DETAIL=1 on top
GROUPS = {"softmax": {}, "layernorm": {}, "gemm": {}, "pool": {}, "se": {}, "attention": {}, "attention_f32": {"OAR_ATTN_X6": "0"}}


@dataclass(frozen=True)
class Case:
    """family: one of FAMILIES; kinds: the input families the case runs with; p: the family's own parameters, read as attributes"""
    family: str
    name: str
    kinds: tuple
    p: tuple

    def __getattr__(self, key):
        for k, v in object.__getattribute__(self, "p"):
            if k == key:
                return v
        raise AttributeError(key)


def _case(family, name, kinds, **p):
    return Case(family, name, tuple(kinds), tuple(sorted(p.items())))


def _r(a):
    return np.asarray(a, F32)


def _fma(a, b, c):
    """fmaf on f32 arrays: the product is exact in float64, one rounding to float64 and one to f32 (a double rounding differs from fmaf's single one in
    about one case in 2^29)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _rng(case, kind, seed):
    return np.random.default_rng([seed, FAMILIES.index(case.family), sum(case.name.encode()), len(case.name), sum(kind.encode())])


# ================================================================================================ soft-max
# softmax_lastdim: C <= 1024 -> softmax_wave_kernel (a wave per row, four rows per workgroup), above -> softmax_block_kernel (a workgroup per row, the
# row staged in C * 4 bytes of LDS: over 64 KB from C = 16385 on)
SOFTMAX_KINDS = ("normal", "flat", "tail peak", "low")
SOFTMAX_FAULTS = ("last element missing from the sum", "maximum per wave", "no subtraction of the maximum", "sum taken before the exp", "rows of a workgroup reduced together")
_SOFTMAX_C = (1, 2, 63, 64, 65, 1000, 1024, 1025, 1279, 1280, 4113, 16384, 16385, 18385)
_SOFTMAX_ROWS = (1, 3, 4, 5, 9)
SOFTMAX_CASES = tuple(_case("softmax", f"softmax r{r} C{C}", SOFTMAX_KINDS, rows=r, C=C)
                      for i, C in enumerate(_SOFTMAX_C) for r in sorted({_SOFTMAX_ROWS[i % 5], 9 if C in (1000, 18385) else _SOFTMAX_ROWS[(2 * i + 1) % 5]}))


def _softmax_inputs(c, kind, rng):
    """normal: N(0, 1).  flat: 50 + 2^-10 N(0, 1) -- every element carries 1 / C of the mass, one lost element is 1 / C of the sum.  tail peak: N(0, 1) - 8
    with the row maximum at index C - 1 (one above the largest other).  low: N(0, 1) - 200 -- without the subtraction of the maximum this is 0 / 0."""
    x = rng.standard_normal((c.rows, c.C))
    if kind == "flat":
        x = 50.0 + 2.0 ** -10 * x
    elif kind == "tail peak":
        x = x - 8.0
        x[:, -1] = x.max(-1) + 1.0
    elif kind == "low":
        x = x - 200.0
    return {"x": _r(x)}


def _softmax_ref(c, inp, dtype):
    z = inp["x"].astype(dtype)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _softmax_emulate(c, inp, fault):
    """wave form: lane l of 64 takes the elements l, l + 64, ..; block form: thread t of 256 takes t, t + 256, ..; the maximum, then exp(x - m) summed per
    lane in that order, a 64-lane butterfly, (block form) the four waves' sums as (w0 + w1) + (w2 + w3), then exp(x - m) / s"""
    x = inp["x"]
    rows, C = x.shape
    wave = C <= 1024
    W = 64 if wave else 256
    n = -(-C // W)
    live = (np.arange(n * W) < C).reshape(n, W)
    xs = np.zeros((rows, n * W), F32)
    xs[:, :C] = x
    xs = xs.reshape(rows, n, W)
    m_lane = np.where(live[None], xs, -FLT_MAX).max(1)                                        # [rows, W]
    m = np.repeat(m_lane.reshape(rows, W // 64, 64).max(-1), 64, axis=1)                        # every lane holds its wave's maximum
    if not (fault == "maximum per wave" and not wave):
        m = np.broadcast_to(m.max(-1, keepdims=True), (rows, W))
    if fault == "no subtraction of the maximum":
        m = np.zeros((rows, W), F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = (xs - m[:, None, :]).astype(F32)
        e = np.exp(d, dtype=F32)
        counted = live.copy()
        if fault == "last element missing from the sum":
            counted.reshape(-1)[C - 1] = False
        term = d if fault == "sum taken before the exp" else e
        s = np.zeros((rows, W), F32)
        for i in range(n):
            s = np.where(counted[i][None], (s + term[:, i]).astype(F32), s)
        w = _butterfly(s.reshape(rows * (W // 64), 64), 64)[:, 0].reshape(rows, W // 64)
        tot = w[:, 0] if wave else ((w[:, 0] + w[:, 1]).astype(F32) + (w[:, 2] + w[:, 3]).astype(F32)).astype(F32)
        if fault == "sum taken before the exp":
            tot = np.exp(tot, dtype=F32)
        if fault == "rows of a workgroup reduced together" and wave:
            for g in range(0, rows, 4):
                t = F32(0)
                for r in range(g, min(g + 4, rows)):
                    t = F32(t + tot[r])
                tot[g:g + 4] = t
        y = (e / tot[:, None, None]).astype(F32)
    return y.reshape(rows, n * W)[:, :C]


def _softmax_form(c, env):
    return (f"softmax wave C={c.C}" if c.C <= 1024 else f"softmax block C={c.C}"),


def _softmax_model(c, inp):
    g = GraphBuilder("softmax_case")
    g.add_input("x", [c.rows, c.C])
    g.add_output(g.op("Softmax", ["x"], axis=-1), [c.rows, c.C])
    return g.model()


# ================================================================================================ LayerNorm (k::layernorm, not the fused add)
# 4 | C <= 1024 and 16-byte pointers -> layernorm_v4_kernel<NV>, NV = ceil(C / 128) in 1 .. 4, else 8: half a wave per row, eight rows per workgroup;
# otherwise layernorm_kernel: a wave per row, four rows per workgroup
LN_KINDS = ("normal", "offset")
LN_FAULTS = ("padded lanes counted", "rows reduced together", "eps dropped", "bias added before the scale", "variance not centred")
#         C   rows affine eps  NaN rows
_LN_TABLE = ((4, 7, False, 1e-5, True), (32, 8, True, 1e-6, False), (124, 9, True, 1e-5, True), (128, 17, False, 1e-6, False),       # NV = 1
             (132, 1, False, 1e-5, False), (256, 7, True, 1e-6, True),                                                                 # NV = 2
             (260, 8, False, 1e-5, False), (384, 9, True, 1e-6, True),                                                                 # NV = 3
             (388, 17, True, 1e-5, False), (512, 1, False, 1e-6, False),                                                               # NV = 4
             (516, 7, True, 1e-5, True), (1020, 8, False, 1e-6, True), (1024, 9, True, 1e-5, False),                                   # NV = 8 (5 .. 8 registers' worth)
             (1, 17, False, 1e-6, False), (3, 1, True, 1e-5, False), (30, 7, False, 1e-6, True), (65, 8, True, 1e-5, True),            # the one-wave form
             (1028, 9, True, 1e-6, False), (1500, 17, False, 1e-5, True))
LN_CASES = tuple(_case("layernorm", f"layernorm r{r} C{C} {'affine' if aff else 'plain'} eps{eps:g}", LN_KINDS + (("nan4", "nan5") if nan else ()),
                       rows=r, C=C, affine=aff, eps=eps) for C, r, aff, eps, nan in _LN_TABLE)


def _ln_inputs(c, kind, rng):
    """normal: N(0, 1).  offset: every row sits at about 8 with unit spread (a mean over the wrong count, a sum in another order show; at 8 the f32
    noise of the row's own rounding keeps 16 noise below 2^-14, at layernorm_cases' 50 it does not).  nan4 / nan5: `normal` with one NaN in row 4 / 5 --
    the two rows share a wave in the half-wave form."""
    x = rng.standard_normal((c.rows, c.C))
    gamma, beta = 1.0 + 0.3 * rng.standard_normal(c.C), 0.2 * rng.standard_normal(c.C)
    if kind == "offset":
        x = x + 8.0 + rng.standard_normal((c.rows, 1))
    out = {"x": _r(x)}
    if kind.startswith("nan"):
        out = {"x": _ln_inputs(c, "normal", _rng(c, "normal", 0))["x"].copy()}
        out["x"][int(kind[3]), c.C // 2] = np.nan
        gamma, beta = (_ln_inputs(c, "normal", _rng(c, "normal", 0)).get(k) for k in ("gamma", "beta"))
    if c.affine:
        out["gamma"], out["beta"] = _r(gamma), _r(beta)
    return out


def _ln_ref(c, inp, dtype):
    x = inp["x"]
    return LN.ln_of_sum(x, np.zeros((1, c.C), F32), 1, inp.get("gamma"), inp.get("beta"), c.eps, dtype)


def _ln_emulate(c, inp, fault):
    """layernorm_cases.emulate with a zero residual (x + 0 is x): the same row routine as add_layernorm.hip's, which is bit-identical to k::layernorm"""
    x, gamma, beta = inp["x"], inp.get("gamma"), inp.get("beta")
    zero = np.zeros((1, c.C), F32)
    v4 = LN.takes_v4(c.C)
    if fault == "variance not centred":
        mean = x.mean(-1, dtype=F32, keepdims=True)
        var = ((x * x).mean(-1, dtype=F32, keepdims=True) - mean * mean).astype(F32)
        with np.errstate(invalid="ignore", divide="ignore"):
            y = ((x - mean) / np.sqrt(var + F32(c.eps))).astype(F32)
        return y if gamma is None else (y * gamma + beta).astype(F32)
    if fault == "bias added before the scale":
        y, _ = LN.emulate(x, zero, 1, None, None, c.eps, None, v4)
        return y if gamma is None else ((y + beta).astype(F32) * gamma).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):      # (eps dropped at C = 1: 0 / 0)
        return LN.emulate(x, zero, 1, gamma, beta, c.eps, fault, v4)[0]


def ln_nv(C):
    nv = (C // 4 + 31) // 32
    return nv if nv <= 4 else 8


def _ln_form(c, env):
    return (f"layernorm v4x{ln_nv(c.C)} C={c.C}" if LN.takes_v4(c.C) else f"layernorm wave C={c.C}"),


def _ln_model(c, inp):
    g = GraphBuilder("layernorm_case")
    g.add_input("x", [c.rows, c.C])
    if c.affine:
        y = g.op("LayerNormalization", ["x", g.init(inp["gamma"]), g.init(inp["beta"])], axis=-1, epsilon=float(c.eps))
    else:      # the opset-17 node must have a scale: without one, the exporters' spelling, which rewrite pass 2c turns into a LayerNormalization of x alone
        y = decomposed_layernorm(g, "x", None, None, float(c.eps))
    g.add_output(y, [c.rows, c.C])
    return g.model()


# ================================================================================================ gemm_batched
# Linear route (op_linear): a MatMul / Gemm with a constant B runs here when K % 4 != 0 or alpha != 1 (batch 1; bias = beta C folded on the host; an
# activation and a residual Add in the epilogue).  MatMul route (op_matmul): two activations, batch = the larger leading extent, the other operand's
# batch stride 0 when it has none.
GEMM_KINDS = ("normal", "positive")
GEMM_FAULTS = ("K tail not zero-filled", "last K column dropped", "transB ignored", "bias indexed by row", "alpha applied after the bias",
               "broadcast operand advanced by its batch stride")


def _lin(name, M, N, K, spelling="matmul", tB=0, bias=True, alpha=1.0, beta=1.0, act="none", res=False):
    return _case("gemm", f"linear {name} M{M} N{N} K{K}", GEMM_KINDS, route="linear", M=M, N=N, K=K, spelling=spelling, tB=tB, bias=bias, alpha=alpha, beta=beta,
                 act=act, res=res, batch=1, bcast="none")


def _mm(M, N, K, batch, bcast, nan=False):
    return _case("gemm", f"matmul b{batch} {bcast} M{M} N{N} K{K}", GEMM_KINDS + (("nan",) if nan else ()), route="matmul", M=M, N=N, K=K, spelling="matmul",
                 tB=0, bias=False, alpha=1.0, beta=1.0, act="none", res=False, batch=batch, bcast=bcast)


GEMM_CASES = (
    _lin("matmul bias", 1, 67, 30),
    _lin("matmul relu", 63, 3, 15, bias=False, act="relu"),
    _lin("matmul residual", 64, 64, 17, res=True),
    _lin("matmul bias relu", 65, 67, 67, act="relu"),
    _lin("matmul residual one column", 130, 1, 30, res=True),
    _lin("matmul one term", 65, 67, 1),
    _lin("matmul residual no bias", 63, 67, 15, bias=False, res=True),
    _lin("gemm half transB relu", 64, 3, 16, "gemm", tB=1, alpha=0.5, act="relu"),
    _lin("gemm half beta", 130, 64, 64, "gemm", alpha=0.5, beta=0.25),
    _lin("gemm transB beta", 63, 67, 15, "gemm", tB=1, beta=0.25),
    _lin("gemm half relu one row", 1, 64, 17, "gemm", alpha=0.5, act="relu"),
    _lin("gemm transB no C", 65, 1, 67, "gemm", tB=1, bias=False),
    _lin("gemm half transB beta relu", 130, 67, 30, "gemm", tB=1, alpha=0.5, beta=0.25, act="relu"),
    _mm(63, 67, 17, 1, "none"),
    _mm(65, 3, 30, 3, "none", nan=True),
    _mm(1, 64, 67, 7, "A"),
    _mm(130, 67, 15, 3, "B", nan=True),
    _mm(64, 1, 1, 7, "none"),
    _mm(65, 67, 16, 3, "A", nan=True),
    _mm(17, 130, 64, 7, "B"),
)
GEMM_NAN_ROW = 0      # the row of A (of its batch 1 where A has batches) that holds the NaN of kind `nan`


def _gemm_inputs(c, kind, rng):
    """normal: every operand N(0, 1).  positive: uniform(1, 2) -- a lost term cannot hide in cancellation.  nan: `normal` with one NaN in one row of A."""
    if kind == "nan":
        out = _gemm_inputs(c, "normal", _rng(c, "normal", 0))
        a = out["a"].copy()
        a.reshape(-1, c.M, c.K)[min(1, a.size // (c.M * c.K) - 1), GEMM_NAN_ROW, c.K // 2] = np.nan
        out["a"] = a
        return out
    draw = (lambda *s: rng.standard_normal(s)) if kind == "normal" else (lambda *s: rng.uniform(1.0, 2.0, s))
    out = {}
    if c.route == "linear":
        out["a"] = _r(draw(c.M, c.K))
        out["w"] = _r(draw(c.N, c.K) if c.tB else draw(c.K, c.N))
        if c.bias:
            out["c"] = _r(draw(c.N))
        if c.res:
            out["r"] = _r(draw(c.M, c.N))
    else:
        out["a"] = _r(draw(c.M, c.K) if c.bcast == "A" else draw(c.batch, c.M, c.K))
        out["w"] = _r(draw(c.K, c.N) if c.bcast == "B" else draw(c.batch, c.K, c.N))
    return out


def _gemm_ops(c, inp):
    """-> A [batch or 1, M, K], B [batch or 1, K, N], bias [N] or None (beta C in f32, as the engine folds it), residual or None: all f32"""
    A_ = inp["a"].reshape(-1, c.M, c.K)
    w = inp["w"]
    B = (w.T if c.tB else w).reshape(-1, c.K, c.N)
    bias = (inp["c"] * F32(c.beta)).astype(F32) if "c" in inp else None
    return A_, B, bias, inp.get("r")


def _gemm_ref(c, inp, dtype, absolute=False, act=True):
    A_, B, bias, r = _gemm_ops(c, inp)
    f = (lambda v: np.abs(v.astype(dtype))) if absolute else (lambda v: v.astype(dtype))
    y = np.matmul(f(A_), f(B)) * np.asarray(abs(c.alpha) if absolute else c.alpha, dtype)
    if bias is not None:
        y = y + f(bias)
    y = y.reshape((c.M, c.N) if c.route == "linear" else (-1, c.M, c.N))
    if r is not None:
        y = y + f(r)
    return np.where(y < 0, np.asarray(0, dtype), y) if (act and c.act == "relu") else y


def _gemm_chain(c, inp):
    """the plain f32 evaluation: k ascending, one rounding per multiplication and per addition, then alpha, the bias, the residual"""
    A_, B, bias, r = _gemm_ops(c, inp)
    acc = np.zeros((max(A_.shape[0], B.shape[0]), c.M, c.N), F32)
    for k in range(c.K):
        acc = (acc + (A_[:, :, k, None] * B[:, k, None, :]).astype(F32)).astype(F32)
    y = (acc * F32(c.alpha)).astype(F32)
    if bias is not None:
        y = (y + bias).astype(F32)
    y = y.reshape((c.M, c.N) if c.route == "linear" else (-1, c.M, c.N))
    return y if r is None else (y + r).astype(F32)


def _gemm_emulate(c, inp, fault):
    """the kernel: K in steps of 16 through LDS (entries past K are zero), acc = fmaf(a, b, acc) with k ascending from acc = 0, then acc * alpha, + bias[n],
    + residual, the activation"""
    A_, B, bias, r = _gemm_ops(c, inp)
    batch = max(A_.shape[0], B.shape[0]) if c.route == "matmul" else 1
    K16 = -(-c.K // 16) * 16
    if fault == "transB ignored" and c.tB:
        B = inp["w"].reshape(-1)[:c.K * c.N].reshape(1, c.K, c.N)

    def operand(X, b, rows_axis):
        """batch b of an operand -> [rows, K16] (A) or [K16, cols] (B), the K tail zero or -- the fault -- whatever follows in memory (zeros past the end)"""
        nb = X.shape[0]
        if fault == "broadcast operand advanced by its batch stride" and nb == 1 and b > 0:
            return np.zeros((c.M, K16) if rows_axis else (K16, c.N), F32)            # reads past the operand's end
        Xb = X[b if nb > 1 else 0]
        if fault == "K tail not zero-filled":
            flat = np.concatenate([X.reshape(-1), np.zeros(K16 * max(c.M, c.N) + 16, F32)])
            base = (b if nb > 1 else 0) * Xb.size
            if rows_axis:
                return flat[base + np.arange(c.M)[:, None] * c.K + np.arange(K16)[None, :]]
            if c.tB and c.route == "linear":      # B stored [N, K]: the tail of a row is the head of the next
                return flat[base + np.arange(c.N)[None, :] * c.K + np.arange(K16)[:, None]]
            return flat[base + np.arange(K16)[:, None] * c.N + np.arange(c.N)[None, :]]
        pad = np.zeros((c.M, K16) if rows_axis else (K16, c.N), F32)
        if rows_axis:
            pad[:, :c.K] = Xb
        else:
            pad[:c.K] = Xb
        return pad
    out = np.zeros((batch, c.M, c.N), F32)
    kend = c.K - 1 if fault == "last K column dropped" else K16
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(batch):
            a, w = operand(A_, b, True), operand(B, b, False)
            acc = np.zeros((c.M, c.N), F32)
            for k in range(kend):
                acc = _fma(a[:, k, None], w[None, k, :], acc)
            bv = None if bias is None else (np.broadcast_to(bias[np.minimum(np.arange(c.M), c.N - 1), None], (c.M, c.N)) if fault == "bias indexed by row" else bias[None, :])
            if fault == "alpha applied after the bias" and bv is not None:
                v = ((acc + bv).astype(F32) * F32(c.alpha)).astype(F32)
            else:
                v = (acc * F32(c.alpha)).astype(F32)
                v = v if bv is None else (v + bv).astype(F32)
            if r is not None:
                v = (v + r).astype(F32)
            out[b] = np.where(v <= 0, F32(0), v) if c.act == "relu" else v
    return out[0] if c.route == "linear" else out


def _gemm_form(c, env):
    return f"gemm_batched b={c.batch} M={c.M} N={c.N} K={c.K} tB={c.tB}",


def _gemm_model(c, inp):
    g = GraphBuilder("gemm_case")
    if c.route == "matmul":
        g.add_input("a", list(inp["a"].shape))
        g.add_input("w", list(inp["w"].shape))
        g.add_output(g.op("MatMul", ["a", "w"]), [c.batch, c.M, c.N])
        return g.model()
    g.add_input("a", [c.M, c.K])
    if c.res:
        g.add_input("r", [c.M, c.N])
    if c.spelling == "gemm":
        y = g.op("Gemm", ["a", g.init(inp["w"])] + ([g.init(inp["c"])] if c.bias else []), alpha=float(c.alpha), beta=float(c.beta), transB=int(c.tB))
    else:
        y = g.op("MatMul", ["a", g.init(inp["w"])])
        if c.bias:
            y = g.op("Add", [y, g.init(inp["c"])])
    if c.act == "relu":
        y = g.op("Relu", [y])
    if c.res:
        y = g.op("Add", [y, "r"])
    g.add_output(y, [c.M, c.N])
    return g.model()


# ================================================================================================ pools
# GlobalAveragePool: 4 | C <= 1024 -> global_avgpool_kernel, one pass or (splits > 1) a pass per pixel split and a second launch over the [splits][C]
# partial sums; otherwise global_avgpool_scalar_kernel.  ReduceMean over the last axis: reduce_lastdim_kernel, mode 0.  AveragePool / MaxPool: pool2d_kernel.
POOL_KINDS = ("normal", "offset")
POOL_FAULTS = ("a split's last pixel dropped", "second pass divides by the number of splits", "an idle thread group contributes", "four-way loop's tail skipped",
               "mean over the padded count")
RED_C = (1, 2, 63, 64, 65, 129, 1000)      # the sizes the exact Reduce tests walk (op_cases.RED_C, restated: this package does not read the checker's)


def _gap(N, C, H, W):
    return _case("pool", f"gap N{N} C{C} {H}x{W}", POOL_KINDS, op="gap", N=N, C=C, H=H, W=W)


def _p2d(op, N, C, H, W, k, s, p, ceil=0, kinds=POOL_KINDS):
    return _case("pool", f"{op} N{N} C{C} {H}x{W} k{k} s{s} p{p}{' ceil' if ceil else ''}", kinds, op=op, N=N, C=C, H=H, W=W, k=k, s=s, pad=p, ceil=ceil)


_MAX_KINDS = POOL_KINDS + ("neginf",)
POOL_CASES = (
    _gap(2, 4, 1, 1), _gap(3, 4, 5, 17), _gap(1, 48, 1, 5), _gap(2, 48, 3, 7), _gap(3, 48, 2, 11), _gap(2, 48, 5, 17), _gap(1, 256, 3, 7), _gap(2, 256, 5, 17),
    _gap(2, 1024, 1, 5), _gap(1, 1024, 2, 11), _gap(3, 1024, 5, 17),
    _gap(1, 48, 23, 23), _gap(2, 4, 26, 50), _gap(1, 256, 16, 33),      # splits: 2 of 265 and 264 pixels; 5 of 260; 2 of 264
    _gap(2, 6, 3, 7), _gap(1, 1028, 1, 5), _gap(3, 1028, 2, 11),        # the scalar form
) + tuple(_case("pool", f"mean r{r} C{C}", POOL_KINDS, op="mean", rows=r, C=C) for r, C in zip((5, 1, 9, 4, 7, 3, 9), RED_C)) + (
    _p2d("avg", 2, 8, 9, 11, 3, 2, 1), _p2d("avg", 1, 5, 10, 14, 2, 2, 0), _p2d("avg", 2, 8, 9, 11, 3, 2, 1, ceil=1),
    _p2d("max", 2, 8, 9, 11, 3, 2, 1, kinds=_MAX_KINDS), _p2d("max", 1, 5, 10, 14, 2, 2, 0, kinds=_MAX_KINDS), _p2d("max", 2, 8, 10, 12, 3, 2, 1, ceil=1, kinds=_MAX_KINDS),
)


def gap_splits(N, HW, C):
    """global_avgpool_splits"""
    if C % 4 or C // 4 > 256 or N <= 0:
        return 1
    return max(1, min(min(-(-1024 // N), max(HW // 256, 1)), 256))


def _pool_inputs(c, kind, rng):
    """normal: N(0, 1).  offset: 3 + N(0, 1), every value of one sign (a lost or doubled pixel cannot hide in cancellation).  neginf (MaxPool): `normal`
    with the top-left 3 x 3 pixels and the whole row 4 at -inf -- the corner window holds nothing else, the windows over row 4 hold some"""
    shape = (c.rows, c.C) if c.op == "mean" else (c.N, c.C, c.H, c.W)
    x = rng.standard_normal(shape)
    if kind == "offset":
        x = x + 3.0
    if kind == "neginf":
        x[:, :, :3, :3] = -np.inf
        x[:, :, 4, :] = -np.inf
    return {"x": _r(x)}


def _pool_out_hw(c):
    def od(n):
        t = n + 2 * c.pad - c.k
        o = (-(-t // c.s) if c.ceil else t // c.s) + 1
        return o - 1 if c.ceil and (o - 1) * c.s >= n + c.pad else o
    return od(c.H), od(c.W)


def _pool2d(c, x, dtype, sequential=False):
    """pool2d_kernel's window walk (rows outside, columns inside), an average divided once by the number of pixels inside the map"""
    ho, wo = _pool_out_hw(c)
    x = x.astype(dtype)
    y = np.zeros((c.N, c.C, ho, wo), dtype)
    for oy in range(ho):
        for ox in range(wo):
            ys = [i for i in range(oy * c.s - c.pad, oy * c.s - c.pad + c.k) if 0 <= i < c.H]
            xs = [j for j in range(ox * c.s - c.pad, ox * c.s - c.pad + c.k) if 0 <= j < c.W]
            win = x[:, :, ys][:, :, :, xs].reshape(c.N, c.C, -1)
            if c.op == "max":
                y[:, :, oy, ox] = win.max(-1)
            elif sequential:
                acc = np.zeros((c.N, c.C), dtype)
                for t in range(win.shape[-1]):
                    acc = acc + win[:, :, t]
                y[:, :, oy, ox] = acc / np.asarray(win.shape[-1], dtype)
            else:
                y[:, :, oy, ox] = win.mean(-1)
    return y


def _pool_ref(c, inp, dtype):
    x = inp["x"]
    if c.op == "gap":
        return x.astype(dtype).mean((2, 3), keepdims=True)
    if c.op == "mean":
        return x.astype(dtype).mean(-1)
    with np.errstate(invalid="ignore"):
        return _pool2d(c, x, dtype)


def _gap_pass(x, splits, div, fault):
    """one launch of global_avgpool_kernel on x [N, HW, C] -> [N, splits, C]: 256 / (C / 4) thread groups stride over the split's pixels four at a time as
    (a + b) + (c + d), then one by one; the groups' sums are added in order and divided by `div`"""
    N, HW, C = x.shape
    C4 = C // 4
    parts = max(256 // C4, 1)
    per = -(-HW // splits)
    out = np.zeros((N, splits, C), F32)
    for sp in range(splits):
        p0, p1 = sp * per, min(HW, sp * per + per)
        if fault == "a split's last pixel dropped" and splits > 1:
            p1 -= 1
        idle = 256 - parts * C4 if fault == "an idle thread group contributes" else 0
        t = None
        for part in range(parts + (1 if idle else 0)):
            acc = np.zeros((N, C), F32)
            i = p0 + part
            while i + 3 * parts < p1:
                ab, cd = (x[:, i] + x[:, i + parts]).astype(F32), (x[:, i + 2 * parts] + x[:, i + 3 * parts]).astype(F32)
                acc = (acc + (ab + cd).astype(F32)).astype(F32)
                i += 4 * parts
            while i < p1 and fault != "four-way loop's tail skipped":
                acc = (acc + x[:, i]).astype(F32)
                i += parts
            if part == parts:
                acc[:, 4 * idle:] = 0
            t = acc if t is None else (t + acc).astype(F32)
        out[:, sp] = (t / F32(div)).astype(F32)
    return out


def _gap_emulate(x, fault=None):
    """x [N, C, H, W] -> the pooled [N, C] as global_avgpool computes it on the channels-last map"""
    N, C, H, W = x.shape
    HW = H * W
    xl = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(N, HW, C)
    if C % 4 == 0 and C // 4 <= 256:
        splits = gap_splits(N, HW, C)
        if splits == 1:
            return _gap_pass(xl, 1, HW, fault)[:, 0]
        return _gap_pass(_gap_pass(xl, splits, 1.0, fault), 1, splits if fault == "second pass divides by the number of splits" else HW, fault)[:, 0]
    acc = np.zeros((N, C), F32)
    for i in range(HW):
        acc = (acc + xl[:, i]).astype(F32)
    return (acc / F32(HW)).astype(F32)


def _wave_rows_sum(x):
    """[rows, C] -> lane l of 64 adds the elements l, l + 64, .. in order, then a 64-lane butterfly"""
    rows, C = x.shape
    n = -(-C // 64)
    pad = np.zeros((rows, n * 64), F32)
    pad[:, :C] = x
    pad = pad.reshape(rows, n, 64)
    acc = np.zeros((rows, 64), F32)
    for i in range(n):
        acc = (acc + pad[:, i]).astype(F32)      # (a lane past C adds 0: x + 0 is x)
    return _butterfly(acc, 64)[:, 0]


def _pool_emulate(c, inp, fault):
    x = inp["x"]
    if c.op == "gap":
        return _gap_emulate(x, fault).reshape(c.N, c.C, 1, 1)
    if c.op == "mean":
        count = -(-c.C // 64) * 64 if fault == "mean over the padded count" else c.C
        return (_wave_rows_sum(x) / F32(count)).astype(F32)
    with np.errstate(invalid="ignore"):
        return _pool2d(c, x, F32, sequential=True)


def _pool_form(c, env):
    if c.op == "gap":
        vec = c.C % 4 == 0 and c.C // 4 <= 256
        return f"global_avgpool N={c.N} HW={c.H * c.W} C={c.C} " + (f"splits={gap_splits(c.N, c.H * c.W, c.C)}" if vec else "scalar"),
    return ("reduce_mean" if c.op == "mean" else "pool2d"),


def _pool_model(c, inp):
    g = GraphBuilder("pool_case")
    if c.op == "mean":
        g.add_input("x", [c.rows, c.C])
        g.add_output(g.op("ReduceMean", ["x"], axes=[-1], keepdims=0), [c.rows])
        return g.model()
    g.add_input("x", [c.N, c.C, c.H, c.W])
    if c.op == "gap":
        g.add_output(g.op("GlobalAveragePool", ["x"]), [c.N, c.C, 1, 1])
        return g.model()
    ho, wo = _pool_out_hw(c)
    y = g.op("AveragePool" if c.op == "avg" else "MaxPool", ["x"], kernel_shape=[c.k, c.k], strides=[c.s, c.s], pads=[c.pad] * 4, ceil_mode=int(c.ceil))
    g.add_output(y, [c.N, c.C, ho, wo])
    return g.model()


# ================================================================================================ squeeze-excite gate
# GlobalAveragePool -> 1x1 + ReLU -> 1x1 + HardSigmoid -> Mul: the two 1x1 layers are ONE se_fc launch on the pooled vector (tiles = 0)
SE_KINDS = ("normal", "shifted")
SE_FAULTS = ("hidden unit past Cmid written", "parts overlap by one unit", "slice tail reads the neighbouring slice's partial", "b1 omitted", "FC1 tail loop skipped")
SE_ALPHA, SE_BETA = 0.2, 0.5


def _se(C, R, N, G, slice_, parts):
    return _case("se", f"se C{C} R{R} N{N}", SE_KINDS, C=C, R=R, N=N, H=3, W=5, G=G, slice=slice_, parts=parts)


#   C     R    N    G  slice parts
SE_CASES = (
    _se(48, 12, 5, 1, 64, 2),          # one workgroup per image, a ragged slice
    _se(192, 48, 130, 1, 192, 5),      # N >= 128: G = 1 whatever the width; a slice above 64
    _se(768, 192, 3, 6, 128, 8),       # few images: six slices of 128, parts = 8, the 16-load main loop three times
    _se(1100, 70, 2, 6, 192, 5),       # C no multiple of 64 (main loop, tail, a ragged last stride), Cmid no multiple of 4 or 8, the scalar pool
    _se(20, 6, 40, 1, 64, 1),          # parts = 1, everything in the tail loops
    _se(300, 30, 9, 5, 64, 4),         # five slices of 64, the last of 44; Cmid = 30 in four parts of 8, 8, 8, 6
)


def se_geometry(N, C, Cmid, Cout):
    """se_fc's launch arithmetic -> (G, slice, parts)"""
    G = 1
    if N < 128:
        G = max(1, min(min(8, 256 // N), (Cout + 63) // 64))
    slice_ = ((Cout + G - 1) // G + 63) // 64 * 64
    while slice_ > 1024:
        G += 1
        slice_ = ((Cout + G - 1) // G + 63) // 64 * 64
    G = (Cout + slice_ - 1) // slice_
    return G, slice_, max(1, min(min(8, 1024 // slice_), (Cmid + 7) // 8))


def _se_inputs(c, kind, rng):
    """normal: x = 1 + N(0, 1) (the pooled vector is about 1, so that b1 and every weight matter), w1 = N(0, 1) / sqrt(C), w2 = N(0, 1) / sqrt(R): the gate
    stays off HardSigmoid's flat ends almost everywhere.  shifted: x = 3 + N(0, 1) and w1 = |N(0, 1)| / C: every hidden unit is positive (no ReLU hides one)."""
    x = rng.standard_normal((c.N, c.C, c.H, c.W)) + (1.0 if kind == "normal" else 3.0)
    w1 = rng.standard_normal((c.R, c.C)) / np.sqrt(c.C) if kind == "normal" else np.abs(rng.standard_normal((c.R, c.C))) / c.C
    return {"x": _r(x), "w1": _r(w1), "b1": _r(0.5 * rng.standard_normal(c.R)), "w2": _r(rng.standard_normal((c.C, c.R)) / np.sqrt(c.R)), "b2": _r(0.3 * rng.standard_normal(c.C))}


def _se_ref(c, inp, dtype):
    t = np.dtype(dtype).type
    x = inp["x"].astype(dtype)
    pooled = x.mean((2, 3))
    h = np.maximum(pooled @ inp["w1"].astype(dtype).T + inp["b1"].astype(dtype), t(0))
    gate = np.clip((h @ inp["w2"].astype(dtype).T + inp["b2"].astype(dtype)) * t(F32(SE_ALPHA)) + t(SE_BETA), t(0), t(1))
    return x * gate[:, :, None, None]


def _se_emulate(c, inp, fault):
    """global_avgpool's pooled vector, then se_fc_kernel: FC1 -- lane l of a wave takes the channels l, l + 64, .. as fmaf in order (the 16-load main loop and its
    tail walk the same order), a 64-lane butterfly, + b1, ReLU; FC2 -- the hidden axis in `parts` ranges of ceil(Cmid / parts), fmaf in order, the ranges' sums
    added to b2 in order, HardSigmoid; then the Mul"""
    x, w1, b1, w2, b2 = (inp[k] for k in ("x", "w1", "b1", "w2", "b2"))
    N, C, R = c.N, c.C, c.R
    G, slice_, parts = se_geometry(N, C, R, C)
    pooled = _gap_emulate(x)
    n = -(-C // 64)
    wp, pp = np.zeros((R, n * 64), F32), np.zeros((N, n * 64), F32)
    wp[:, :C], pp[:, :C] = w1, pooled
    lanes = np.arange(64)
    iters = np.maximum(0, -(-(C - 192 - lanes) // 256))                 # rounds of the 16-load main loop per lane
    acc = np.zeros((N, R, 64), F32)
    for i in range(n):
        live = (i * 64 + lanes < C) & ((i < 4 * iters) | (fault != "FC1 tail loop skipped"))
        acc = np.where(live[None, None], _fma(wp[None, :, i * 64:(i + 1) * 64], pp[:, None, i * 64:(i + 1) * 64], acc), acc)
    v = _butterfly(acc.reshape(N * R, 64), 64)[:, 0].reshape(N, R)
    if fault != "b1 omitted":
        v = (v + b1[None]).astype(F32)
    hidden = np.where(v <= 0, F32(0), v)
    per = -(-R // parts)
    ext = -(-R // 4) * 4 if fault == "hidden unit past Cmid written" else R     # the units of the last pass of four, each a copy of unit Cmid - 1, are summed too
    hid = np.concatenate([hidden, np.repeat(hidden[:, -1:], max(per * parts, ext) - R + 1, axis=1)], 1)
    w2t = np.concatenate([w2.T, np.repeat(w2.T[-1:], hid.shape[1] - R, axis=0)], 0)      # [units][Cout]
    partial = np.zeros((N, parts, C), F32)
    for q in range(parts):
        j0 = q * per
        j1 = min(j0 + per, R)
        if fault == "parts overlap by one unit":
            j1 = min(j0 + per + 1, R)
        if fault == "hidden unit past Cmid written" and q == parts - 1:
            j1 = max(j1, ext)
        a = np.zeros((N, C), F32)
        for j in range(j0, j1):
            a = _fma(w2t[None, j, :], hid[:, j, None], a)
        partial[:, q] = a
    if fault == "slice tail reads the neighbouring slice's partial":      # the last slice's rows of `partial` read at its own width, not at `slice`
        lo = (G - 1) * slice_
        wd = C - lo
        flat = np.zeros((N, parts * slice_), F32)
        for q in range(parts):
            flat[:, q * slice_:q * slice_ + wd] = partial[:, q, lo:]
        for q in range(parts):
            partial[:, q, lo:] = flat[:, q * wd:q * wd + wd]
    a = np.broadcast_to(b2[None], (N, C)).astype(F32)
    for q in range(parts):
        a = (a + partial[:, q]).astype(F32)
    gate = np.clip(((a * F32(SE_ALPHA)).astype(F32) + F32(SE_BETA)).astype(F32), F32(0), F32(1))
    return (x * gate[:, :, None, None]).astype(F32)


def _se_form(c, env):
    G, slice_, parts = se_geometry(c.N, c.C, c.R, c.C)
    return f"se_fc G={G} slice={slice_} parts={parts} tiles=0",


def _se_model(c, inp):
    g = GraphBuilder("se_case")
    g.add_input("x", [c.N, c.C, c.H, c.W])
    conv = dict(kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
    p = g.op("GlobalAveragePool", ["x"])
    h = g.op("Relu", [g.op("Conv", [p, g.init(inp["w1"].reshape(c.R, c.C, 1, 1)), g.init(inp["b1"])], **conv)])
    s = g.op("HardSigmoid", [g.op("Conv", [h, g.init(inp["w2"].reshape(c.C, c.R, 1, 1)), g.init(inp["b2"])], **conv)], alpha=SE_ALPHA, beta=SE_BETA)
    g.add_output(g.op("Mul", ["x", s]), [c.N, c.C, c.H, c.W])
    return g.model()


# ================================================================================================ SVTR attention (the f32 kernels)
# k::attention: head dim 32 with more than 32 tokens goes to the bf16x6 kernel unless OAR_ATTN_X6=0; everything else runs attention_kernel<HD> (K and V of
# a head in LDS: 2 T HD floats <= 150 KB) or attention_stream_kernel<HD> (key blocks of 128 with a running maximum), HD = 16, 32 or 64 >= the head dim
ATTN_KINDS = ("normal", "equal", "rising", "falling")
ATTN_FAULTS = ("padded head-dim lanes read", "correction factor dropped when the maximum rises", "last key block's length taken as 128", "scale applied to k as well",
               "maximum frozen after the first block")
ATTN_BLOCK = 128


def _att(hd, heads, T, kinds=ATTN_KINDS):
    return _case("attention", f"attention hd{hd} h{heads} T{T}", kinds, hd=hd, heads=heads, T=T, n=1)


ATTN_CASES = (
    _att(4, 2, 1), _att(15, 1, 31), _att(16, 2, 64),                         # HD = 16
    _att(20, 1, 2), _att(32, 2, 32), _att(32, 1, 65), _att(20, 2, 63),       # HD = 32 (hd 32, T 65: the f32 kernel only with OAR_ATTN_X6=0)
    _att(33, 1, 63), _att(64, 1, 257), _att(64, 2, 64),                      # HD = 64; T = 257: one thread takes a second query
    _att(64, 1, 301, ("normal", "rising", "falling")), _att(64, 2, 385, ("normal", "rising", "falling")), _att(33, 1, 301),      # streamed: three key blocks, the last ragged
    _att(20, 1, 601, ("normal", "rising")), _att(16, 1, 1201, ("normal", "falling")),                                              # the streaming kernel's HD = 32 and HD = 16
)


def attn_hd_padded(hd):
    return 16 if hd <= 16 else 32 if hd <= 32 else 64


def attn_whole(T, hd):
    return 2 * T * attn_hd_padded(hd) * 4 <= 150 * 1024


def _attn_inputs(c, kind, rng):
    """attention_cases.mha_inputs (normal / equal / rising / falling: scores of -+200 that raise the running maximum in every key block, or leave every
    block but the first to underflow), packed as the [n, T, 3 heads hd] projection the kernel reads"""
    q, k, v = A.mha_inputs(kind, c.n, c.T, c.T, c.heads, c.hd, seed=int(rng.integers(1 << 30)))
    return {"x": np.ascontiguousarray(np.concatenate([a.reshape(c.n, c.T, c.heads * c.hd) for a in (q, k, v)], -1))}


def _attn_split(c, x):
    return tuple(x.reshape(c.n, c.T, 3, c.heads, c.hd)[:, :, i] for i in range(3))


def _attn_ref(c, inp, dtype):
    q, k, v = _attn_split(c, inp["x"])
    return A.mha_core(q, k, v, A.scale_of(c.hd), True, dtype)


def _attn_emulate(c, inp, fault):
    """one thread per query: q scale rounded once, a score = fmaf over the head dim from 0, (whole-head form) the maximum over all keys, then p = exp(s - m),
    l += p and o = fmaf(p, v, o) with the keys ascending; (streamed form) the same per block of 128 keys with m, l and o rescaled by exp(m_old - m_new)"""
    x = inp["x"]
    n, T, heads, hd = c.n, c.T, c.heads, c.hd
    HD = attn_hd_padded(hd)
    scale = A.scale_of(hd)
    q, k, v = (np.ascontiguousarray(a.transpose(0, 2, 1, 3)) for a in _attn_split(c, x))      # [n, heads, T, hd]
    qs = (q * scale).astype(F32)
    if fault == "scale applied to k as well":
        k = (k * scale).astype(F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        S = np.zeros((n, heads, T, T), F32)
        for d in range(hd):
            S = _fma(qs[..., :, None, d], k[..., None, :, d], S)
        if fault == "padded head-dim lanes read":      # lanes hd .. HD - 1 of q and k are the following columns of the row (zeros past its end)
            row = np.concatenate([x, np.zeros((n, T, HD), F32)], -1)
            dim = heads * hd
            for h in range(heads):
                for d in range(hd, HD):
                    S[:, h] = _fma((row[:, :, None, h * hd + d] * scale).astype(F32), row[:, None, :, dim + h * hd + d], S[:, h])
        whole = attn_whole(T, hd)
        blocks = [(0, T)] if whole else [(j0, min(j0 + ATTN_BLOCK, T)) for j0 in range(0, T, ATTN_BLOCK)]
        m = np.full((n, heads, T), -FLT_MAX, F32)
        l = np.zeros((n, heads, T), F32)
        o = np.zeros((n, heads, T, hd), F32)
        for bi, (j0, j1) in enumerate(blocks):
            Sb, vb = S[..., j0:j1], v[:, :, j0:j1]
            if fault == "last key block's length taken as 128" and not whole and j1 - j0 < ATTN_BLOCK:      # the rows past the last key: zeros
                extra = ATTN_BLOCK - (j1 - j0)
                Sb = np.concatenate([Sb, np.zeros(Sb.shape[:-1] + (extra,), F32)], -1)
                vb = np.concatenate([vb, np.zeros(vb.shape[:2] + (extra, hd), F32)], 2)
            mb = np.maximum(m, Sb.max(-1))
            if fault == "maximum frozen after the first block" and bi > 0:
                mb = m
            corr = np.exp((m - mb).astype(F32), dtype=F32)
            if fault == "correction factor dropped when the maximum rises" and bi > 0:
                corr = np.ones_like(corr)
            m = mb
            l = (l * corr).astype(F32)
            o = (o * corr[..., None]).astype(F32)
            P = np.exp((Sb - m[..., None]).astype(F32), dtype=F32)
            for j in range(Sb.shape[-1]):
                l = (l + P[..., j]).astype(F32)
                o = _fma(P[..., j, None], vb[:, :, j, None, :], o)
        y = (o / l[..., None]).astype(F32)
    return np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(n, T, heads * hd)


def attn_f32_runs(c, env):
    """does k::attention take an f32 kernel for this case under `env`?"""
    return not (int(dict(env).get("OAR_ATTN_X6", 1)) != 0 and c.hd == 32 and c.T > 32)


def _attn_form(c, env):
    if not attn_f32_runs(c, env):
        return "attention_x6",
    return f"attention {'whole' if attn_whole(c.T, c.hd) else 'stream'} HD={attn_hd_padded(c.hd)} T={c.T}",


def _attn_model(c, inp):
    g = GraphBuilder("attention_case")
    dim = c.heads * c.hd
    g.add_input("x", [c.n, c.T, 3 * dim])
    qkv = g.op("Reshape", ["x", g.init(np.array([0, -1, 3, c.heads, c.hd], np.int64), "shape")])
    qkv = g.op("Transpose", [qkv], perm=[2, 0, 3, 1, 4])
    q, k, v = g.op("Split", [qkv], n_out=3, axis=0)
    ax0 = g.init(np.array([0], np.int64), "axes")
    q, k, v = g.op("Squeeze", [q, ax0]), g.op("Squeeze", [k, ax0]), g.op("Squeeze", [v, ax0])
    q = g.op("Mul", [q, g.init(np.array(A.scale_of(c.hd), F32), "scale")])
    att = g.op("Softmax", [g.op("MatMul", [q, g.op("Transpose", [k], perm=[0, 1, 3, 2])])], axis=-1)
    o = g.op("Transpose", [g.op("MatMul", [att, v])], perm=[0, 2, 1, 3])
    g.add_output(g.op("Reshape", [o, g.init(np.array([0, -1, dim], np.int64), "shape")]), [c.n, c.T, dim])
    return g.model()


# ================================================================================================ the families' common face
_F = {
    "softmax": (SOFTMAX_CASES, SOFTMAX_FAULTS, _softmax_inputs, _softmax_ref, _softmax_emulate, _softmax_form, _softmax_model),
    "layernorm": (LN_CASES, LN_FAULTS, _ln_inputs, _ln_ref, _ln_emulate, _ln_form, _ln_model),
    "gemm": (GEMM_CASES, GEMM_FAULTS, _gemm_inputs, _gemm_ref, _gemm_emulate, _gemm_form, _gemm_model),
    "pool": (POOL_CASES, POOL_FAULTS, _pool_inputs, _pool_ref, _pool_emulate, _pool_form, _pool_model),
    "se": (SE_CASES, SE_FAULTS, _se_inputs, _se_ref, _se_emulate, _se_form, _se_model),
    "attention": (ATTN_CASES, ATTN_FAULTS, _attn_inputs, _attn_ref, _attn_emulate, _attn_form, _attn_model),
}
CASES = tuple(c for f in FAMILIES for c in _F[f][0])
FAULTS = {f: _F[f][1] for f in FAMILIES}
# every launch form of the kernels above, a template instantiation each: tests/test_row_cases_cpu.py wants a case for every one
ALL_FORMS = (("softmax wave", "softmax block", "softmax block over 64 KB")
             + tuple(f"layernorm v4x{nv}" for nv in (1, 2, 3, 4, 8)) + ("layernorm wave",)
             + ("gemm_batched linear tB=0", "gemm_batched linear tB=1", "gemm_batched matmul")
             + ("global_avgpool one pass", "global_avgpool split", "global_avgpool scalar", "reduce_mean", "pool2d avg", "pool2d max")
             + ("se_fc",)
             + tuple(f"attention {w} HD={hd}" for w in ("whole", "stream") for hd in (16, 32, 64)))
# the profiler classes of which no other launch may appear in a case's run
CLASS_OF = {"softmax": ("softmax",), "layernorm": ("layernorm",), "gemm": ("gemm_batched", "conv_igemm"), "pool": ("global_avgpool", "reduce_mean", "pool2d"),
            "se": ("se_fc", "global_avgpool", "conv_igemm"), "attention": ("attention", "attention_x6", "softmax", "gemm_batched")}


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def cases_of(family):
    return _F[family][0]


def group_of(c):
    """the child process a case runs in"""
    return "attention_f32" if c.family == "attention" and not attn_f32_runs(c, {}) else c.family


def inputs(c, kind, seed=0):
    """-> {name: f32 array}: the graph's inputs and its constants"""
    assert kind in c.kinds, (c.name, kind)
    return _F[c.family][2](c, kind, _rng(c, kind, seed))


def feed(c, inp):
    """the graph inputs among `inp`"""
    if c.family != "gemm":
        return {"x": inp["x"]}
    return {k: inp[k] for k in (("a", "r") if c.route == "linear" else ("a", "w")) if k in inp}


def model(c, inp):
    return _F[c.family][6](c, inp)


def ref(c, inp, dtype="float64"):
    with np.errstate(invalid="ignore", over="ignore"):
        return _F[c.family][3](c, inp, dtype)


def emulate(c, inp, fault=None):
    assert fault is None or fault in FAULTS[c.family], (c.family, fault)
    return _F[c.family][4](c, inp, fault)


def form(c, env=()):
    """-> the profiler names (OAR_PROF_DETAIL=1) of the case's own launches under the process switches `env`; (for the se family: the gate's launch and
    the pool's in front of it)"""
    names = _F[c.family][5](c, dict(env))
    if c.family == "se":
        names += _pool_form(_gap(c.N, c.C, c.H, c.W), env)
    return names


def form_key(c, env=()):
    """the entry of ALL_FORMS a case exercises (None: the case does not run an f32 kernel under `env`)"""
    if c.family == "softmax":
        return "softmax wave" if c.C <= 1024 else "softmax block over 64 KB" if c.C * 4 > 64 * 1024 else "softmax block"
    if c.family == "layernorm":
        return form(c, env)[0].split(" C=")[0]
    if c.family == "gemm":
        return "gemm_batched matmul" if c.route == "matmul" else f"gemm_batched linear tB={c.tB}"
    if c.family == "pool":
        if c.op == "gap":
            f = form(c, env)[0]
            return "global_avgpool scalar" if f.endswith("scalar") else "global_avgpool one pass" if f.endswith("splits=1") else "global_avgpool split"
        return {"mean": "reduce_mean", "avg": "pool2d avg", "max": "pool2d max"}[c.op]
    if c.family == "se":
        return "se_fc"
    return form(c, env)[0].split(" T=")[0] if attn_f32_runs(c, dict(env)) else None


def exact(c):
    """MaxPool: compared bit for bit"""
    return c.family == "pool" and c.op == "max"


def bundle(c, inp):
    """-> dict(f64, noise, tol) and, for gemm, (S, noise_S, tol_S) with tol = tol_S: see the module's head.  f64 is the reference of the graph's output (for
    gemm: behind the activation; the bound is S-normalised in front of it and ReLU neither moves nor widens it)."""
    f64 = ref(c, inp, "float64")
    if exact(c):
        return dict(f64=f64, noise=0.0, tol=0.0)
    if c.family == "gemm":
        lin = _gemm_ref(c, inp, "float64", act=False)
        S = _gemm_ref(c, inp, "float64", absolute=True, act=False)
        s1 = np.where(S > 0, S, 1.0)
        noise = max(float((np.abs(y.astype(np.float64) - lin) / s1).max()) for y in (_gemm_chain(c, inp), _gemm_ref(c, inp, "float32", act=False)))
        return dict(f64=f64, S=S, noise=noise, noise_S=noise, tol=4.0 * noise, tol_S=4.0 * noise)
    f32 = ref(c, inp, "float32").astype(np.float64)
    d = np.abs(f32 - f64)
    noise = float((d / f64).max()) if c.family == "softmax" else float(d.max())
    return dict(f64=f64, noise=noise, tol=max(16.0 * noise, FLOOR))


def error(c, got, b):
    """the output `got` against the bundle, in the units of its tol: relative per element (soft-max), S-normalised (gemm), 0 or inf (MaxPool: equal bit
    for bit or not), absolute (the rest); inf for a shape other than the reference's or a non-finite value where the reference is finite"""
    got, f64 = np.asarray(got), b["f64"]
    if got.shape != f64.shape:
        return float("inf")
    if exact(c):
        return 0.0 if np.array_equal(got.astype(np.float64), f64) else float("inf")
    if not np.isfinite(got).all():
        return float("inf")
    if c.family == "softmax":
        return float((np.abs(got.astype(np.float64) - f64) / f64).max())
    if c.family == "gemm":
        return err_S(got, f64, b["S"])
    return float(np.abs(got.astype(np.float64) - f64).max())


def jobs(c):
    """-> (key, model bytes, feed) per input family of the case"""
    for kind in c.kinds:
        inp = inputs(c, kind)
        yield (c.name, kind), model(c, inp), feed(c, inp)
