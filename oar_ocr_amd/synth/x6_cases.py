"""The bf16x6 arithmetic of the hot matrix kernels restated in numpy, with named faults, and the cases that hold the kernels to it.

Every bf16x6 kernel cuts an f32 operand into three exact bf16 slices x = h + m + l (`split3` in igemm_ws_x6.hip) and accumulates six of the nine slice
products -- (w plane, x plane) = mm, lh, hl, mh, hm, hh -- in f32, one 32-deep chunk of K at a time.  `x6_matmul` does the same on a GEMM view
[M, K] x [K, N]: the products of a chunk are formed exactly (f64 sums of products of bf16 values) and added to an f32 accumulator in the kernels' order.
`FAULTS` are the ways such a kernel goes wrong while staying 15 times inside the suite's 2e-4: tests/test_x6_cases_cpu.py shows that every case of
`GPU_CASES` tells each of them from the right arithmetic on its `cancel` family (only there: the other families' f32 noise hides a lost l-plane product), tests/test_gpu_x6_accuracy.py holds the kernels to the bound the right arithmetic meets.

All errors are measured against S = sum_k |x| |w| + |bias| (the operation on absolute values), not against the output: a cancelling sum is still
judged by the size of what was added.  CPU only: numpy."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32 = np.float32
_MASK = np.uint32(0xFFFF0000)

CLASSES = ("mm", "lh", "hl", "mh", "hm", "hh")   # (w plane, x plane), in the order the kernels add them: smallest terms first
DROPPED = ("ml", "lm", "ll")                     # left out by design
FAULTS = tuple(f"no {c}" for c in CLASSES) + ("x l zeroed", "w l zeroed", "x m/l swapped", "round to nearest", "mm twice")
FAMILIES = ("normal", "positive", "dense", "cancel", "pow2")
POISONS = ("nan", "inf")
POW2_X, POW2_W, POW2_B = 40, -25, 15             # pow2: x 2^40, w 2^-25, bias and output 2^15


# ------------------------------------------------------------------------------------------------ the split and the six-product GEMM
def split3(x):
    """-> (h, m, l) f32, bit for bit the device function: mask the upper 16 bits, subtract, mask again, subtract, mask again."""
    x = np.ascontiguousarray(x, F32)
    h = (x.view(np.uint32) & _MASK).view(F32)
    with np.errstate(invalid="ignore"):
        r1 = x - h
        m = (r1.view(np.uint32) & _MASK).view(F32)
        r2 = r1 - m
    l = (r2.view(np.uint32) & _MASK).view(F32)
    return h, m, l


def _rtn_bf16(x):
    """f32 -> nearest bf16 (ties to even), as f32"""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & _MASK).view(F32)


def _split_rtn(x):
    """the 'round to nearest' fault: two rounded slices, no third residual"""
    x = np.ascontiguousarray(x, F32)
    h = _rtn_bf16(x)
    m = _rtn_bf16(x - h)
    return h, m, np.zeros_like(x)


def x6_matmul(X, W, bias=None, order="chunk", fault=None, extra=(), chunk=32):
    """X [M, K] f32, W [K, N] f32, bias [N] f32 or None -> [M, N] f32 by the kernels' arithmetic.
    order 'chunk': one accumulator that starts at the bias; per 32-deep chunk the six classes are added to it in CLASSES order (igemm_ws_x6, igemm_os_x6,
    igemm_lk_x6 but for its bias).  order 'class': one accumulator per class over the whole K, the bias in hh's, summed smallest
    first at the end (igemm_rs3_x6).  order 'chunk, bias last': 'chunk' from zero, the bias added at the end.
    fault: one of FAULTS.  extra: classes of DROPPED to add as well (in front of the six)."""
    assert fault is None or fault in FAULTS, fault
    assert order in ("chunk", "class", "chunk, bias last"), order
    assert all(e in DROPPED for e in extra), extra
    X, W = np.asarray(X, F32), np.asarray(W, F32)
    M, K = X.shape
    N = W.shape[1]
    xs = dict(zip("hml", (_split_rtn if fault == "round to nearest" else split3)(X)))
    ws = dict(zip("hml", (_split_rtn if fault == "round to nearest" else split3)(W)))
    if fault == "x l zeroed":
        xs["l"] = np.zeros_like(X)
    if fault == "w l zeroed":
        ws["l"] = np.zeros_like(W)
    if fault == "x m/l swapped":
        xs["m"], xs["l"] = xs["l"], xs["m"]
    xs = {p: v.astype(np.float64) for p, v in xs.items()}
    ws = {p: v.astype(np.float64) for p, v in ws.items()}
    classes = [c for c in tuple(extra) + CLASSES if fault != f"no {c}"]
    if fault == "mm twice":
        classes = ["mm"] + classes
    b = np.zeros(N, F32) if bias is None else np.asarray(bias, F32)
    nch = -(-K // chunk)
    padk = lambda a, axis: np.concatenate([a, np.zeros([nch * chunk - K if i == axis else d for i, d in enumerate(a.shape)])], axis)
    xs = {p: padk(v, 1).reshape(M, nch, chunk).transpose(1, 0, 2) for p, v in xs.items()}     # [chunk index, M, 32]: a K tail is zero-padded, as W's is
    ws = {p: padk(v, 0).reshape(nch, chunk, N) for p, v in ws.items()}
    prod = {c: np.matmul(xs[c[1]], ws[c[0]]) for c in set(classes)}                              # [chunk index, M, N] f64: exact sums of exact products
    add = lambda acc, p: (acc.astype(np.float64) + p).astype(F32)                                # one f32 rounding per class and chunk
    if order == "class":
        accs = []
        for c in classes:
            acc = np.broadcast_to(b, (M, N)).copy() if c == "hh" else np.zeros((M, N), F32)
            for i in range(nch):
                acc = add(acc, prod[c][i])
            accs.append(acc)
        out = accs[0]
        for acc in accs[1:]:
            out = out + acc
        return out
    acc = np.zeros((M, N), F32) if order.endswith("last") else np.broadcast_to(b, (M, N)).copy()
    for i in range(nch):
        for c in classes:
            acc = add(acc, prod[c][i])
    return acc + b if order.endswith("last") else acc


# ------------------------------------------------------------------------------------------------ cases: one convolution each
@dataclass(frozen=True)
class Case:
    """One Conv (stride 1, padding k // 2, dilation 1) on an [n, cin, h, w] input, the profiler class it must run as and the emulator order of that kernel.
    group > 1: a grouped convolution (every group one launch of the kernel)."""
    name: str
    kernel: str
    n: int
    cin: int
    cout: int
    h: int
    w: int
    k: int = 1
    group: int = 1
    relu: bool = False
    order: str = "chunk"
    poison: str = "tile"       # where the one non-finite input element sits: see poison_at
    se: bool = False           # the convolution reads Mul(x, squeeze-excite gate): the gate is multiplied in as the pixels are loaded (se_gate)
    msrc: bool = False         # the convolution reads Concat(Relu(x), Neg(x), Abs(x)) of a cin / 3-channel input: three sources, the concatenation is never written

    @property
    def in_ch(self):
        return self.cin // 3 if self.msrc else self.cin

    @property
    def M(self):
        return self.n * self.h * self.w

    @property
    def K(self):
        return self.k * self.k * self.cin // self.group

    @property
    def N(self):
        return self.cout // self.group


# The smallest shapes the selection rules take (igemm.hip: igemm_weight_format, os_x6_eligible, conv_igemm; igemm_rs3_x6.hip: conv3x3_n16_x6_eligible;
# igemm_lk_x6.hip: conv_lk_x6_eligible), with pixel counts that are no multiple of any tile.  Every case runs every family.
GPU_CASES = (
    # weight-stationary: 1x1, K >= 96, N >= 96, ceil(M / 16) ceil(nfrag / 8) >= 4096 passes; PF = 2 from 98304 pixels
    Case("ws_x6 K96 pf1", "conv_igemm_ws_x6", 3, 96, 192, 100, 111, poison="tile"),
    Case("ws_x6 K104 pf1 relu", "conv_igemm_ws_x6", 3, 104, 192, 100, 111, relu=True, poison="ktail"),
    Case("ws_x6 K104 pf2", "conv_igemm_ws_x6", 3, 104, 192, 180, 183, poison="ktail"),
    Case("ws_x6 K96 pf2 relu", "conv_igemm_ws_x6", 3, 96, 192, 180, 183, relu=True, poison="tile"),
    Case("ws_x6 K96 pf1 gated", "conv_igemm_ws_x6", 3, 96, 192, 100, 111, se=True, poison=None),     # 11100 pixels per image: tiles straddle two images' gate rows
    Case("ws_x6 K104 pf2 gated", "conv_igemm_ws_x6", 3, 104, 192, 180, 183, se=True, poison=None),
    # output-stationary: Cin % 8, K >= 256, N >= 48, M >= 65536 or (M >= 8192 and 256 tiles of 256 pixels x 128 couts)
    Case("os_x6 3x3 32->1024", "conv_igemm_os_x6", 1, 32, 1024, 83, 100, k=3, poison="border"),
    Case("os_x6 3x3 40->64 K tail", "conv_igemm_os_x6", 1, 40, 64, 257, 256, k=3, relu=True, poison="ktail"),
    Case("os_x6 1x1 416->1024", "conv_igemm_os_x6", 1, 416, 1024, 83, 100, poison="tile"),
    Case("os_x6 1x1 3x144->1024 three sources", "conv_igemm_os_x6", 1, 432, 1024, 83, 100, msrc=True, poison="tile"),     # (the planner defers a Concat of >= 3 maps)
    Case("os_x6 grouped 3x3 2x(32->32)", "conv_igemm_os_x6", 1, 64, 64, 65, 67, k=3, group=2, poison="border"),
    # row-streaming 3x3: Cin 32 / 64 (wider: 64- and 32-channel passes that add to y), Cout <= 16, M >= 100000
    Case("rs3_x6 32->8", "conv_rs3_x6", 1, 32, 8, 317, 317, k=3, order="class", poison="border"),
    Case("rs3_x6 32->16 relu", "conv_rs3_x6", 1, 32, 16, 317, 317, k=3, relu=True, order="class", poison="tile"),
    Case("rs3_x6 32->12", "conv_rs3_x6", 1, 32, 12, 317, 317, k=3, order="class", poison="ktail"),
    Case("rs3_x6 64->8 relu", "conv_rs3_x6", 1, 64, 8, 317, 317, k=3, relu=True, order="class", poison="ktail"),
    Case("rs3_x6 64->12", "conv_rs3_x6", 1, 64, 12, 317, 317, k=3, order="class", poison="border"),
    Case("rs3_x6 64->16 relu", "conv_rs3_x6", 1, 64, 16, 317, 317, k=3, relu=True, order="class", poison="tile"),
    Case("rs3_x6 96->16 two passes", "conv_rs3_x6", 1, 96, 16, 317, 317, k=3, order="class", poison="border"),
    # large kernels from an LDS halo tile: 9x9 (Cout <= 64) and 5x5 / Cin = 32 (Cout <= 32), >= 128 tiles
    Case("lk_x6 9x9 32->24", "conv_lk_x6", 1, 32, 24, 66, 450, k=9, order="chunk, bias last", poison="border"),
    Case("lk_x6 5x5 32->32 relu", "conv_lk_x6", 1, 32, 32, 66, 370, k=5, relu=True, order="chunk, bias last", poison="tile"),
)


def case_by_name(name):
    return next(c for c in GPU_CASES if c.name == name)


# ------------------------------------------------------------------------------------------------ input families (all f32, seeded)
def _dense_bits(a, rng):
    """keep sign, exponent and the upper 7 mantissa bits; the low 16 bits from the upper half of their range: m and l slices near their maxima"""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    low = rng.integers(0x8000, 0x10000, size=u.shape, dtype=np.uint32)
    return ((u & _MASK) | low).view(F32)


def family_inputs(family, x_shape, w_shape, seed=0):
    """-> (x, w, bias) f32 for an input [n, cin, h, w] and a weight [cout, cin / group, k, k]; K = the weight's fan-in.
    normal: x N(0,1), w N(0,1) / sqrt(K), bias N(0,1).  positive: x U(1,2), w U(1,2) / K, bias U(1,2): every dropped term adds coherently.
    dense: positive with the low 16 mantissa bits of x and w from the upper half of their range.  cancel: positive where every odd input channel repeats
    the even one below it but for its low 8 mantissa bits, which are drawn again (the l slices differ), and its weights are minus the
    even channel's times (1 + 1e-3 N(0,1)), bias 1e-3 U(1,2): neighbours in k cancel, the output is about 1e-3 of S and so is every honest partial sum.
    pow2: the `normal` draw of the same seed with x 2^40, w 2^-25, bias 2^15 -- exact scalings, every slice far from subnormal and overflow."""
    assert family in FAMILIES, family
    cout, cg, kh, kw = w_shape
    K = cg * kh * kw
    base = "normal" if family == "pow2" else family
    rng = np.random.default_rng([seed, *x_shape, *w_shape, FAMILIES.index(base)])
    if base == "normal":
        x, w, b = rng.standard_normal(x_shape), rng.standard_normal(w_shape) / np.sqrt(K), rng.standard_normal(cout)
    else:
        x, w, b = rng.uniform(1, 2, x_shape), rng.uniform(1, 2, w_shape) / K, rng.uniform(1, 2, cout)
    x, w, b = x.astype(F32), w.astype(F32), b.astype(F32)
    if base == "dense":
        x, w = _dense_bits(x, rng), _dense_bits(w, rng)
    if base == "cancel":
        assert x_shape[1] % 2 == 0 and cg % 2 == 0
        u = x[:, 0::2].view(np.uint32)
        x[:, 1::2] = ((u & np.uint32(0xFFFFFF00)) | rng.integers(0, 256, size=u.shape, dtype=np.uint32)).view(F32)
        w[:, 1::2] = (-w[:, 0::2].astype(np.float64) * (1.0 + 1e-3 * rng.standard_normal(w[:, 0::2].shape))).astype(F32)
        b = (b * F32(1e-3)).astype(F32)
    if family == "pow2":
        x, w, b = np.ldexp(x, POW2_X), np.ldexp(w, POW2_W), np.ldexp(b, POW2_B)
    return np.ascontiguousarray(x, F32), np.ascontiguousarray(w, F32), np.ascontiguousarray(b, F32)


SE_ALPHA, SE_BETA = 0.25, 0.5


def se_gate(case):
    """-> (w1, b1, w2, b2, gate [cin]) of a squeeze-excite block whose gate does not depend on x: the second convolution's weights are zero, its bias is
    2, 0 or -1 by channel, so HardSigmoid(0.25, 0.5) gives exactly 1, 0.5 or 0.25 -- x times the gate is exact and the gated layer stays one linear
    product of known operands.  (One non-finite input would reach every gate of its image through the pool: the gated cases take no poison.)"""
    r = max(case.cin // 4, 8)
    rng = np.random.default_rng([case.cin, r])
    w1, b1 = (rng.standard_normal((r, case.cin, 1, 1)) / np.sqrt(case.cin)).astype(F32), rng.standard_normal(r).astype(F32)
    b2 = np.array([2.0, 0.0, -1.0], F32)[np.arange(case.cin) % 3]
    return w1, b1, np.zeros((case.cin, r, 1, 1), F32), b2, (F32(SE_ALPHA) * b2 + F32(SE_BETA)).astype(F32)


def gated(case, x):
    """what the convolution multiplies: x, x times the gate of se_gate, or the three sources side by side (all exact)"""
    if case.msrc:
        with np.errstate(invalid="ignore"):
            return np.concatenate([np.where(x < 0, F32(0), x), -x, np.abs(x)], 1)
    return x * se_gate(case)[4][None, :, None, None] if case.se else x


def case_inputs(case, family, seed=0):
    return family_inputs(family, (case.n, case.in_ch, case.h, case.w), (case.cout, case.cin // case.group, case.k, case.k), seed)


def poison_at(case):
    """-> (image, channel, row, column) of the one non-finite element of the `poison` inputs.
    'tile': the last pixel of the last image -- the last, partial pixel tile, whose other rows are clamped re-reads of this pixel.
    'ktail': the same pixel, last channel -- the 8-channel group that the zero-padded tail of the last 32-deep chunk reads again.
    'border': first row, last column of the last image -- the clamped address of every padding tap of the pixels next to it."""
    if case.poison == "tile":
        return case.n - 1, case.in_ch // 2, case.h - 1, case.w - 1
    if case.poison == "ktail":
        return case.n - 1, case.in_ch - 1, case.h - 1, case.w - 1
    assert case.poison == "border", case.poison
    return case.n - 1, case.in_ch - 1, 0, case.w - 1


def poison_inputs(case, kind, seed=0):
    """the `normal` inputs of the case with exactly one element of x set to NaN ('nan') or +inf ('inf')"""
    assert kind in POISONS, kind
    x, w, b = case_inputs(case, "normal", seed)
    x[poison_at(case)] = np.nan if kind == "nan" else np.inf
    return x, w, b


# ------------------------------------------------------------------------------------------------ references
def conv_ref(x, w, bias, group=1, dtype="float64", relu=False):
    """Conv, stride 1, padding k // 2, on [n, cin, h, w] -> [n, cout, h, w] in `dtype`: per tap one matrix product, the taps added in order, then the bias."""
    dt = np.dtype(dtype)
    n, cin, h, wd = x.shape
    cout, cg, kh, kw = w.shape
    og = cout // group
    xl = np.ascontiguousarray(np.asarray(x).transpose(0, 2, 3, 1)).astype(dt)
    xp = np.zeros((n, h + kh - 1, wd + kw - 1, cin), dt)
    xp[:, kh // 2:kh // 2 + h, kw // 2:kw // 2 + wd] = xl
    out = np.zeros((n * h * wd, cout), dt)
    wt = np.asarray(w).astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(group):
            for i in range(kh):
                for j in range(kw):
                    wij = wt[g * og:(g + 1) * og, :, i, j].T
                    if cg <= og:      # few input channels: copy the shifted window, multiply
                        out[:, g * og:(g + 1) * og] += xp[:, i:i + h, j:j + wd, g * cg:(g + 1) * cg].reshape(n * h * wd, cg) @ wij
                    else:             # few output channels: multiply the whole padded map, add the shifted window of the product
                        prod = (xp[..., g * cg:(g + 1) * cg].reshape(-1, cg) @ wij).reshape(n, h + kh - 1, wd + kw - 1, og)
                        out[:, g * og:(g + 1) * og] += prod[:, i:i + h, j:j + wd].reshape(n * h * wd, og)
        out += np.asarray(bias).astype(dt)
    if relu:
        out = np.where(out < 0, np.zeros((), dt), out)     # (NaN stays NaN)
    return np.ascontiguousarray(out.reshape(n, h, wd, cout).transpose(0, 3, 1, 2))


def sample_rows(case, rows=256):
    """`rows` output pixels of the case, evenly spread from the first to the last (corners and borders included)"""
    return np.unique(np.linspace(0, case.M - 1, rows).astype(np.int64))


def gemm_view(case, x, w, rows, cols=64):
    """-> X [len(rows), K], W [K, N'], the column indices: the im2col rows of the output pixels `rows` and the first `cols` output channels of group 0,
    k = (tap row, tap column, channel) as the kernels walk it."""
    n, cin, h, wd = x.shape
    cout, cg, kh, kw = w.shape
    xl = np.asarray(x, F32).transpose(0, 2, 3, 1)
    xp = np.zeros((n, h + kh - 1, wd + kw - 1, cg), F32)
    xp[:, kh // 2:kh // 2 + h, kw // 2:kw // 2 + wd] = xl[..., :cg]
    img, r = np.divmod(np.asarray(rows), h * wd)
    oy, ox = np.divmod(r, wd)
    X = np.stack([xp[img, oy + i, ox + j] for i in range(kh) for j in range(kw)], 1).reshape(len(rows), kh * kw * cg)
    nc = min(cols, cout // case.group)
    W = np.asarray(w, F32)[:nc].transpose(2, 3, 1, 0).reshape(kh * kw * cg, nc)
    return np.ascontiguousarray(X), np.ascontiguousarray(W), np.arange(nc)


def f32_matmul(X, W, b):
    """the plain f32 product: bias first, then k ascending, one rounding per multiplication and per addition (no library kernel: the same bits everywhere)"""
    X, W = np.asarray(X, F32), np.asarray(W, F32)
    acc = np.broadcast_to(np.asarray(b, F32), (X.shape[0], W.shape[1])).copy()
    for k in range(X.shape[1]):
        acc += X[:, k:k + 1] * W[k:k + 1, :]
    return acc


def gemm_bundle(X, W, b, order="chunk"):
    """The tolerance of one GEMM view -> dict(f64, S, noise_S, emu_S, tol_S).  noise_S: f32_matmul against f64; emu_S: the fault-free emulator against f64,
    both max |. - f64| / S; tol_S = 4 max(noise_S, emu_S): the kernels' summation order is neither of the two, a factor 4 over the larger of two honest f32
    orders covers a third."""
    X64, W64, b64 = X.astype(np.float64), W.astype(np.float64), np.asarray(b, np.float64)
    f64 = X64 @ W64 + b64
    S = np.abs(X64) @ np.abs(W64) + np.abs(b64)
    noise = float((np.abs(f32_matmul(X, W, b).astype(np.float64) - f64) / S).max())
    emu = float((np.abs(x6_matmul(X, W, b, order=order).astype(np.float64) - f64) / S).max())
    return dict(f64=f64, S=S, noise_S=noise, emu_S=emu, tol_S=4.0 * max(noise, emu))


def sample_bundle(case, x, w, bias):
    """gemm_bundle of the case's sample (sample_rows x gemm_view's columns) plus the view itself (X, W, b): what both test files take tol_S from"""
    X, W, cols = gemm_view(case, x, w, sample_rows(case))
    b = np.asarray(bias, F32)[cols]
    return dict(gemm_bundle(X, W, b, case.order), X=X, W=W, b=b)


def reference_bundle(case, x, w, bias):
    """The whole convolution -> dict(f64, S, noise_S, emu_S, tol_S): f64 and S as [n, cout, h, w] (activation none: the caller applies Relu, which does
    not enlarge an error); noise_S, emu_S and tol_S are those of sample_bundle."""
    sb = sample_bundle(case, x, w, bias)
    f64 = conv_ref(x, w, bias, case.group, "float64")
    S = conv_ref(np.abs(x), np.abs(w), np.abs(bias), case.group, "float64")
    return dict(f64=f64, S=S, noise_S=sb["noise_S"], emu_S=sb["emu_S"], tol_S=sb["tol_S"])


# ------------------------------------------------------------------------------------------------ fused kernels: the output is not linear in one product
# Each is compared with the same operation in float64; tolerance 4 max |f32 numpy - f64| on the same inputs (absolute: both sides share the output scale).
def act_ref(a, kind):
    if kind is None:
        return a
    if kind == "relu":
        return np.where(a < 0, a.dtype.type(0), a)
    assert kind == "hswish", kind
    t = a.dtype.type
    return a * np.clip(a * t(1.0 / 6.0) + t(0.5), t(0), t(1))


@dataclass(frozen=True)
class DsCase:
    """Conv(depthwise k x k, stride 1) + act -> Conv(1 x 1) + act as one kernel; `env`: the per-call switches that force the kernel `kernel`"""
    name: str
    kernel: str
    env: tuple
    c: int
    cout: int
    k: int
    n: int
    h: int
    w: int
    act: str = None


DS_CASES = (
    DsCase("dsblock_wa 48->48 3x3 relu", "dsblock_wa", (("OAR_DSBLOCK_RS", "0"), ("OAR_DSBLOCK_CS", "0")), 48, 48, 3, 2, 13, 35, "relu"),
    DsCase("dsblock 72->40 5x5", "dsblock", (("OAR_DSBLOCK_RS", "0"), ("OAR_DSBLOCK_WA", "0"), ("OAR_DSBLOCK_CS", "0")), 72, 40, 5, 1, 20, 36, None),
    DsCase("dsblock 96->96 3x3 relu", "dsblock", (("OAR_DSBLOCK_RS", "0"), ("OAR_DSBLOCK_WA", "0"), ("OAR_DSBLOCK_CS", "0")), 96, 96, 3, 2, 12, 37, "relu"),
    DsCase("dsblock_cs 192->192 5x5 relu", "dsblock_cs", (("OAR_DSBLOCK_CS", "2"),), 192, 192, 5, 2, 12, 40, "relu"),
)
FUSED_FAMILIES = ("normal", "positive", "pow2")


def ds_inputs(case, family, seed=0):
    """-> x [n, c, h, w], wd [c, 1, k, k], bd [c], wp [cout, c, 1, 1], bp [cout].  normal / positive as family_inputs for each of the two convolutions;
    pow2: `normal` with x 2^40, wd 2^-25, bd 2^15 (the depthwise output times 2^15), wp as it is, bp 2^15."""
    assert family in FUSED_FAMILIES, family
    base = "normal" if family == "pow2" else family
    x, wd, bd = family_inputs(base, (case.n, case.c, case.h, case.w), (case.c, 1, case.k, case.k), seed)
    _, wp, bp = family_inputs(base, (1, case.c, 1, 1), (case.cout, case.c, 1, 1), seed + 1)
    if family == "pow2":
        x, wd, bd, bp = np.ldexp(x, POW2_X), np.ldexp(wd, POW2_W), np.ldexp(bd, POW2_B), np.ldexp(bp, POW2_B)
    return x, wd, bd, wp, bp


def ds_ref(case, x, wd, bd, wp, bp, dtype="float64", fault=None):
    """-> [n, cout, h, w] in `dtype`; with `fault` the pointwise product runs through x6_matmul on the f32 depthwise output (the kernels' last product)"""
    dt = np.dtype(dtype)
    n, c, h, w = x.shape
    k = case.k
    xp = np.zeros((n, h + k - 1, w + k - 1, c), dt)
    xp[:, k // 2:k // 2 + h, k // 2:k // 2 + w] = np.asarray(x).transpose(0, 2, 3, 1).astype(dt)
    t = np.broadcast_to(np.asarray(bd).astype(dt), (n, h, w, c)).copy()
    for i in range(k):
        for j in range(k):
            t += xp[:, i:i + h, j:j + w] * np.asarray(wd)[:, 0, i, j].astype(dt)
    t = act_ref(t, case.act).reshape(-1, c)
    W = np.asarray(wp)[:, :, 0, 0].T
    if fault is not None:
        y = x6_matmul(t.astype(F32), W, bp, fault=fault or None).astype(dt)     # fault '': the fault-free emulator
    else:
        y = t @ W.astype(dt) + np.asarray(bp).astype(dt)
    return np.ascontiguousarray(act_ref(y, case.act).reshape(n, h, w, -1).transpose(0, 3, 1, 2))


def fused_bundle(ref_fn):
    """ref_fn(dtype) -> the operation in that dtype.  -> dict(f64, scale, noise, tol): noise = max |f32 - f64|, tol = 4 noise (absolute), scale = max |f64|"""
    f64 = ref_fn("float64")
    noise = float(np.abs(ref_fn("float32").astype(np.float64) - f64).max())
    return dict(f64=f64, scale=float(np.abs(f64).max()), noise=noise, tol=4.0 * noise)


ATTN_CASES = (("attention_x6 T33", 64, 2, 3, 33), ("attention_x6 T100", 96, 3, 2, 100))     # (name, dim, heads, images, tokens): head dim 32, T > 32


def attn_inputs(dim, heads, n, T, family, seed=0):
    """-> x [n, T, dim], w [dim, 3 dim], b [3 dim]: the projection in front of the attention kernel (normal / positive as above; positive weights / dim)"""
    assert family in ("normal", "positive"), family
    rng = np.random.default_rng([seed, dim, heads, n, T, FAMILIES.index(family)])
    if family == "normal":
        x, w, b = rng.standard_normal((n, T, dim)), rng.standard_normal((dim, 3 * dim)) / np.sqrt(dim), 0.1 * rng.standard_normal(3 * dim)
    else:
        x, w, b = rng.uniform(1, 2, (n, T, dim)), rng.uniform(1, 2, (dim, 3 * dim)) / dim, 0.1 * rng.uniform(1, 2, 3 * dim)
    return x.astype(F32), w.astype(F32), b.astype(F32)


def attn_ref(x, w, b, heads, dtype="float64", qkv=None):
    """Linear -> split into q, k, v [n, heads, T, hd] -> softmax(q hd^-0.5 k^T) v -> merge, in `dtype`.  qkv: the projection's output if given (f32), so
    that the attention alone is judged."""
    dt = np.dtype(dtype)
    n, T, dim = x.shape
    hd = dim // heads
    p = (np.asarray(x).astype(dt) @ np.asarray(w).astype(dt) + np.asarray(b).astype(dt)) if qkv is None else np.asarray(qkv).astype(dt)
    q, k, v = p.reshape(n, T, 3, heads, hd).transpose(2, 0, 3, 1, 4)
    s = (q * np.float32(hd ** -0.5).astype(dt)) @ k.transpose(0, 1, 3, 2)
    e = np.exp(s - s.max(-1, keepdims=True))
    o = (e / e.sum(-1, keepdims=True)) @ v
    return np.ascontiguousarray(o.transpose(0, 2, 1, 3).reshape(n, T, dim))


# ------------------------------------------------------------------------------------------------ the CTC head (ctc_head_x6.hip: Linear K -> V + soft-max + arg max, no logits written)
# A recognizer made for the test: Conv (48 x 8 kernel and stride: one time step per 8 columns) whose weights SELECT one pixel per feature (one 1.0 per
# output channel, so a feature is that normalised pixel plus a bias whatever the order of the sum) -> [n, T, K] -> Linear K -> V -> Softmax.  Nothing but
# the head lies between known f32 features and the output; the test takes the features from the engine on the graph cut in front of the Linear.
CTC_CASES = (("ctc_head_x6 K32", 32, 1100), ("ctc_head_x6 K64", 64, 1100), ("ctc_head_x6 K96", 96, 1100))     # (name, K, classes): K / 32 = 1, 2, 3 k-steps; 1100 -> 1104 padded
CTC_CROPS = (5, 48, 320)                                                                                     # crops, height, width: 40 time steps each
CTC_SIGMA = 3.0                                                                                               # `normal`: logits of std 3 -> the largest of 1100 probabilities is about 0.15


def ctc_inputs(K, V, family, seed=0):
    """-> crops (list of u8 [48, 320, 3]), sel [K, 3, 48, 8] one-hot, fb [K], w [K, V], b [V].  normal: pixels 0 .. 255 (features uniform in [-1, 1]),
    w N(0,1) CTC_SIGMA sqrt(3 / K), b N(0,1); positive: pixels 128 .. 255 and fb = 1 (features in [1, 2]), w U(1,2) / K, b U(1,2)."""
    assert family in ("normal", "positive"), family
    n, h, wd = CTC_CROPS
    rng = np.random.default_rng([seed, K, V, FAMILIES.index(family)])
    lo = 0 if family == "normal" else 128
    crops = [rng.integers(lo, 256, (h, wd, 3), dtype=np.uint8) for _ in range(n)]
    sel = np.zeros((K, 3 * h * 8), F32)
    sel[np.arange(K), rng.choice(3 * h * 8, K, replace=False)] = 1.0
    if family == "normal":
        fb, w, b = np.zeros(K), rng.standard_normal((K, V)) * (CTC_SIGMA * np.sqrt(3.0 / K)), rng.standard_normal(V)
    else:
        fb, w, b = np.ones(K), rng.uniform(1, 2, (K, V)) / K, rng.uniform(1, 2, V)
    return crops, sel.reshape(K, 3, h, 8), fb.astype(F32), w.astype(F32), b.astype(F32)


def ctc_pixels(crops):
    """[n, 3, 48, W] f32: the recognizer's input for crops that need no resize -- channels in B, G, R order, (pixel / 255 - 0.5) / 0.5"""
    return np.stack([(c[:, :, ::-1].astype(F32) / F32(255) - F32(0.5)) / F32(0.5) for c in crops]).transpose(0, 3, 1, 2)


def ctc_select(x, sel, fb):
    """the feature layer on x [n, 3, 48, W] -> [n T, K] f32: every feature one selected value of its 48 x 8 window plus fb"""
    n, _, h, wd = x.shape
    cols = np.asarray(x, F32).reshape(n, 3, h, wd // 8, 8).transpose(0, 3, 1, 2, 4).reshape(n * (wd // 8), 3 * h * 8)
    return (cols @ sel.reshape(sel.shape[0], -1).T + fb).astype(F32)


def ctc_features(crops, sel, fb):
    """the features in numpy alone: the CPU test's stand-in for what the engine computes"""
    return ctc_select(ctc_pixels(crops), sel, fb)


def ctc_ref(F, w, b, dtype="float64", fault=None):
    """features [M, K] f32 -> (arg max [M], its probability [M] in float64) of softmax(F w + b) computed in `dtype`; fault ('' = none): the product through
    x6_matmul, the soft-max of those f32 logits in float64"""
    dt = np.dtype(dtype)
    if fault is not None:
        z = x6_matmul(F, w, b, fault=fault or None).astype(np.float64)
    else:
        z = np.asarray(F).astype(dt) @ np.asarray(w).astype(dt) + np.asarray(b).astype(dt)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    idx = p.argmax(-1)
    return idx, p[np.arange(len(idx)), idx].astype(np.float64)
