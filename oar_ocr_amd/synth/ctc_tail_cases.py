"""Every route of the recognizer's CTC tail (vocabulary Linear -> soft-max -> last index of the row maximum), the rule that picks the route restated in
Python, and the float64 references with their bounds.

The recognizer is x6_cases' one-layer harness: a selecting convolution makes known f32 features [M, K], so nothing but the tail lies between known
inputs and the (index, probability) pairs.  `route` restates op_linear (engine.cc), igemm_weight_format / conv_igemm / ctc_partials_supported[_x6] /
ctc_tiles (igemm.hip), ctc_head_x6_supported (ctc_head_x6.hip) and the recognizer's fuse_tail rule (pipeline.cc); its Plan names per route the profiler
classes that must and must not have run.  tests/test_ctc_tail_cases_cpu.py holds the matrix to its own claims on the CPU (every route and cross has a
case, the families are what they say, three wrong references fall outside the bounds), tests/test_gpu_ctc_tail.py holds the kernels to the bounds.

CPU only: numpy."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import x6_cases as X
from .onnx_writer import GraphBuilder

F32 = np.float32
ROUTES = ("R1", "R2", "R3", "R4", "R5", "R6", "R7")
FLOOR = 2.0 ** -21      # relative floor of the probability bound: see `bounds`
SWITCHES = ("OAR_CTC_PARTIALS", "OAR_CTC_HEAD_OS", "OAR_IGEMM_X6")     # read once per process: a case that sets one runs in a child


# ------------------------------------------------------------------------------------------------ the graph
def ctc_model(K, V, sel, fb, w, b, head=True, spelling="matmul"):
    """[n, 3, 48, W] -> Conv 48 x 8 / stride 48 x 8 (one selected pixel per feature) -> [n, T, K] (head=False: the output) -> Linear K -> V -> Softmax.
    spelling 'matmul': MatMul + Add; 'gemm': one Gemm with transB = 1 and the bias as C."""
    assert spelling in ("matmul", "gemm"), spelling
    g = GraphBuilder("ctc")
    g.add_input("x", ["N", 3, 48, "W"])
    f = g.op("Conv", ["x", g.init(sel), g.init(fb)], kernel_shape=[48, 8], strides=[48, 8], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
    f = g.op("Transpose", [g.op("Squeeze", [f, g.init(np.array([2], np.int64), "axes")])], perm=[0, 2, 1])
    if not head:
        g.add_output(f, ["N", "T", K])
        return g.model()
    if spelling == "gemm":
        z = g.op("Gemm", [f, g.init(np.ascontiguousarray(np.asarray(w, F32).T)), g.init(b)], transB=1)
    else:
        z = g.op("Add", [g.op("MatMul", [f, g.init(w)]), g.init(b)])
    g.add_output(g.op("Softmax", [z], axis=2), ["N", "T", V])
    return g.model()


# ------------------------------------------------------------------------------------------------ the route rule
def pad16(V):
    return (V + 15) // 16 * 16


def ctc_tiles(n_padded):
    return ((n_padded + 15) // 16 + 7) // 8


def partials_supported(K):
    return K % 4 == 0 and K >= 32 and 8 * ((K + 15) // 16) * 1024 <= 150 * 1024


def partials_supported_x6(K):
    return K % 8 == 0 and K >= 32 and 8 * ((K + 31) // 32) * 3072 <= 150 * 1024


def _ws_x6_tile(K, nfrag):
    KC, best, nt = (K + 31) // 32, 1 << 30, 0
    for t in (8, 6, 4):
        if t * KC * 3072 > 150 * 1024:
            continue
        padded = -(-nfrag // t) * t
        if padded < best:
            best, nt = padded, t
    return nt


def _os_x6_eligible(M, K, N, Cin):
    tiles = -(-M // 256) * -(-N // 128)
    fills = M >= 65536 or (M >= 8192 and tiles >= 256) or (K >= 2048 and M >= 8192 and tiles >= 128)
    return Cin % 8 == 0 and K >= 256 and N >= 48 and N % 4 == 0 and fills and K < 65536


def passes(M, N):
    """(16-row tile, 128-column tile) pairs: what igemm_weight_format and conv_igemm's ws_auto compare with 4096"""
    return -(-M // 16) * -(-(-(-N // 16)) // 8)


def weight_format(M, K, N, env):
    """igemm_weight_format for a 1x1 layer -> 'x6' or 'f32'"""
    if int(env.get("OAR_IGEMM_X6", 1)) == 0:
        return "f32"
    nfrag = -(-N // 16)
    if K % 8 == 0 and K >= 96 and N >= 96 and N % 4 == 0 and passes(M, N) >= 4096 and _ws_x6_tile(K, nfrag) > 0:
        return "x6"
    return "x6" if _os_x6_eligible(M, K, N, K) else "f32"


def head_x6_supported(M, K, n_padded, env):
    return int(env.get("OAR_CTC_HEAD_OS", 1)) != 0 and M > 0 and K in (32, 64, 96) and n_padded >= 128 and n_padded % 16 == 0 and M * ctc_tiles(n_padded) * 16 < 1 << 40


@dataclass(frozen=True)
class Plan:
    route: str
    linear: str          # the profiler class of the vocabulary Linear
    C: int               # columns the soft-max runs over
    ld: int              # row stride of the logits (R1 .. R3: none are written; the padded width the partial tiles cover)
    tiles: int           # R1 .. R3: partial tiles per row
    must: frozenset
    must_not: frozenset


def _f32_linear_class(M, K, N):
    """conv_igemm's f32 choice for a plain 1x1 layer: the weight-stationary kernel where N % 4 == 0, K > 16 and the layer is wide and tall enough"""
    ws_auto = (N >= 96 and passes(M, N) >= 4096) or (K >= 512 and M >= 262144)
    return "conv_igemm_ws" if N % 4 == 0 and (K + 15) // 16 >= 2 and ws_auto else "conv_igemm"


def route(K, V, M, env=None):
    """-> Plan for a head of input width K and V classes on M rows, under the process switches `env` (the spelling does not enter: MatMul + Add and
    Gemm(transB, C) both become one Linear with a bias)."""
    env = dict(env or {})
    tails = {"ctc_combine", "softmax_argmax", "ctc_argmax", "softmax"}
    heads = {"ctc_head_x6", "conv_igemm_ws_x6", "conv_igemm_ws", "gemm_batched"}

    def plan(r, linear, C, ld, tiles, must):
        must = frozenset(must) | {linear}
        # (the feature layer is a convolution of its own: `conv_igemm` may always be there)
        return Plan(r, linear, C, ld, tiles, must, frozenset((tails | heads) - must))

    if V <= 1024:                                   # pipeline.cc: fuse_tail is V > 1024 -- the graph's own Softmax, then pp::ctc_argmax
        if K % 4:
            lin = "gemm_batched"
        elif weight_format(M, K, V, env) == "x6":
            lin = "conv_igemm_ws_x6"
        else:
            lin = _f32_linear_class(M, K, V)
        return plan("R7", lin, V, V, 0, {"softmax", "ctc_argmax"})
    if K % 4:                                       # op_linear: no padding, no igemm
        return plan("R6", "gemm_batched", V, V, 0, {"softmax_argmax"})
    if V % 16 == 0:                                 # nothing to pad: logits_valid stays 0, no partials
        lin = "conv_igemm_ws_x6" if weight_format(M, K, V, env) == "x6" else _f32_linear_class(M, K, V)
        return plan("R5", lin, V, V, 0, {"softmax_argmax"})
    Np = pad16(V)
    on = int(env.get("OAR_CTC_PARTIALS", 1)) != 0
    head = head_x6_supported(M, K, Np, env) and partials_supported_x6(K) and on
    fmt = "x6" if head else weight_format(M, K, Np, env)
    if on and (partials_supported_x6(K) if fmt == "x6" else partials_supported(K)):
        if fmt == "x6" and head_x6_supported(M, K, Np, env):      # conv_igemm asks again at launch: bf16x6 weights and a short K
            return plan("R1", "ctc_head_x6", V, Np, ctc_tiles(Np), {"ctc_combine"})
        if fmt == "x6":
            return plan("R3", "conv_igemm_ws_x6", V, Np, ctc_tiles(Np), {"ctc_combine"})
        return plan("R2", "conv_igemm_ws", V, Np, ctc_tiles(Np), {"ctc_combine"})
    lin = "conv_igemm_ws_x6" if fmt == "x6" else _f32_linear_class(M, K, Np)
    return plan("R4", lin, V, Np, 0, {"softmax_argmax"})


def detail_name(plan, M, K):
    """the prefix of the Linear's profiler name under OAR_PROF_DETAIL=1 (conv_igemm classes only; None where the class keeps its plain name)"""
    if not plan.linear.startswith("conv_igemm"):
        return None
    kind = {"conv_igemm": "conv_igemm", "conv_igemm_ws": "conv_igemm_ws", "conv_igemm_ws_x6": "conv_igemm_x6"}[plan.linear]
    return f"{kind} M={M} K={K} N={plan.ld} k1x1 s1"


def classes_ran(plan, names, M, K, detail=False):
    """-> (missing, forbidden): the route's classes that `names` lacks and the excluded ones it holds.  With detail names a conv_igemm class is looked
    for by its M / K / N, so that the feature layer cannot stand in for the head."""
    names = set(names)
    spelled = lambda c: "conv_igemm_x6" if detail and c == "conv_igemm_ws_x6" else c      # (the detail name of that class drops the `ws`)
    has = lambda c: any(n == spelled(c) or n.startswith(spelled(c) + " ") for n in names)
    missing = [c for c in plan.must if not has(c)]
    if detail and detail_name(plan, M, K) is not None:
        if not any(n.startswith(detail_name(plan, M, K)) for n in names):
            missing.append(detail_name(plan, M, K))
        missing = [c for c in missing if c != plan.linear]
    return sorted(missing), sorted(c for c in plan.must_not if has(c))


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    """One recognition call: `crops` crops of 48 x `width` (one batch, M = crops width / 8 rows) through a head K -> V.  family: normal / positive /
    negative (random inputs) or designed (the rows of `designed_rows`, one model each).  env: process switches (a child process)."""
    name: str
    route: str
    K: int
    V: int
    crops: int = 5
    width: int = 320
    family: str = "normal"
    spelling: str = "matmul"
    env: tuple = ()
    seam: bool = False        # also through the OrtInfer seam: the whole probability tensor (softmax_block_kernel above 1024 classes)

    @property
    def T(self):
        return self.width // 8

    @property
    def M(self):
        return self.crops * self.T

    @property
    def envd(self):
        return dict(self.env)

    def plan(self):
        return route(self.K, self.V, self.M, self.envd)


_BIG = dict(crops=45, width=360)      # 2025 rows: 127 row tiles x 33 column tiles = 4191 passes >= 4096 at V = 4113, and 2025 % 16 = 9
_ONE = dict(crops=1, width=320)       # a single crop alone in its batch: 40 rows, the fewest the 320-wide recognizer tensor gives
_P0, _H0, _X0 = (("OAR_CTC_PARTIALS", "0"),), (("OAR_CTC_HEAD_OS", "0"),), (("OAR_IGEMM_X6", "0"),)

CASES = (
    # R1: K = 32, 64, 96 -> ctc_head_x6, ctc_combine
    Case("r1 K32 V1100 normal", "R1", 32, 1100),
    Case("r1 K64 V2065 negative", "R1", 64, 2065, family="negative", seam=True),
    Case("r1 K96 V4113 positive", "R1", 96, 4113, family="positive"),
    Case("r1 K64 V2049 one crop", "R1", 64, 2049, **_ONE),                                  # 17 tiles, the last holds the single column 2048
    Case("r1 K32 V1100 385 rows", "R1", 32, 1100, crops=7, width=440, family="negative"),   # one row past the first 384-row workgroup
    Case("r1 K64 V1100 gemm", "R1", 64, 1100, spelling="gemm"),
    Case("r1 K64 V1025 fused from 1025", "R1", 64, 1025, seam=True),
    Case("r1 K96 V4113 many rows", "R1", 96, 4113, family="negative", **_BIG),              # (igemm_weight_format says bf16x6 by itself here)
    Case("r1 K64 V4113 designed", "R1", 64, 4113, family="designed", **_ONE),
    # R2: f32 weight-stationary kernel with the CTC epilogue
    Case("r2 K48 V1100 normal", "R2", 48, 1100),
    Case("r2 K48 V2049 negative one crop", "R2", 48, 2049, family="negative", **_ONE),
    Case("r2 K120 V4113 few rows", "R2", 120, 4113, family="positive"),
    Case("r2 K120 V1100 gemm negative", "R2", 120, 1100, family="negative", spelling="gemm", seam=True),
    Case("r2 K288 V2065 normal", "R2", 288, 2065),
    Case("r2 K288 V4113 negative", "R2", 288, 4113, family="negative"),
    Case("r2 K120 V4113 designed", "R2", 120, 4113, family="designed"),
    # R3: bf16x6 weight-stationary kernel with the CTC epilogue (K >= 96, passes >= 4096)
    Case("r3 K120 V4113 normal", "R3", 120, 4113, **_BIG),
    Case("r3 K120 V4113 negative", "R3", 120, 4113, family="negative", **_BIG),
    Case("r3 K192 V4113 positive", "R3", 192, 4113, family="positive", **_BIG),
    Case("r3 K192 V4097 negative", "R3", 192, 4097, family="negative", **_BIG),            # 33 tiles, the last holds the single column 4096
    Case("r3 K120 V4113 designed", "R3", 120, 4113, family="designed", **_BIG),
    # R4: padded logits, softmax_argmax(C = V, ld = Np)
    Case("r4 K16 V1100 normal", "R4", 16, 1100),
    Case("r4 K16 V2049 negative one crop", "R4", 16, 2049, family="negative", **_ONE),
    Case("r4 K384 V1100 positive", "R4", 384, 1100, family="positive"),
    Case("r4 K384 V4113 negative", "R4", 384, 4113, family="negative"),
    Case("r4 K384 V4113 many rows", "R4", 384, 4113, **_BIG),                               # the Linear on the bf16x6 kernel, logits written
    Case("r4 K16 V4113 designed", "R4", 16, 4113, family="designed"),
    Case("r4 K120 V1100 no partials", "R4", 120, 1100, env=_P0),
    Case("r4 K120 V2065 no partials negative", "R4", 120, 2065, family="negative", env=_P0),
    Case("r4 K64 V4113 no partials designed", "R4", 64, 4113, family="designed", env=_P0, **_ONE),
    Case("r4 K16 V18385", "R4", 16, 18385, family="positive", **_ONE),                      # the PP-OCRv5 mobile vocabulary: 73.5 KB of LDS per row, over 64 KB.  (positive: every
                                                                                            # column carries 1 / V of the sum; an in-order f32 sum of 18385 `normal` terms is noisier than 2^-16)
    # R5: V % 16 == 0 -> unpadded logits, softmax_argmax(C = ld = V)
    Case("r5 K64 V1104 normal", "R5", 64, 1104),
    Case("r5 K120 V2080 negative", "R5", 120, 2080, family="negative"),
    Case("r5 K48 V2080 designed", "R5", 48, 2080, family="designed", **_ONE),
    Case("r5 K64 V18400", "R5", 64, 18400, family="positive", **_ONE),
    # R6: K % 4 != 0 -> gemm_batched, softmax_argmax
    Case("r6 K30 V1100 normal", "R6", 30, 1100),
    Case("r6 K67 V2065 negative", "R6", 67, 2065, family="negative"),
    Case("r6 K67 V1104 positive", "R6", 67, 1104, family="positive"),
    Case("r6 K30 V1100 gemm one crop", "R6", 30, 1100, spelling="gemm", **_ONE),
    Case("r6 K67 V4113 designed", "R6", 67, 4113, family="designed"),
    Case("r6 K30 V18385", "R6", 30, 18385, family="positive", **_ONE),
    # R7: V <= 1024 -> the graph's Softmax, then pp::ctc_argmax
    Case("r7 K64 V97 normal", "R7", 64, 97, seam=True),
    Case("r7 K30 V97 negative", "R7", 30, 97, family="negative", seam=True),
    Case("r7 K64 V1024 positive", "R7", 64, 1024, family="positive", seam=True),
    Case("r7 K120 V1024 normal", "R7", 120, 1024, seam=True),
    Case("r7 K64 V1024 designed", "R7", 64, 1024, family="designed", **_ONE),
    # crosses: the switches turn one route's shape into another route
    Case("r2 K64 V1100 head kernel off", "R2", 64, 1100, env=_H0),
    Case("r2 K96 V4113 head kernel off negative", "R2", 96, 4113, family="negative", env=_H0),
    Case("r2 K64 V4113 head kernel off designed", "R2", 64, 4113, family="designed", env=_H0, **_ONE),
    Case("r2 K120 V4113 many rows f32", "R2", 120, 4113, env=_X0, **_BIG),
    Case("r2 K192 V4113 many rows f32 negative", "R2", 192, 4113, family="negative", env=_X0, **_BIG),
    # the default environment once more with detail names, one case per route whose Linear is a conv_igemm class
    Case("r2 K120 V1100 detail", "R2", 120, 1100, env=(("OAR_PROF_DETAIL", "1"),)),
    Case("r3 K120 V4113 detail", "R3", 120, 4113, env=(("OAR_PROF_DETAIL", "1"),), **_BIG),
    Case("r4 K384 V1100 detail", "R4", 384, 1100, env=(("OAR_PROF_DETAIL", "1"),)),
    Case("r5 K64 V1104 detail", "R5", 64, 1104, env=(("OAR_PROF_DETAIL", "1"),)),
)

# the OrtInfer seam above 1024 classes (softmax_block_kernel) is asked for at exactly these sizes; the cases marked `seam` cover them
SEAM_SIZES = (1025, 1100, 2065)


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def env_groups():
    """-> {env tuple: [cases]} of the cases that need a child process, one child per distinct environment"""
    out = {}
    for c in CASES:
        if c.env:
            out.setdefault(c.env, []).append(c)
    return out


def tensor_width(widths, heights, img_h=48, img_w=320, max_img_w=3200):
    """host::rec_tensor_width in f32, as the recognizer computes it"""
    r = F32(img_w) / F32(img_h)
    for w, h in zip(widths, heights):
        r = max(r, F32(w) / F32(h))
    return min(int(F32(img_h) * F32(r)), max_img_w)


# ------------------------------------------------------------------------------------------------ inputs
def inputs(case, seed=0):
    """-> crops, sel, fb, w, b of a random-family case.  normal / positive: x6_cases.ctc_inputs at the case's crop count and width.  negative: `normal`
    with the bias lowered by (largest float64 logit of any row + 1), so that every real logit is below 0 and a padded column (logit 0) wins wherever
    a mask is missing."""
    assert case.family in ("normal", "positive", "negative"), case.family
    fam = "positive" if case.family == "positive" else "normal"
    n, h = case.crops, 48
    rng = np.random.default_rng([seed, case.K, case.V, case.crops, case.width, X.FAMILIES.index(fam)])
    lo = 0 if fam == "normal" else 128
    crops = [rng.integers(lo, 256, (h, case.width, 3), dtype=np.uint8) for _ in range(n)]
    K, V = case.K, case.V
    sel = np.zeros((K, 3 * h * 8), F32)
    sel[np.arange(K), rng.choice(3 * h * 8, K, replace=False)] = 1.0
    if fam == "normal":
        fb, w, b = np.zeros(K), rng.standard_normal((K, V)) * (X.CTC_SIGMA * np.sqrt(3.0 / K)), rng.standard_normal(V)
    else:
        fb, w, b = np.ones(K), rng.uniform(1, 2, (K, V)) / K, rng.uniform(1, 2, V)
    sel, fb, w, b = sel.reshape(K, 3, h, 8), fb.astype(F32), w.astype(F32), b.astype(F32)
    if case.family == "negative":
        z = logits64(X.ctc_features(crops, sel, fb), w, b)
        b = (b.astype(np.float64) - (z.max() + 1.0)).astype(F32)
    return crops, sel, fb, w, b


def logits64(F, w, b):
    return np.asarray(F, np.float64) @ np.asarray(w, np.float64) + np.asarray(b, np.float64)


@dataclass(frozen=True)
class Row:
    """One designed model: every row of the call has the same logits.  answer: the index every row must give."""
    name: str
    w: np.ndarray
    b: np.ndarray
    answer: int
    tie: tuple = ()       # the columns that share the maximum (answer = the last of them)


def pair_placements(V):
    """-> {name: (j1, j2)} where the repeated maximum sits, for the tile geometry of V (128-column tiles; ctc_combine's lane l takes tiles l, l + 16, ...)"""
    tiles = ctc_tiles(pad16(V))
    last0 = 128 * (tiles - 1)                                  # first column of the last tile
    out = {"one fragment": (3, 9), "across a tile": (100, 130), "other lanes": (300, 700), "into the last tile": (50, max(V - 2, last0))}
    if tiles > 17:
        out["same lane"] = (128 + 2, 128 * 17 + 5)                       # tiles 1 and 17
    elif tiles == 17:
        out["same lane"] = (2, 128 * 16 + (V - 1 - 128 * 16) // 2)        # tiles 0 and 16
    return {k: v for k, v in out.items() if v[0] < v[1] < V}


def designed_rows(case, seed=0):
    """-> crops, sel, fb, [Row].  All but the last have w = 0 (the logits are the bias, exactly, in every kernel: the bias enters the accumulation first
    and b + 0 is exact).  The bias is -1 - |N(0,1)| everywhere but at the named columns:
      pair rows      the maximum -0.25 at two columns -- below the padding's 0 -- the answer is the later one;
      zero max       0.0 at one real column: ties with the padding, which must never win;
      first / last   the maximum at column 0, at column V - 1;
      twin columns   the `normal` weights with column j2 a copy of column j1 and both biases raised so that the pair is every row's maximum: the
                     last index wins where the products are not trivially exact."""
    K, V = case.K, case.V
    rng = np.random.default_rng([seed, K, V, 7])
    base = replace_family(case, "normal")
    crops, sel, fb, wn, bn = inputs(base, seed)
    low = (-1.0 - np.abs(rng.standard_normal(V))).astype(F32)
    zero = np.zeros((K, V), F32)
    rows = []
    for name, (j1, j2) in pair_placements(V).items():
        b = low.copy()
        b[[j1, j2]] = -0.25
        rows.append(Row(f"pair {name} {j1},{j2}", zero, b, j2, (j1, j2)))
    j0 = V - 1 if pad16(V) != V else V // 2          # the column next to the padding where there is one
    b = low.copy(); b[j0] = 0.0
    rows.append(Row(f"zero max at {j0}", zero, b, j0))
    for j in (0, V - 1):
        b = low.copy(); b[j] = 0.5
        rows.append(Row(f"max at {j}", zero, b, j))
    j1, j2 = 5, V - 1
    w, b = wn.copy(), bn.copy()
    w[:, j2] = w[:, j1]
    z = logits64(X.ctc_features(crops, sel, fb), w, b)
    z[:, [j1, j2]] = -np.inf
    lift = F32(np.ceil(z.max() + 4.0 + np.abs(logits64(X.ctc_features(crops, sel, fb), w[:, j1:j1 + 1], 0.0)).max()))
    b[[j1, j2]] = lift
    rows.append(Row(f"twin columns {j1},{j2}", w, b, j2, (j1, j2)))
    return crops, sel, fb, rows


def replace_family(case, family):
    from dataclasses import replace
    return replace(case, family=family)


# ------------------------------------------------------------------------------------------------ references and bounds
def softmax64(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def last_argmax(p):
    """last index of the row maximum"""
    return p.shape[-1] - 1 - np.argmax(p[..., ::-1], axis=-1)


def _f32_softmaxes(F, w, b):
    """two honest f32 evaluations of the soft-max of the f32 head: exp of (logit - max) in f32, the sum pairwise (numpy's) and in order (cumsum)"""
    z = (np.asarray(F, F32) @ np.asarray(w, F32) + np.asarray(b, F32)).astype(F32)
    e = np.exp(z - z.max(-1, keepdims=True), dtype=F32)
    s_pair = e.sum(-1, dtype=F32, keepdims=True)
    s_ord = np.cumsum(e, axis=-1, dtype=F32)[..., -1:]
    return e / s_pair, e / s_ord


def bounds(F, w, b, tie=()):
    """features [M, K] f32 -> dict of the float64 reference and what the tail is held to:
      idx, p       last arg max and its probability in float64 (tie: columns whose logits are made exactly equal first -- identical columns of w);
      P            the whole float64 soft-max [M, V];
      noise        max |p32 - p| over two honest f32 evaluations (pairwise and in-order sums);  tol = max(4 noise, 2^-21 p) per row.
                   The floor is igemm_ctc_epilogue's own account: __expf at about 2 ulp per term, <= 2^-22 relative on the sum, and as much again for
                   the roundings of 1 / S and of ctc_combine's merge;
      clear        rows whose float64 runner-up lies further below the winner than tol (ties of `tie` apart);
      noise_full   max |P32 - P| / max_j P over the whole tensor;  tol_full = max(4 noise_full, 2^-21), relative to the row's largest probability;
      tol_sum      max(4 max |sum_j P32 - 1|, 2^-21): the same form on the row sums, whose reference is 1."""
    if len(F) > 1 and not np.asarray(w).any():      # w = 0: every row is the first
        one = bounds(F[:1], w, b, tie)
        return {k: np.broadcast_to(v, (len(F),) + v.shape[1:]) if isinstance(v, np.ndarray) else v for k, v in one.items()}
    z = logits64(F, w, b)
    if tie:
        assert np.abs(z[:, tie[0]] - z[:, tie[1]]).max() <= 1e-12 * np.abs(z).max()
        z[:, tie[1]] = z[:, tie[0]]
    P = softmax64(z)
    idx = last_argmax(P)
    rows = np.arange(len(idx))
    p = P[rows, idx]
    pa, pb = _f32_softmaxes(F, w, b)
    noise = max(float(np.abs(pa[rows, idx] - p).max()), float(np.abs(pb[rows, idx] - p).max()))
    tol = np.maximum(4.0 * noise, FLOOR * p)
    Q = P.copy()
    Q[rows, idx] = -1.0
    if tie:
        Q[:, list(tie)] = -1.0
    clear = p - Q.max(-1) > tol
    pm = P.max(-1, keepdims=True)
    noise_full = max(float((np.abs(pa - P) / pm).max()), float((np.abs(pb - P) / pm).max()))
    noise_sum = max(float(np.abs(pa.sum(-1, dtype=np.float64) - 1.0).max()), float(np.abs(pb.sum(-1, dtype=np.float64) - 1.0).max()))
    return dict(idx=idx, p=p, P=P, noise=noise, tol=tol, clear=clear, noise_full=noise_full, tol_full=max(4.0 * noise_full, FLOOR),
                tol_sum=max(4.0 * noise_sum, FLOOR))


def check(bundle, idx, prob, V):
    """the GPU's (index, probability) per row against `bounds` -> dict(err, ratio = max err / tol, bad_index = clear rows whose index differs,
    out_of_range = rows with an index outside [0, V))"""
    idx, prob = np.asarray(idx).reshape(-1), np.asarray(prob, np.float64).reshape(-1)
    err = np.abs(prob - bundle["p"])
    return dict(err=float(err.max()), ratio=float((err / bundle["tol"]).max()),
                bad_index=np.flatnonzero(bundle["clear"] & (idx != bundle["idx"])), out_of_range=np.flatnonzero((idx < 0) | (idx >= V)))


# three wrong tails: what a missing mask, the other tie rule and a short merge would give
def wrong_padded(F, w, b):
    """the soft-max taken over the 16-padded width: the padding's logit 0 takes part"""
    z = logits64(F, w, b)
    z = np.concatenate([z, np.zeros((len(z), pad16(z.shape[1]) - z.shape[1]))], 1)
    P = softmax64(z)
    idx = last_argmax(P)
    return idx, P[np.arange(len(idx)), idx]


def wrong_first(F, w, b, tie=()):
    """first index of the row maximum"""
    z = logits64(F, w, b)
    if tie:
        z[:, tie[1]] = z[:, tie[0]]
    P = softmax64(z)
    idx = P.argmax(-1)
    return idx, P[np.arange(len(idx)), idx]


def wrong_merge(F, w, b):
    """a merge that reads 16 tiles and stops: the columns from 2048 on never take part"""
    P = softmax64(logits64(F, w, b)[:, :2048])
    idx = last_argmax(P)
    return idx, P[np.arange(len(idx)), idx]
