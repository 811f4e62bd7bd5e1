"""An independent statement of the engine's second operator family (comparisons, logic, select, rounding, Pow, reductions, arg-reductions, broadcast
copies, generators, Pad, Transpose, Cast, Resize) in plain NumPy: one small function per operator that says the ONNX rule directly.

Nothing here repeats the engine's arithmetic or oracle/onnx_ref.py's (no torch, no f32 coordinate tricks):

* exact operators take np.float32 (or np.int64 / np.bool_) arrays and return the same types -- IEEE f32 add / sub / mul / div / sqrt, comparisons, selections
  and copies have ONE right answer, and the library is compiled without fast-math and without contraction, so its kernels must give those bits;
* Pow and linear Resize are computed in float64 (returned as float64: the caller compares under a tolerance);
* the nearest-Resize index map is computed in exact rationals (fractions.Fraction);
* integer tensors follow the integer rules: Div truncates toward zero, Cast float -> int truncates toward zero, Cast -> bool is `!= 0`.

NaN is out of scope everywhere (fmaxf / fminf and the arg-reductions deliberately do not follow NumPy there).
`apply(op, inputs, attrs)` dispatches by operator name; oracle/op_cases.py builds every test graph through it, node by node."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32 = np.float32
I64 = np.int64


def _is_int(*xs):
    return all(np.asarray(x).dtype.kind in "iu" for x in xs)


def _same_kind(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert (a.dtype.kind == "f") == (b.dtype.kind == "f"), "ONNX binary operators take operands of one type"
    return a, b


# ------------------------------------------------------------------------------------------------ arithmetic
def add(a, b):
    a, b = _same_kind(a, b)
    return a + b


def sub(a, b):
    a, b = _same_kind(a, b)
    return a - b


def mul(a, b):
    a, b = _same_kind(a, b)
    return a * b


def div(a, b):
    """floats: IEEE division; integers: C division, the quotient truncated toward zero (-7 / 2 == -3)"""
    a, b = _same_kind(a, b)
    if _is_int(a, b):
        q = np.abs(a) // np.abs(b)
        return (np.where((a < 0) != (b < 0), -q, q)).astype(I64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return a / b


def pow_(a, b):
    """float64 for floats (the caller allows a tolerance); exact integer powers for integers"""
    a, b = _same_kind(a, b)
    if _is_int(a, b):
        return np.power(a.astype(I64), b.astype(I64))
    with np.errstate(all="ignore"):
        return np.power(a.astype(np.float64), b.astype(np.float64))


def max_(a, b):
    """the larger VALUE; between +0.0 and -0.0 (equal values) either may come back -- compare with `canon_zero`"""
    a, b = _same_kind(a, b)
    return np.where(a > b, a, b)


def min_(a, b):
    a, b = _same_kind(a, b)
    return np.where(a < b, a, b)


def sqrt(x):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(x, F32))


# ------------------------------------------------------------------------------------------------ comparisons, logic, select
def equal(a, b):
    return np.asarray(a) == np.asarray(b)


def less(a, b):
    return np.asarray(a) < np.asarray(b)


def greater(a, b):
    return np.asarray(a) > np.asarray(b)


def truth(x):
    return np.asarray(x) != 0


def and_(a, b):
    return truth(a) & truth(b)


def or_(a, b):
    return truth(a) | truth(b)


def not_(x):
    return ~truth(x)


def where(c, a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.where(truth(c), a, b)


# ------------------------------------------------------------------------------------------------ unary
def floor(x):
    return np.floor(x)


def ceil(x):
    return np.ceil(x)


def round_(x):
    """half to even, the sign of zero kept (Round(-0.5) == -0.0)"""
    return np.rint(x)


def abs_(x):
    return np.abs(x)


def neg(x):
    return -np.asarray(x)


def clip(x, lo=None, hi=None):
    """an absent bound is no bound (+-inf pass)"""
    x = np.asarray(x)
    if lo is not None:
        x = np.where(x < lo, np.asarray(lo, x.dtype), x)
    if hi is not None:
        x = np.where(x > hi, np.asarray(hi, x.dtype), x)
    return x


def cast(x, to):
    """to: ONNX element type -- 1 float, 6 / 7 integers (truncation toward zero), 9 bool (`!= 0`)"""
    x = np.asarray(x)
    if to == 9:
        return x != 0
    if to in (6, 7):
        return np.trunc(x).astype(I64) if x.dtype.kind == "f" else x.astype(I64)
    if to == 1:
        return x.astype(F32)
    raise NotImplementedError(to)


# ------------------------------------------------------------------------------------------------ reductions
def _axes(x, axes):
    r = np.ndim(x)
    return tuple(range(r)) if axes is None or len(axes) == 0 else tuple(sorted(int(a) % r for a in axes))


def reduce(kind, x, axes=None, keepdims=1):
    """ReduceSum / ReduceProd / ReduceMax / ReduceMin.  Sum and product are formed in float64 and must be EXACT there and in f32 (the inputs are chosen
    so that no order of evaluation rounds): anything else is refused, because then there is no single right f32 answer."""
    x = np.asarray(x)
    ax = _axes(x, axes)
    kd = bool(keepdims)
    if kind in ("max", "min"):
        return (np.max if kind == "max" else np.min)(x, axis=ax, keepdims=kd)
    if _is_int(x):
        return (np.sum if kind == "sum" else np.prod)(x, axis=ax, keepdims=kd, dtype=I64)
    if kind == "sum":    # multiples of 1/8 whose magnitudes sum below 2^21: every partial sum, in any order, is exact in f32
        assert np.array_equal(x * 8, np.rint(x * 8)) and np.abs(x.astype(np.float64)).sum(axis=ax).max(initial=0.0) < 2.0 ** 21, "ReduceSum: inputs that sum exactly only"
    else:                # +-powers of two with a bounded exponent sum: every partial product is one too
        m, e = np.frexp(np.abs(x))
        assert np.all(m == 0.5) and np.abs(e - 1).sum(axis=ax).max(initial=0) <= 100, "ReduceProd: +-powers of two only"
    wide = (np.sum if kind == "sum" else np.prod)(x.astype(np.float64), axis=ax, keepdims=kd)
    out = wide.astype(F32)
    assert np.array_equal(out.astype(np.float64), wide)
    return out


def argreduce(x, axis=0, keepdims=1, select_last_index=0, is_min=False):
    """index of the extreme value along `axis`; among equal values (+0.0 == -0.0) the first, or the last with select_last_index"""
    x = np.asarray(x)
    axis = int(axis) % x.ndim
    n = x.shape[axis]
    ext = (np.min if is_min else np.max)(x, axis=axis, keepdims=True)
    hit = x == ext
    pos = np.arange(n).reshape([n if d == axis else 1 for d in range(x.ndim)])
    idx = np.where(hit, pos, -1).max(axis=axis) if select_last_index else np.where(hit, pos, n).min(axis=axis)
    idx = idx.astype(I64)
    return np.expand_dims(idx, axis) if keepdims else idx


# ------------------------------------------------------------------------------------------------ copies and generators
def expand(x, shape):
    x = np.asarray(x)
    return np.broadcast_to(x, np.broadcast_shapes(x.shape, tuple(int(v) for v in shape))).copy()


def tile(x, repeats):
    return np.tile(np.asarray(x), tuple(int(v) for v in repeats))


def transpose(x, perm=None):
    return np.ascontiguousarray(np.transpose(np.asarray(x), perm))


def constant_of_shape(shape, value=None):
    v = np.zeros(1, F32) if value is None else np.asarray(value).reshape(-1)
    return np.full(tuple(int(s) for s in shape), v[0], dtype=v.dtype)


def range_(start, limit, delta):
    """max(ceil((limit - start) / delta), 0) elements start + i * delta, in exact rationals, then the input type"""
    dt = np.asarray(start).dtype
    s, l, d = (Fraction(float(np.asarray(v).reshape(-1)[0])) if dt.kind == "f" else Fraction(int(np.asarray(v).reshape(-1)[0])) for v in (start, limit, delta))
    n = max(math.ceil((l - s) / d), 0)
    vals = [s + i * d for i in range(n)]
    return np.array([float(v) for v in vals], dtype=dt) if dt.kind == "f" else np.array([int(v) for v in vals], dtype=I64)


def pad(x, pads, mode="constant", value=0.0, axes=None):
    """ONNX Pad: negative pads crop FIRST; what is left is then padded (constant / edge / reflect without repeating the edge; a length-1 axis reflects
    onto its only element)."""
    x = np.asarray(x)
    r = x.ndim
    pads = [int(v) for v in pads]
    ax = list(range(r)) if axes is None else [int(a) % r for a in axes]
    assert len(pads) == 2 * len(ax)
    before, after = [0] * r, [0] * r
    for k, a in enumerate(ax):
        before[a], after[a] = pads[k], pads[len(ax) + k]
    index = []
    inside = np.ones([1] * r, bool)
    for d in range(r):
        lo, hi = max(-before[d], 0), x.shape[d] - max(-after[d], 0)      # the kept part [lo, hi) of the axis
        assert hi >= lo
        kept = hi - lo
        n_out = max(before[d], 0) + kept + max(after[d], 0)
        c = np.arange(n_out) - max(before[d], 0)                         # position in the kept part
        ok = (c >= 0) & (c < kept)
        if mode == "edge":
            c = np.clip(c, 0, kept - 1)
        elif mode == "reflect":
            if kept == 1:
                c = np.zeros_like(c)
            else:
                assert max(before[d], after[d], 0) < kept, "reflect wider than the axis"
                c = np.where(c < 0, -c, np.where(c >= kept, 2 * (kept - 1) - c, c))
        else:
            c = np.clip(c, 0, max(kept - 1, 0))
            shape = [1] * r
            shape[d] = n_out
            inside = inside & ok.reshape(shape)
        index.append(c + lo)
    y = x[np.ix_(*index)]
    if mode == "constant":
        y = np.where(inside, y, np.asarray(value, x.dtype).reshape(()))
    return np.ascontiguousarray(y)


# ------------------------------------------------------------------------------------------------ Resize
CTMS = ("asymmetric", "half_pixel", "pytorch_half_pixel", "align_corners")
NEAREST_MODES = ("floor", "ceil", "round_prefer_floor", "round_prefer_ceil")


def resize_coord(o: int, n_in: int, n_out: int, scale: Fraction, ctm: str) -> Fraction:
    """the source coordinate of output index o, as the Resize text gives it (x_resized -> x_original)"""
    if ctm == "asymmetric":
        return Fraction(o) / scale
    if ctm == "half_pixel":
        return (Fraction(o) + Fraction(1, 2)) / scale - Fraction(1, 2)
    if ctm == "pytorch_half_pixel":
        return (Fraction(o) + Fraction(1, 2)) / scale - Fraction(1, 2) if n_out > 1 else Fraction(0)
    if ctm == "align_corners":
        return Fraction(o * (n_in - 1), n_out - 1) if n_out > 1 else Fraction(0)
    raise NotImplementedError(ctm)


def nearest_index(n_in: int, n_out: int, scale: Fraction, ctm: str, nearest_mode: str) -> np.ndarray:
    """[n_out] source indices, exact"""
    out = []
    for o in range(n_out):
        x = resize_coord(o, n_in, n_out, scale, ctm)
        if nearest_mode == "floor":
            i = math.floor(x)
        elif nearest_mode == "ceil":
            i = math.ceil(x)
        elif nearest_mode == "round_prefer_floor":
            i = math.ceil(x - Fraction(1, 2))
        elif nearest_mode == "round_prefer_ceil":
            i = math.floor(x + Fraction(1, 2))
        else:
            raise NotImplementedError(nearest_mode)
        out.append(min(max(i, 0), n_in - 1))
    return np.array(out, I64)


def _resize_geometry(x, scales, sizes):
    """(out length, scale as a rational) for H and W: `sizes` gives out / in; `scales` gives the f32 scale itself and out = floor(in * scale)"""
    geo = []
    for ax in (2, 3):
        n_in = x.shape[ax]
        if sizes is not None and len(sizes):
            n_out = int(sizes[ax])
            geo.append((n_out, Fraction(n_out, n_in)))
        else:
            s = Fraction(float(F32(scales[ax])))
            geo.append((math.floor(n_in * s), s))
    return geo


def resize(x, scales=None, sizes=None, mode="nearest", ctm="half_pixel", nearest_mode="round_prefer_floor"):
    """NCHW Resize over H and W.  nearest: a gather through the exact index maps (bit-exact result).  linear: float64."""
    x = np.asarray(x)
    (ho, sh), (wo, sw) = _resize_geometry(x, scales, sizes)
    if mode == "nearest":
        iy, ix = nearest_index(x.shape[2], ho, sh, ctm, nearest_mode), nearest_index(x.shape[3], wo, sw, ctm, nearest_mode)
        return np.ascontiguousarray(x[:, :, iy][:, :, :, ix])
    assert mode == "linear"

    def axis(n_in, n_out, s):
        c = np.array([float(min(max(resize_coord(o, n_in, n_out, s, ctm), 0), n_in - 1)) for o in range(n_out)], np.float64)
        i0 = np.floor(c).astype(I64)
        return i0, np.minimum(i0 + 1, n_in - 1), c - i0

    y0, y1, fy = axis(x.shape[2], ho, sh)
    x0, x1, fx = axis(x.shape[3], wo, sw)
    v = x.astype(np.float64)
    fy, fx = fy.reshape(1, 1, -1, 1), fx.reshape(1, 1, 1, -1)
    top = v[:, :, y0][:, :, :, x0] * (1 - fx) + v[:, :, y0][:, :, :, x1] * fx
    bot = v[:, :, y1][:, :, :, x0] * (1 - fx) + v[:, :, y1][:, :, :, x1] * fx
    return top * (1 - fy) + bot * fy


# ------------------------------------------------------------------------------------------------ plumbing the test graphs need around the operator under test
def slice_(x, starts, ends, axes=None, steps=None):
    x = np.asarray(x)
    axes = list(range(len(starts))) if axes is None else [int(a) for a in axes]
    steps = [1] * len(starts) if steps is None else [int(s) for s in steps]
    sl = [slice(None)] * x.ndim
    for s, e, a, st in zip(starts, ends, axes, steps):
        sl[a] = slice(int(s), int(e), st)
    return np.ascontiguousarray(x[tuple(sl)])


def conv1x1(x, w, b=None):
    """pointwise convolution in float64, rounded once (the test stems use 0 / 1 weights: exact)"""
    y = np.einsum("nchw,oc->nohw", np.asarray(x, np.float64), np.asarray(w, np.float64)[:, :, 0, 0])
    if b is not None:
        y = y + np.asarray(b, np.float64).reshape(1, -1, 1, 1)
    return y.astype(F32)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def softmax(x, axis=-1):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def canon_zero(x):
    """-0.0 -> +0.0: for results whose zero sign the operator leaves open (Max / Min of zeros of both signs)"""
    x = np.asarray(x)
    return np.where(x == 0, np.zeros_like(x), x)


TOLERANT = {"Pow", "Sigmoid", "Softmax"}       # float64 references (plus linear Resize): compared under the suite's tolerance
ZERO_SIGN_OPEN = {"Max", "Min", "ReduceMax", "ReduceMin"}


def apply(op, x, a=None):
    """x: input values (None for an absent optional input); a: attributes.  Returns the node's value."""
    a = a or {}
    two = {"Add": add, "Sub": sub, "Mul": mul, "Div": div, "Pow": pow_, "Max": max_, "Min": min_, "Equal": equal, "Less": less, "Greater": greater, "And": and_, "Or": or_}
    one = {"Floor": floor, "Ceil": ceil, "Round": round_, "Abs": abs_, "Neg": neg, "Sqrt": sqrt, "Not": not_, "Sigmoid": sigmoid, "Identity": np.asarray}
    opt = lambda i: x[i] if len(x) > i and x[i] is not None else None
    if op in two:
        return two[op](x[0], x[1])
    if op in one:
        return one[op](x[0])
    if op == "Relu":
        return np.where(np.asarray(x[0]) > 0, x[0], np.zeros_like(x[0]))
    if op == "Conv":
        assert np.asarray(x[1]).shape[2:] == (1, 1)
        return conv1x1(x[0], x[1], opt(2))
    if op == "Softmax":
        return softmax(x[0], a.get("axis", -1))
    if op == "Clip":
        return clip(x[0], opt(1), opt(2))
    if op == "Where":
        return where(x[0], x[1], x[2])
    if op == "Cast":
        return cast(x[0], a["to"])
    if op in ("ReduceSum", "ReduceProd", "ReduceMax", "ReduceMin"):
        axes = a.get("axes") if a.get("axes") is not None else opt(1)
        return reduce(op[6:].lower(), x[0], axes, a.get("keepdims", 1))
    if op in ("ArgMax", "ArgMin"):
        return argreduce(x[0], a.get("axis", 0), a.get("keepdims", 1), a.get("select_last_index", 0), op == "ArgMin")
    if op == "Expand":
        return expand(x[0], x[1])
    if op == "Tile":
        return tile(x[0], x[1])
    if op == "Transpose":
        return transpose(x[0], a.get("perm"))
    if op == "ConstantOfShape":
        return constant_of_shape(x[0], a.get("value"))
    if op == "Range":
        return range_(x[0], x[1], x[2])
    if op == "Pad":
        v = opt(2)
        return pad(x[0], x[1], a.get("mode", "constant"), 0.0 if v is None else np.asarray(v).reshape(-1)[0], opt(3))
    if op == "Resize":
        return resize(x[0], opt(2), opt(3), a.get("mode", "nearest"), a.get("coordinate_transformation_mode", "half_pixel"), a.get("nearest_mode", "round_prefer_floor"))
    if op == "Shape":
        return np.array(np.asarray(x[0]).shape, I64)
    if op == "Gather":
        return np.take(np.asarray(x[0]), np.asarray(x[1]), axis=a.get("axis", 0))
    if op == "Slice":
        return slice_(x[0], x[1], x[2], opt(3), opt(4))
    if op == "Concat":
        return np.concatenate([np.asarray(v) for v in x], axis=a["axis"])
    if op == "Reshape":
        return np.asarray(x[0]).reshape([int(v) for v in x[1]])
    if op == "Unsqueeze":
        y = np.asarray(x[0])
        for ax in sorted(int(v) for v in x[1]):
            y = np.expand_dims(y, ax)
        return y
    raise NotImplementedError(op)
