"""The case tables of the operator-semantics tests: every graph is built node by node through `Trace`, which writes the ONNX node AND evaluates it
with oracle/op_ref.py in the same call -- graph and expected values cannot drift.  tests/test_op_semantics_cpu.py runs the tables against
oracle/onnx_ref.py (torch) and checks the quality of the inputs; tests/test_gpu_op_semantics.py runs them through the engine.

A `Case` is one model with one or more runs (feeds -> expected outputs).  Each expected output carries its rule:
  "exact"  bits of the f32 values (int64 values for integer outputs)          "zero"  the same after -0.0 -> +0.0 (Max / Min family: see op_ref.max_)
  "tol"    |d| <= 2e-4 * max(1, |ref|.max()), the suite's rule, against a float64 reference (Pow, linear Resize, Sigmoid, Softmax)
Groups are built on first use and cached; nothing here needs a GPU."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oar_ocr_amd.synth.onnx_writer import GraphBuilder
from oracle import op_ref

F32, I64 = np.float32, np.int64
INF = np.float32(np.inf)
VALUES = np.array([-2, -1, -0.0, 0.0, 0.5, 1, 2, 3, np.inf, -np.inf], F32)                      # comparisons, logic, select
_VALUE_P = np.array([.07, .07, .2, .2, .07, .07, .07, .07, .09, .09])                            # zeros often: And / Or / Equal see both outcomes
NONNEG = np.array([0.0, 0.5, 1, 2, 3], F32)                                                     # what passes a Conv + Relu stem unchanged (0 * inf is NaN, Relu drops the rest)
_NONNEG_P = np.array([.4, .15, .15, .15, .15])
ARITH = np.array([-2, -1, 0.5, 1, 2, 3, 0.75, -1.5, 7, -0.375], F32)                             # Sub / Div carriers: finite, non-zero
ROUNDING = np.array([k + 0.5 for k in range(-4, 5)] + [0.0, -0.0, 0.49999997, -0.49999997, 8388607.5, 8388608, -8388608, 1e30, -1e30, np.inf, -np.inf], F32)
NS = (1, 3, 4, 5, 1023, 1025)                                                                    # float4 body and scalar tail of the flat kernels
TOL = 2e-4

SCALE_PAIRS = ((5, 10), (7, 21), (8, 4), (12, 3), (6, 9), (16, 40), (1, 4))                      # Resize given `scales` (all exact in f32)
SIZE_PAIRS = ((9, 6), (10, 4), (5, 13), (3, 7), (11, 5), (4, 1))                                 # Resize given `sizes`


@dataclass
class Case:
    name: str
    model: bytes
    runs: list                                   # [(feeds [(name, array)], expect {output: (reference, rule)})]
    onnx_ref: bool = True                        # oracle/onnx_ref.py can run this graph
    notes: dict = field(default_factory=dict)


@dataclass
class ErrorCase:
    name: str
    model: bytes
    feeds: list
    code: str                                    # name of the api.OAR_* constant
    needle: str                                  # must occur in the message


class Trace:
    def __init__(self, name, opset=17):
        self.g = GraphBuilder(name, opset)
        self.val, self.feeds, self.expect, self.tolerant, self._last_op = {}, [], {}, set(), {}

    def input(self, name, arr, dims=None):
        arr = np.ascontiguousarray(arr, F32)
        self.g.add_input(name, list(arr.shape) if dims is None else dims)
        self.val[name] = arr
        self.feeds.append((name, arr))
        return name

    def const(self, arr, prefix="c"):
        arr = np.asarray(arr)
        name = self.g.init(arr, prefix)
        self.val[name] = arr
        return name

    def i64(self, *v):
        return self.const(np.array(v, I64), "i")

    def op(self, op, ins, **attrs):
        name = self.g.op(op, ins, **attrs)
        self.val[name] = op_ref.apply(op, [self.val[i] if i else None for i in ins], attrs)
        if op in op_ref.TOLERANT and self.val[name].dtype.kind == "f" or (op == "Resize" and attrs.get("mode") == "linear") or any(i in self.tolerant for i in ins if i):
            self.tolerant.add(name)
        self._last_op[name] = op
        return name

    def stem(self, x, relu=True):
        """a channels-last producer (graph inputs are NCHW): 1x1 convolution with the identity matrix, then Relu -- exact"""
        c = self.val[x].shape[1]
        y = self.op("Conv", [x, self.const(np.eye(c, dtype=F32).reshape(c, c, 1, 1), "w")], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
        return self.op("Relu", [y]) if relu else y

    def out(self, name, rule=None):
        v = self.val[name]
        if v.dtype == np.bool_:                  # bool results leave through Cast(to = float)
            src = name
            name = self.op("Cast", [name], to=1)
            self._last_op[name] = self._last_op.get(src, "")
            v = self.val[name]
        if rule is None:
            rule = "tol" if name in self.tolerant else "zero" if self._last_op.get(name) in op_ref.ZERO_SIGN_OPEN else "exact"
        if rule != "tol" and v.dtype.kind == "f":
            assert v.dtype == F32, (name, v.dtype)
        assert not np.isnan(np.asarray(v, np.float64)).any(), ("NaN in a reference", name)
        self.g.add_output(name, list(v.shape), elem_type=7 if v.dtype.kind == "i" else 1)
        self.expect[name] = (v, rule)
        assert len(self.expect) <= 16
        return name


def single(name, t, **kw):
    return Case(name, t.g.model(), [(t.feeds, t.expect)], **kw)


def multi(name, build, arg_list, **kw):
    """one model, several feeds: `build(arg)` must write the same graph every time (symbolic dims for what varies)"""
    ts = [build(a) for a in arg_list]
    return Case(name, ts[0].g.model(), [(t.feeds, t.expect) for t in ts], **kw)


def uni(values):
    return np.full(len(values), 1.0 / len(values))


def draw(rng, shape, values=VALUES, p=None):
    return rng.choice(values, size=shape, p=_VALUE_P if values is VALUES and p is None else p).astype(F32)


def both_outcomes(expect, notes, lo=0.10):
    """the input-quality rule of the comparison / logic outputs (exact 0 / 1 tensors of at least 10 elements): each outcome on at least 10 % of the elements"""
    for name, (ref, rule) in expect.items():
        if name in notes.get("one_sided", []) or ref.dtype != F32 or ref.size < 10 or rule != "exact" or not np.isin(ref, (0.0, 1.0)).all():
            continue
        if not lo <= float(ref.mean()) <= 1 - lo:
            return False
    return True


# ================================================================================================ a. binary kernels
def _binary_block(t, rng, A, B, notes):
    """the 16 outputs of one operand-shape pair.  A(name, values) / B(name, values) make the first / second operand's tensor from drawn values:
    a graph input, an initializer, a stem output, a Slice view ... -- the caller decides; each returns (tensor name, its value)."""
    p, q = A("p", VALUES), B("q", VALUES)
    u, v = A("u", ARITH), B("v", ARITH)
    pb, pe = A("pb", "base"), B("pe", np.array([2, 0.5, -1, 3, 0], F32))
    qb, qe = B("qb", "base"), A("qe", np.array([2, 0.5, -1, 3, 0], F32))
    nb, ne = A("nb", "negbase"), B("ne", np.array([2, 3], F32))
    for op in ("Max", "Min", "Equal", "And", "Or"):
        o = t.out(t.op(op, [p, q]))
        if op in ("And", "Or") and min(t.val[p].size, t.val[q].size) == 1:
            notes.setdefault("one_sided", []).append(o)      # a single-element operand decides And or Or alone
    for op, a, b in (("Less", p, q), ("Greater", p, q), ("Sub", u, v), ("Div", u, v)):
        t.out(t.op(op, [a, b]))
        t.out(t.op(op, [b, a]))
    o1, o2, o3 = t.out(t.op("Pow", [pb, pe])), t.out(t.op("Pow", [qb, qe])), t.out(t.op("Pow", [nb, ne]))
    shape = t.val[o1].shape
    notes.setdefault("pow_one", []).append((o1, np.broadcast_to(t.val[pe] == 0, shape).copy()))
    notes["pow_one"].append((o2, np.broadcast_to(t.val[qe] == 0, shape).copy()))


def _maker(t, rng, shape, how="input", positive_only=False):
    """how: "input" graph input | "const" initializer | "stem" channels-last producer | "neg" a computed native tensor (Neg of an input holding -values)"""
    def make(name, values):
        if isinstance(values, str):
            x = rng.uniform(0.25, 4.0, shape).astype(F32)
            if values == "negbase" and how != "stem":
                x = -x
        elif how == "stem":
            vs = NONNEG if values is VALUES else values[(values > 0) | ((values == 0) & ~np.signbit(values))]
            vs = vs[np.isfinite(vs)]
            x = draw(rng, shape, vs, _NONNEG_P if vs is NONNEG else uni(vs))
        else:
            x = draw(rng, shape, values, None if values is VALUES else uni(values))
            if values is VALUES and x.size == 1:
                x = np.full(shape, 1, F32)         # a lone operand in the middle of the other side's values: the comparisons still see both outcomes
        nm = f"{name}_{len(t.feeds)}"
        if how == "const":
            return t.const(x, name)
        if how == "stem":
            return t.stem(t.input(nm, x))
        if how == "neg":
            return t.op("Neg", [t.input(nm, -x)])
        return t.input(nm, x)
    return make


@functools.lru_cache(None)
def binary_cases():
    cases = []
    for n in NS:                                                             # same shape: binary_flat_kernel
        rng, t, notes = np.random.default_rng(100 + n), Trace(f"flat{n}"), {}
        mk = _maker(t, rng, (n,))
        _binary_block(t, rng, mk, mk, notes)
        cases.append(single(f"flat n={n}", t, notes=notes))
    partners = [("[1,C,1,1]", lambda N, C, H, W: (1, C, 1, 1), "input"), ("[C,1,1]", lambda N, C, H, W: (C, 1, 1), "const"), ("[N,C,1,1]", lambda N, C, H, W: (N, C, 1, 1), "input"),
                ("[N,1,H,W]", lambda N, C, H, W: (N, 1, H, W), "const"), ("[1,1,1,W]", lambda N, C, H, W: (1, 1, 1, W), "input"), ("scalar", lambda N, C, H, W: (), "const"),
                ("computed full size", lambda N, C, H, W: (N, C, H, W), "neg")]
    H, W = 5, 7
    for C in (8, 6):                                                         # channels-last producer: binary_chan_kernel (C % 4 == 0) / binary_kernel
        for N in (1, 3):
            for k, (pn, shape, how) in enumerate(partners):
                for attempt in range(50):     # a partner of a few elements can leave a comparison one-sided: the first seed whose inputs pass the quality rule
                    rng, t, notes = np.random.default_rng(1000 * C + 10 * N + k + 100000 * attempt), Trace(f"clast{C}_{N}_{k}"), {}
                    _binary_block(t, rng, _maker(t, rng, (N, C, H, W), "stem"), _maker(t, rng, shape(N, C, H, W), how), notes)
                    if both_outcomes(t.expect, notes):
                        break
                cases.append(single(f"channels-last C={C} N={N} with {pn}", t, notes=notes))
    for sa, sb in (((2, 3, 1, 5, 1, 7), (1, 3, 4, 1, 6, 1)), ((2, 3, 1, 5, 7), (1, 3, 4, 1, 7)), ((3, 1), (1, 3))):   # generic broadcast, ranks 6 / 5 / 2
        rng, t, notes = np.random.default_rng(len(sa) * 77), Trace(f"rank{len(sa)}"), {}
        _binary_block(t, rng, _maker(t, rng, sa), _maker(t, rng, sb), notes)
        cases.append(single(f"rank {len(sa)} broadcast", t, notes=notes))
    for k in (1, 2, 3):                                                      # a view that starts k elements into its buffer: the vector path off its alignment
        rng, t, notes = np.random.default_rng(50 + k), Trace(f"view{k}"), {}
        base = _maker(t, rng, (1027 + k,))

        def view(name, values, k=k, base=base, t=t):
            return t.op("Slice", [base(name, values), t.i64(k), t.i64(k + 1027), t.i64(0)])
        _binary_block(t, rng, view, _maker(t, rng, (1027,)), notes)
        cases.append(single(f"Slice view from element {k}", t, notes=notes))
    return cases


@functools.lru_cache(None)
def grid_stride_cases():
    """more elements than the capped grid (8192 blocks x 256 threads) covers in one pass; Less, so every element is checked exactly"""
    out = []
    for name, na, nb in (("generic kernel, 2^21 + 3 elements against a broadcast one", 2 ** 21 + 3, 1), ("flat kernel, 2^23 + 5 elements", 2 ** 23 + 5, 2 ** 23 + 5)):
        rng, t = np.random.default_rng(na), Trace("gridstride")
        a = t.input("a", rng.integers(-3, 4, na).astype(F32))
        b = t.input("b", rng.integers(-3, 4, nb).astype(F32) if nb > 1 else np.array([0.5], F32))
        t.out(t.op("Less", [a, b]))
        out.append(single(name, t))
    return out


# ================================================================================================ b. unary
@functools.lru_cache(None)
def unary_cases():
    cases = []
    for n in NS:
        t = Trace(f"unary{n}")
        x = t.input("x", np.roll(np.resize(ROUNDING, max(n, len(ROUNDING))), n)[:n])
        for op in ("Floor", "Ceil", "Round", "Not", "Abs", "Neg"):
            t.out(t.op(op, [x]))
        z = t.input("z", draw(np.random.default_rng(n), (n,)))                # Not on the logic values too
        notes = {"logic": [t.out(t.op("Not", [z]))]}
        lo, hi = t.const(np.array(-1.25, F32)), t.const(np.array(2.5, F32))
        t.out(t.op("Clip", [x, lo]))
        t.out(t.op("Clip", [x, "", hi]))
        t.out(t.op("Clip", [x, lo, hi]))
        cases.append(single(f"unary n={n}", t, notes=notes))
    t = Trace("castbool")                                                    # f32 -> bool -> f32 is x != 0, not x
    x = t.input("x", np.array([0.5, -2, 0, -0.0, 3, 1e-38], F32))
    b = t.op("Cast", [x], to=9)
    f = t.op("Cast", [b], to=1)
    assert np.array_equal(t.val[f], np.array([1, 1, 0, 0, 1, 1], F32))
    t.out(f)
    t.out(t.op("Equal", [f, t.const(np.array(1, F32))]))
    t.out(t.op("Mul", [f, t.const(np.array([2, 3, 4, 5, 6, 7], F32))]))
    t.out(t.op("ReduceSum", [f, t.i64(0)], keepdims=0))
    s = t.op("ReduceSum", [t.op("Cast", [t.op("Greater", [x, t.const(np.array(0, F32))])], to=1), t.i64(0)], keepdims=1)   # a count: a float that is no mask
    t.out(t.op("Cast", [t.op("Cast", [s], to=9)], to=1))
    cases.append(single("Cast to bool and back", t))
    return cases


# ================================================================================================ c. Where
@functools.lru_cache(None)
def where_cases():
    cases = []
    N, H, W = 3, 4, 5
    rng, t = np.random.default_rng(7), Trace("where3")
    a, b = t.input("a", draw(rng, (1, H, 1))), t.const(np.array(-0.0, F32))
    p, q = t.input("p", draw(rng, (N, 1, W))), t.input("q", draw(rng, (N, 1, W)))
    mask = rng.integers(0, 2, (N, 1, W))
    for cond in (t.op("Greater", [p, q]), t.const(mask.astype(F32)), t.const(mask.astype(np.bool_))):
        t.out(t.op("Where", [cond, a, b]))
        t.out(t.op("Where", [cond, b, a]))
    cases.append(single("three-way broadcast [N,1,W] / [1,H,1] / scalar", t))
    rng, t = np.random.default_rng(8), Trace("where44")                      # operands of one size and crossed shapes: taking one's strides for the other transposes it
    a, b = t.input("a", np.arange(1, 5, dtype=F32).reshape(4, 1)), t.input("b", -np.arange(1, 5, dtype=F32).reshape(1, 4))
    t.out(t.op("Where", [t.const((np.add.outer(np.arange(4), np.arange(4)) % 2).astype(F32)), a, b]))
    t.out(t.op("Where", [t.op("Greater", [a, t.const(np.array(2.5, F32))]), b, a]))
    cases.append(single("[4,1] against [1,4]", t))
    for C in (8, 6):
        rng, t = np.random.default_rng(70 + C), Trace(f"where_clast{C}")
        shape = (2, C, 3, 5)
        a, b = t.stem(t.input("a", draw(rng, shape, NONNEG, uni(NONNEG)))), t.stem(t.input("b", draw(rng, shape, NONNEG, uni(NONNEG))))
        cond = t.op("Less", [t.input("p", draw(rng, shape)), t.input("q", draw(rng, (1, C, 1, 1)))])
        t.out(t.op("Where", [cond, a, b]))
        t.out(t.op("Where", [t.op("Greater", [a, b]), b, t.input("r", draw(rng, (2, 1, 3, 5)))]))
        cases.append(single(f"operands from channels-last producers, C={C}", t))
    rng, t = np.random.default_rng(76), Trace("where6")
    c = t.op("Less", [t.input("p", draw(rng, (2, 1, 3, 1, 2, 1))), t.input("q", draw(rng, (1, 3, 1, 1, 2, 5)))])
    t.out(t.op("Where", [c, t.input("a", draw(rng, (2, 3, 1, 4, 1, 5))), t.input("b", draw(rng, (1, 1, 3, 4, 2, 1)))]))
    cases.append(single("rank 6", t))
    return cases


# ================================================================================================ d. reductions over the last axis
RED_C = (1, 2, 63, 64, 65, 129, 1000)
RED_ROWS = (1, 3, 4, 5, 70)                                                  # four rows per block: the ragged last block


def reduce_inputs(rows, C):
    rng = np.random.default_rng(31 * C + rows)
    ints = rng.integers(-9, 10, (rows, C)).astype(F32)
    prod = rng.choice(np.array([1, -1], F32), (rows, C))
    for r in range(rows):                                                    # at most 20 entries of 2 or 0.5 per row
        k = min(20, C)
        idx = rng.choice(C, size=rng.integers(0, k + 1), replace=False)
        prod[r, idx] *= rng.choice(np.array([2, 0.5], F32), len(idx))
    return ints, prod, draw(rng, (rows, C))


def arg_inputs(rows, C):
    """kind -> [rows, C]; "ties": even rows all equal, odd rows four-valued with the largest and the smallest value at least 3 times each (C permitting)"""
    rng = np.random.default_rng(17 * C + rows)
    distinct = (rng.permutation(rows * C).astype(F32).reshape(rows, C) - F32(rows * C // 2)) * F32(0.5)
    ties = rng.choice(np.array([-1, 0, 1, 2], F32), (rows, C))
    for r in range(rows):
        if r % 2 == 0:
            ties[r] = ties[r, 0]
        elif C >= 6:
            pos = rng.permutation(C)[:6]
            ties[r, pos[:3]], ties[r, pos[3:]] = 2, -1
    zeros = rng.choice(np.array([0.0, -0.0], F32), (rows, C))
    infs = rng.choice(np.array([np.inf, -np.inf, 1.0, -1.0], F32), (rows, C))
    return {"distinct": distinct, "ties": ties, "zeros": zeros, "infs": infs}


@functools.lru_cache(None)
def reduce_cases():
    cases = []
    for C in RED_C:
        def build(rows, C=C):
            t = Trace(f"reduce{C}")
            ints, prod, gen = reduce_inputs(rows, C)
            xs, xp, xg = t.input("xs", ints, ["R", C]), t.input("xp", prod, ["R", C]), t.input("xg", gen, ["R", C])
            for kd in (0, 1):
                t.out(t.op("ReduceSum", [xs, t.i64(-1)], keepdims=kd))
                t.out(t.op("ReduceProd", [xp], axes=[1], keepdims=kd))
                t.out(t.op("ReduceMax", [xg], axes=[-1], keepdims=kd))
                t.out(t.op("ReduceMin", [xg], axes=[1], keepdims=kd))
            return t
        cases.append(multi(f"reduce C={C}", build, RED_ROWS))
    rng, t = np.random.default_rng(5), Trace("reduce_axes")                  # non-trailing axes: the Transpose route
    xp = t.input("xp", rng.choice(np.array([1, -1, 2, 0.5], F32), (3, 10, 7, 12), p=[.4, .4, .1, .1]))
    xg = t.input("xg", draw(rng, (3, 10, 7, 12)))
    for axes in ([1], [1, 3], [2]):
        for kd in (0, 1):
            t.out(t.op("ReduceProd", [xp], axes=axes, keepdims=kd))
            t.out(t.op("ReduceMin", [xg], axes=axes, keepdims=kd))
    cases.append(single("ReduceProd / ReduceMin over non-trailing axes", t))
    return cases


@functools.lru_cache(None)
def argreduce_cases():
    cases = []
    for C in RED_C:
        def build(arg, C=C):
            rows, kind = arg
            t = Trace(f"arg{C}")
            x = t.input("x", arg_inputs(rows, C)[kind], ["R", C])
            for op in ("ArgMax", "ArgMin"):
                for last in (0, 1):
                    for kd in (0, 1):
                        t.out(t.op(op, [x], axis=-1, keepdims=kd, select_last_index=last))
            return t
        cases.append(multi(f"arg-reduce C={C}", build, [(rows, kind) for rows in RED_ROWS for kind in ("distinct", "ties", "zeros", "infs")]))
    return cases


# ================================================================================================ e. broadcast copies and generators
@functools.lru_cache(None)
def copy_cases():
    cases = []
    rng, t = np.random.default_rng(11), Trace("expand")
    t.out(t.op("Expand", [t.input("a", draw(rng, (3, 1, 5))), t.i64(2, 3, 4, 5)]))
    t.out(t.op("Expand", [t.input("b", draw(rng, (1,))), t.i64(7)]))
    t.out(t.op("Expand", [t.input("c", draw(rng, (3, 4, 5))), t.i64(3, 1, 5)]))            # a target holding 1 where the input has n
    t.out(t.op("Expand", [t.stem(t.input("d", draw(rng, (1, 8, 3, 5), NONNEG, uni(NONNEG)))), t.i64(3, 8, 3, 5)]))
    t.out(t.op("Tile", [t.input("e", draw(rng, (2, 3, 4, 5))), t.i64(1, 2, 1, 3)]))
    t.out(t.op("Tile", [t.input("f", draw(rng, (3, 5))), t.i64(2, 3)]))
    cases.append(single("Expand / Tile", t))
    rng, t = np.random.default_rng(12), Trace("cos")
    for shape in ((5, 13), (4, 16)):                                                         # 65 elements: a device constant; 64: a host value
        x = t.input(f"x{shape[0]}", draw(rng, shape, ARITH, uni(ARITH)))
        t.out(t.op("Add", [x, t.op("ConstantOfShape", [t.i64(*shape)], value=np.array([1.5], F32))]))
        t.out(t.op("Mul", [t.op("ConstantOfShape", [t.op("Shape", [x])], value=np.array([-2.0], F32)), x]))
    cases.append(single("ConstantOfShape on both sides of 64 elements", t))
    t = Trace("range")
    x = t.input("x", np.zeros((2, 9), F32))
    w = t.op("Gather", [t.op("Shape", [x]), t.const(np.array(1, I64))], axis=0)
    t.out(t.op("Range", [t.const(np.array(0, I64)), w, t.const(np.array(1, I64))]))
    t.out(t.op("Range", [t.const(np.array(0.0, F32)), t.const(np.array(2.0, F32)), t.const(np.array(0.25, F32))]))
    t.out(t.op("Range", [t.const(np.array(5, I64)), t.const(np.array(-4, I64)), t.const(np.array(-2, I64))]))
    t.out(t.op("Range", [t.const(np.array(1.5, F32)), t.const(np.array(-1.0, F32)), t.const(np.array(-0.75, F32))]))
    t.out(t.op("Range", [w, w, t.const(np.array(1, I64))]))                                   # empty
    t.out(t.op("Add", [x, t.op("Cast", [t.op("Range", [t.const(np.array(0, I64)), w, t.const(np.array(1, I64))])], to=1)]))
    cases.append(single("Range", t))
    return cases


# ================================================================================================ f. Resize
MODE_PAIRS = tuple((c, n) for c in op_ref.CTMS for n in op_ref.NEAREST_MODES)


def _pairings(pairs):
    """every pair once on H and once on W, next to a different one"""
    return [(pairs[i], pairs[(i + 2) % len(pairs)]) for i in range(len(pairs))]


def _resize_args(t, x, hp, wp, by_scale):
    """roi, scales / sizes inputs of a Resize of x"""
    if by_scale:
        return ["", t.const(np.array([1, 1, hp[1] / hp[0], wp[1] / wp[0]], F32), "s")]
    return ["", "", t.i64(t.val[x].shape[0], t.val[x].shape[1], hp[1], wp[1])]


def _ramp(shape, start=1):
    return ((np.arange(int(np.prod(shape))) + start) * 0.5).astype(F32).reshape(shape)      # every element different, positive, bf16x3-exact


@functools.lru_cache(None)
def resize_nearest_cases():
    cases = []
    jobs = [(h, w, True) for h, w in _pairings(SCALE_PAIRS)] + [(h, w, False) for h, w in _pairings(SIZE_PAIRS)]
    for mi, (ctm, nm) in enumerate(MODE_PAIRS):
        for C in (8, 3):
            t = Trace(f"resize_{mi}_{C}")
            at = dict(mode="nearest", coordinate_transformation_mode=ctm, nearest_mode=nm)
            for j, (hp, wp, by_scale) in enumerate(jobs):
                x = t.input(f"x{j}", _ramp((2 if j % 2 else 1, C, hp[0], wp[0]), j))
                sizes = lambda: _resize_args(t, x, hp, wp, by_scale)
                route = (j + mi) % 6
                if route == 0:                                               # straight from the graph input
                    t.out(t.op("Resize", [x] + sizes(), **at))
                elif route == 1:                                             # deferred, its one consumer cannot absorb it: run first
                    t.out(t.op("Neg", [t.op("Resize", [t.stem(x)] + sizes(), **at)]))
                elif route == 2:                                             # deferred into a channel Concat
                    s = t.stem(x)
                    t.out(t.op("Concat", [t.op("Resize", [s] + sizes(), **at), t.op("Resize", [t.op("Neg", [s])] + sizes(), **at)], axis=1))
                elif route == 3:                                             # two consumers: materialised
                    r = t.op("Resize", [t.stem(x)] + sizes(), **at)
                    t.out(r)
                    t.out(t.op("Abs", [r]))
                elif route == 4:                                             # deferred into an Add (read through the index map when it is o / f)
                    r = t.op("Resize", [t.stem(x)] + sizes(), **at)
                    other = t.stem(t.input(f"y{j}", _ramp(t.val[r].shape, 3 * j)))
                    t.out(t.op("Add", [other, r] if j % 4 else [r, other]))
                else:                                                        # deferred in front of a convolution
                    t.out(t.stem(t.op("Resize", [t.stem(x)] + sizes(), **at), relu=False))
            cases.append(single(f"nearest {ctm} / {nm}, C={C}", t, onnx_ref=True))
    return cases


@functools.lru_cache(None)
def resize_linear_cases():
    t = Trace("resize_linear")
    rng = np.random.default_rng(9)
    for ctm in op_ref.CTMS:
        at = dict(mode="linear", coordinate_transformation_mode=ctm)
        a = t.input(f"a_{ctm}", rng.standard_normal((2, 3, 1, 1)).astype(F32))                                     # in == 1
        t.out(t.op("Resize", [a, "", t.const(np.array([1, 1, 4, 4], F32))], **at))
        b = t.input(f"b_{ctm}", rng.standard_normal((1, 8, 4, 4)).astype(F32))                                     # out == 1
        t.out(t.op("Resize", [b, "", "", t.i64(1, 8, 1, 1)], **at))
    for ctm in ("align_corners", "pytorch_half_pixel"):
        at = dict(mode="linear", coordinate_transformation_mode=ctm)
        c = t.input(f"c_{ctm}", rng.standard_normal((1, 3, 5, 8)).astype(F32))
        t.out(t.op("Resize", [c, "", "", t.i64(1, 3, 13, 4)], **at))                                               # 5 -> 13 and 8 -> 4 by sizes
        d = t.input(f"d_{ctm}", rng.standard_normal((1, 8, 8, 6)).astype(F32))
        t.out(t.op("Resize", [d, "", t.const(np.array([1, 1, 0.5, 1.5], F32))], **at))                             # 8 -> 4 and 6 -> 9 by scales
    return [single("linear Resize at the edges of the coordinate modes", t)]


# ================================================================================================ g. Pad
@functools.lru_cache(None)
def pad_cases():
    cases = []
    specs = [
        ("rank 2", (6, 7), False, [
            ("constant", [-1, -2, -1, 0], None, None), ("reflect", [-2, -1, 0, -2], None, None), ("edge", [0, -3, -2, -1], None, None),
            ("constant", [2, -2, -1, 3], None, 1.5), ("edge", [-1, 2, 3, -2], None, None), ("reflect", [-1, 2, 2, -1], None, None),
            ("constant", [1, -2], [1], -7.0), ("reflect", [3, 2], [-2], None)]),
        ("rank 4", (2, 3, 5, 6), False, [
            ("constant", [0, -1, -1, -2, 0, 0, -2, 1], None, 0.25), ("reflect", [0, 0, -1, 2, 0, 0, 3, -1], None, None), ("edge", [1, -1, 2, -2, -1, 1, -1, 3], None, None),
            ("reflect", [2, -1, 1, -2], [3, 2], None), ("constant", [-1, 1], [0], None)]),
        ("rank 4 channels-last", (2, 8, 5, 6), True, [
            ("constant", [0, -2, -1, 2, 0, -1, 2, -1], None, 3.0), ("reflect", [0, 0, -1, 2, 0, 0, 3, -1], None, None), ("edge", [0, 1, 2, -2, 0, -3, -1, 3], None, None),
            ("reflect", [1, -2], [-1], None)]),
        ("rank 5", (2, 3, 4, 5, 6), False, [
            ("constant", [0, -1, 1, -1, 2, 1, 0, -1, 2, -2], None, -1.0), ("reflect", [0, 1, -1, 2, -2, 1, -1, 2, -1, 3], None, None), ("edge", [-1, 0, 2, -2, 1, 0, 1, -1, 0, -3], None, None)]),
        ("rank 6", (2, 3, 1, 4, 5, 3), False, [
            ("constant", [0, -1, 0, 1, -1, 1, 1, 0, 0, -2, 2, -1], None, 9.0), ("reflect", [0, -1, 2, -1, 2, 0, 0, 1, 3, 2, -2, 1], None, None),
            ("edge", [-1, 1, 1, -2, 0, 2, 1, -1, 0, 3, -1, -1], None, None)]),
        ("a length-1 axis under reflect", (1, 4), False, [("reflect", [2, 0, 3, 0], None, None), ("reflect", [1, 2, 2, -1], None, None)]),
    ]
    for name, shape, clast, pads in specs:
        rng, t = np.random.default_rng(len(shape) * 13 + clast), Trace("pad")
        x = t.input("x", draw(rng, shape, NONNEG, uni(NONNEG)) if clast else draw(rng, shape))
        if clast:
            x = t.stem(x)
        for mode, p, axes, value in pads:
            ins = [x, t.i64(*p)]
            if value is not None or axes is not None:
                ins.append(t.const(np.array(value, F32)) if value is not None else "")
            if axes is not None:
                ins.append(t.i64(*axes))
            t.out(t.op("Pad", ins, mode=mode))
        cases.append(single(f"Pad {name}", t))
    return cases


# ================================================================================================ h. Transpose
@functools.lru_cache(None)
def transpose_cases():
    rng, t = np.random.default_rng(21), Trace("transpose")
    x6, x5 = t.input("x6", draw(rng, (2, 3, 4, 5, 6, 7))), t.input("x5", draw(rng, (2, 3, 4, 5, 6)))
    m6, m5 = t.input("m6", draw(rng, (2, 3, 1, 5, 6, 7))), t.input("m5", draw(rng, (2, 3, 1, 5, 6)))
    for x, m, r in ((x6, m6, 6), (x5, m5, 5)):
        ident = list(range(r))
        t.out(t.op("Transpose", [x], perm=ident[::-1]))                      # full reversal
        t.out(t.op("Transpose", [x], perm=ident[2:] + ident[:2]))            # a rotation
        t.out(t.op("Transpose", [x], perm=ident[:-2] + [r - 1, r - 2]))      # the two innermost axes
        t.out(t.op("Transpose", [m], perm=[1, r - 1, 2, 0] + ident[3:-1]))   # a size-1 axis in the middle
    return [single("Transpose ranks 5 and 6", t)]


# ================================================================================================ i. host path and device path
HOST_DIMS = (3, 7, 2, 5)


def _twin_nodes(t, a, b, c, kind):
    """the node list both paths run: a, b, c are rank-1 operands of four elements (a: the dims, b: mixed signs, c: halves when float).
    kind: "int" | "float".  Returns the output tensors."""
    outs = []
    for op in ("Add", "Sub", "Mul", "Div", "Max", "Min"):
        outs += [t.op(op, [a, b]), t.op(op, [b, a])] if op in ("Sub", "Div") else [t.op(op, [a, b])]
    lt, gt, eq = t.op("Less", [a, c]), t.op("Greater", [a, c]), t.op("Equal", [a, c])
    outs += [lt, gt, eq, t.op("And", [lt, t.op("Greater", [b, c])]), t.op("Or", [eq, t.op("Less", [b, c])]), t.op("Not", [lt])]
    outs += [t.op("Neg", [b]), t.op("Abs", [b])]
    outs += [t.op("Where", [lt, a, b]), t.op("Where", [gt, b, c])]
    a31, b13 = t.op("Reshape", [t.op("Slice", [a, t.i64(0), t.i64(3), t.i64(0)]), t.i64(3, 1)]), t.op("Reshape", [t.op("Slice", [b, t.i64(1), t.i64(4), t.i64(0)]), t.i64(1, 3)])
    zero = t.const(np.array(0, I64 if kind == "int" else F32))
    outs.append(t.op("Where", [t.op("Greater", [a31, t.const(np.array(2, I64 if kind == "int" else F32))]), b13, zero]))     # [3,1] x [1,3] x scalar -> [3,3]
    for op in ("ReduceSum", "ReduceMax", "ReduceMin"):
        outs.append(t.op(op, [b, t.i64(0)] if op == "ReduceSum" else [b], keepdims=0, **({} if op == "ReduceSum" else {"axes": [0]})))
    if kind == "int":
        outs.append(t.op("ReduceProd", [b], axes=[0], keepdims=1))
        outs.append(t.op("Pow", [a, t.const(np.array([2, 0, 3, 1], I64))]))
        outs += [t.op("Cast", [b], to=1), t.op("Cast", [b], to=9)]
    else:
        outs.append(t.op("Pow", [a, c]))
        outs += [t.op(op, [c]) for op in ("Floor", "Ceil", "Round")] + [t.op("Sqrt", [a])]
        outs.append(t.op("ReduceProd", [t.op("Div", [a, a])], axes=[0], keepdims=1))
        outs.append(t.op("Cast", [c], to=9))
    return outs


def _twin_sources(t, where, kind):
    """a = HOST_DIMS, b = [-7, 2, -2(.5), 9], c = [3, -7, 4, 5] / [2.5, -7.5, 0.5, -0.5]; on the host path all three hang off Shape, so op_host evaluates every node"""
    bi, ci = np.array([-7, 2, -2, 9], I64), np.array([3, -7, 4, 5], I64)
    bf, cf = np.array([-7, 2, -2.5, 9], F32), np.array([2.5, -7.5, 0.5, -0.5], F32)
    x = t.input("x", np.zeros(HOST_DIMS, F32))
    dims = np.array(HOST_DIMS)
    if where == "host":
        a = t.op("Shape", [x])
        if kind == "int":
            return a, t.op("Sub", [a, t.const((dims - bi).astype(I64))]), t.op("Sub", [a, t.const((dims - ci).astype(I64))])
        a = t.op("Cast", [a], to=1)
        return a, t.op("Sub", [a, t.const((dims - bf).astype(F32))]), t.op("Sub", [a, t.const((dims - cf).astype(F32))])
    return t.input("a", np.array(HOST_DIMS, F32)), t.input("b", bf), t.input("c", cf)


@functools.lru_cache(None)
def twin_cases():
    cases = []
    for where, kind in (("host", "int"), ("host", "float"), ("device", "float")):
        probe = Trace("probe")
        n_out = len(_twin_nodes(probe, *_twin_sources(probe, where, kind), kind))
        for lo in range(0, n_out, 14):
            t = Trace(f"twin_{where}_{kind}_{lo}")
            a, b, c = _twin_sources(t, where, kind)
            outs = _twin_nodes(t, a, b, c, kind)
            for o in outs[lo:lo + 14]:
                t.out(o)
            if where == "host" and kind == "float" and lo == 0:
                t.out(t.op("Cast", [t.op("Mul", [a, c])], to=7))             # float -> int64 truncates toward zero (-52.5 -> -52)
            cases.append(single(f"{where} path, {kind} operands, outputs {lo}..", t))
    return cases


@functools.lru_cache(None)
def crossing_cases():
    """plan-time values that reach operators which exist only as kernels: each gives the reference value"""
    t = Trace("crossing")
    x = t.input("x", np.zeros(HOST_DIMS, F32))
    s = t.op("Shape", [x])
    m = t.op("Reshape", [t.op("Mul", [s, t.const(np.array([1, -1, 2, 1], I64))]), t.i64(2, 2)])      # [[3, -7], [4, 5]] on the host
    t.out(t.op("ReduceSum", [m, t.i64(1)], keepdims=0))
    t.out(t.op("ReduceSum", [m, t.i64(0)], keepdims=1))
    t.out(t.op("ArgMax", [m], axis=1, keepdims=0))
    t.out(t.op("ArgMin", [m], axis=-1, keepdims=1, select_last_index=1))
    f = t.op("Mul", [t.op("Cast", [s], to=1), t.const(np.array([0.5, -0.25, 1.5, 0.125], F32))])     # a host float vector
    t.out(t.op("Sigmoid", [f]))
    t.out(t.op("Softmax", [f], axis=0))
    t.out(t.op("Expand", [m, t.i64(3, 2, 2)]))
    t.out(t.op("Tile", [m, t.i64(2, 3)]))
    t.out(t.op("Transpose", [m], perm=[1, 0]))
    t.out(t.op("Floor", [t.op("Reshape", [f, t.i64(2, 2)])]))
    return [single("host values into device-only operators", t)]


# ================================================================================================ refusals
def error_cases():
    out = []
    for op in ("ArgMax", "ArgMin"):
        g = GraphBuilder("arg_axis", 17)
        g.add_input("x", [3, 4, 5])
        g.add_output(g.op(op, ["x"], axis=1, keepdims=0), [3, 5], elem_type=7)
        out.append(ErrorCase(f"{op} over a non-last axis", g.model(), [("x", np.zeros((3, 4, 5), F32))], "OAR_UNSUPPORTED_OP", "last axis"))
    g = GraphBuilder("tile8", 17)
    g.add_input("x", [2, 3, 4, 5])
    g.add_output(g.op("Tile", ["x", g.init(np.array([2, 2, 3, 2], I64), "r")]), [4, 6, 12, 10])
    out.append(ErrorCase("Tile with four repeats > 1 (8 effective dims)", g.model(), [("x", np.zeros((2, 3, 4, 5), F32))], "OAR_UNSUPPORTED_OP", "6 effective dimensions"))
    g = GraphBuilder("reflect_wide", 17)
    g.add_input("x", [1, 5])
    g.add_output(g.op("Pad", ["x", g.init(np.array([0, -3, 0, 2], I64), "p")], mode="reflect"), [1, 4])
    out.append(ErrorCase("reflect Pad wider than what a crop leaves", g.model(), [("x", np.zeros((1, 5), F32))], "OAR_UNSUPPORTED_OP", "reflect"))
    return out


GROUPS = {"binary": binary_cases, "unary": unary_cases, "where": where_cases, "reduce": reduce_cases, "argreduce": argreduce_cases, "copy": copy_cases,
          "resize_nearest": resize_nearest_cases, "resize_linear": resize_linear_cases, "pad": pad_cases, "transpose": transpose_cases, "twin": twin_cases,
          "crossing": crossing_cases}


def compare(got, ref, rule):
    """None when `got` satisfies `rule` against `ref`, else a short description"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return f"shape {got.shape} != {ref.shape}"
    if ref.dtype.kind == "i":
        if got.dtype.kind != "i":
            return f"dtype {got.dtype}, expected int64"
        return None if np.array_equal(got, ref) else f"{int((got != ref).sum())} of {ref.size} integers differ"
    if got.dtype.kind != "f":
        return f"dtype {got.dtype}, expected float"
    if rule == "tol":
        if not ref.size:
            return None
        d, scale = float(np.abs(got.astype(np.float64) - ref).max()), max(1.0, float(np.abs(ref).max()))
        return None if d <= TOL * scale else f"|d| = {d:.3g} > {TOL} * {scale:.3g}"
    g, r = np.ascontiguousarray(got, F32), np.ascontiguousarray(ref, F32)
    if rule == "zero":
        g, r = op_ref.canon_zero(g), op_ref.canon_zero(r)
    bad = g.view(np.uint32) != r.view(np.uint32)
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad.reshape(-1))[0])
    return f"{int(bad.sum())} of {r.size} elements differ in their bits, first at {i}: {g.reshape(-1)[i]!r} != {r.reshape(-1)[i]!r}"
