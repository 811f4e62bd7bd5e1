"""Arena liveness of the planner: values that a multi-operator planning site leaves as a VIEW of an internal temporary ("out::sm", "out::kept",
"out::reduced", "out::gather_slice", ...) and graph-level views must keep their bytes until their last reader.

Every case is a clobber-then-late-read graph: y = the node under test; then two intermediates computed from the graph input (not from y) through the
same kind of node, so every block freed at y's node is handed out again; then a late reader of y.  A result booked under a name compute_last_use()
does not know is overwritten by then, and the engine's plan-time check (Planner::check_release) refuses the plan.

Each graph runs on two input shapes through one engine and then on the first shape again (identical bytes), against the torch oracle and the
float64 numpy oracle.  The second group holds every rewrite pass to stepping aside when its would-be-fused intermediate is read elsewhere."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth.onnx_writer import GraphBuilder
from oracle import onnx_np, onnx_ref

pytestmark = pytest.mark.gpu
TOL = 2e-4
MAP_SHAPES = ((2, 8, 12, 20), (3, 8, 12, 40))     # (N, 8, H, W), second shape as op_fuzz's OP_FUZZ_RESHAPE rule
SEQ_SHAPES = ((2, 9, 24), (3, 18, 24))            # (N, T, C)


def _close(got, ref, what):
    assert len(got) == len(ref), what
    for (name, g), r in zip(got, ref):
        r = np.asarray(r)
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        d = float(np.abs(g.astype(np.float64) - r).max()) if g.size else 0.0
        scale = max(1.0, float(np.abs(r).max())) if r.size else 1.0
        assert d <= TOL * scale, (what, name, d, scale)


def _run(model, shapes, seed=0, setenv_after_load=None):
    """A, B, A again through one engine; each against both oracles; the second run of A must repeat the first byte for byte."""
    rng = np.random.default_rng(seed)
    xa, xb = (rng.standard_normal(s).astype(np.float32) for s in shapes)
    eng = api.OrtInfer(model)
    if setenv_after_load:
        setenv_after_load()
    name = eng.input_name()
    pm = onnx_ref.parse_model(model)
    first = None
    for tag, x in (("A", xa), ("B", xb)):
        got = eng.infer(x)
        _close(got, onnx_ref.run(pm, {name: x}), f"shape {tag} vs onnx_ref")
        _close(got, onnx_np.run(pm, {name: x}), f"shape {tag} vs onnx_np")
        if first is None:
            first = got
    again = eng.infer(xa)
    for (n1, a), (_, b) in zip(first, again):
        assert np.array_equal(a, b), f"{n1}: shape A after shape B is not the bytes of its first run"
    return first


class _G:
    """GraphBuilder with seeded weights and the producers the cases share."""

    def __init__(self, kind, seed=1):
        self.g = GraphBuilder("live")
        self.rng = np.random.default_rng(seed)
        self.kind = kind
        if kind == "map":
            self.g.add_input("x", ["N", 8, "H", "W"])
        else:
            self.g.add_input("x", ["N", "T", 24])

    def w(self, *shape, scale=1.0):
        fan = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        return self.g.init((scale * self.rng.standard_normal(shape) / np.sqrt(fan)).astype(np.float32))

    def c(self, v):
        return self.g.init(np.array(v, np.float32), "c")

    def i64(self, v):
        return self.g.init(np.array(v, np.int64), "i")

    def op(self, *a, **k):
        return self.g.op(*a, **k)

    def conv(self, x, cin, cout, k=1, group=1, stride=1, bias=True):
        ins = [x, self.w(cout, cin // group, k, k)] + ([self.g.init((0.2 * self.rng.standard_normal(cout)).astype(np.float32))] if bias else [])
        return self.op("Conv", ins, kernel_shape=[k, k], strides=[stride, stride], pads=[k // 2] * 4, group=group, dilations=[1, 1])

    def clast(self, c=16):
        """a channels-last map [N, c, H, W] computed from the input"""
        return self.op("Relu", [self.conv("x", 8, c)])

    def native(self):
        """a native-layout map [N, 8, H, W] computed from the input"""
        return self.op("Mul", ["x", self.c(1.0 + self.rng.random())])   # (a scale per call: two instances must not compute the same bytes)

    def seq(self, c=24):
        """a native [N, T, c] computed from the input"""
        return self.op("Add", [self.op("MatMul", ["x", self.w(24, c)]), self.g.init((0.1 * self.rng.standard_normal(c)).astype(np.float32))])

    def model(self, outs):
        for o, r in outs:
            self.g.add_output(o, [f"d{i}" for i in range(r)])
        return self.g.model()


def _late(kind, prod, node, rank):
    """y = node(prod); two more instances of the node on fresh producers of the input (the clobber); the graph output reads y last."""
    b = _G(kind)
    y = node(b, prod(b))
    i1 = node(b, prod(b))
    i2 = node(b, prod(b))
    z = b.op("Add", [i1, i2])
    return b.model([(b.op("Sub", [y, z]), rank)])


def _sm(axis):
    return lambda b, t: b.op("Softmax", [t], axis=axis)


def _reduce(op, axes, keepdims):
    return lambda b, t: b.op(op, [t], axes=axes, keepdims=keepdims)


def _conv_bcast_residual(b, t):   # pass 4 folds the Add; its operand broadcasts -> "::pre" then a separate Add
    return b.op("Add", [b.conv(t, 16, 16), b.op("GlobalAveragePool", [t])])


def _conv_se_refused(b, t):       # SE gate on a 12-channel map: the gated bf16x6 kernel needs C % 8 == 0 -> "::se" Mul, then the conv
    p = b.op("GlobalAveragePool", [t])
    gate = b.op("HardSigmoid", [b.conv(b.op("Relu", [b.conv(p, 12, 4)]), 4, 12)], alpha=1.0 / 6.0, beta=0.5)
    return b.conv(b.op("Mul", [t, gate]), 12, 16)


def _dsblock(b, t):               # depthwise 3x3 -> pointwise 1x1 (pass 7: one DSBlock node)
    return b.conv(b.op("Relu", [b.conv(t, 16, 16, k=3, group=16)]), 16, 24)


def _rank5_softmax_ax1(b, t):
    return b.op("Softmax", [b.op("Reshape", [t, b.i64([0, 0, 0, 2, -1])])], axis=1)


def _gather(axis, index):
    return lambda b, t: b.op("Gather", [t, b.g.init(np.array(index, np.int64), "i")], axis=axis)


def _view(which):
    def f(b, t):
        if which == "to_last":          # channels-last map -> its NHWC view
            return b.op("Transpose", [t], perm=[0, 2, 3, 1])
        if which == "from_last":        # native map [N, C, H, W] -> [N, W, C, H], a channels-last view of the same bytes
            return b.op("Transpose", [t], perm=[0, 3, 1, 2])
        if which == "reshape_clast":    # [N, C, H, W] -> [N, C, H*W] of a channels-last map
            return b.op("Reshape", [t, b.i64([0, 0, -1])])
        if which == "reshape_native":
            return b.op("Reshape", [t, b.i64([0, -1])])
        if which == "squeeze":          # [N, C, 1, W] after a full-height pool
            return b.op("Squeeze", [b.op("MaxPool", [t], kernel_shape=[12, 1], strides=[12, 1]), b.i64([2])])
        if which == "slice":            # first sample: a contiguous view
            return b.op("Slice", [t, b.i64([0]), b.i64([1]), b.i64([0])])
        raise ValueError(which)
    return f


def _split_first(b, t):             # [N, T, 24] -> [24, N, T], split along the leading axis: each part is a view of the transposed copy
    return b.op("Split", [b.op("Transpose", [t], perm=[2, 0, 1]), b.i64([8, 16])], n_out=2, axis=0)[1]


_M, _S = "map", "seq"
LATE_CASES = {
    # Softmax over an inner axis: Transpose -> last-axis softmax into "::sm" -> Transpose back
    "softmax_ax1_rank3": (_S, lambda b: b.seq(), _sm(1), 3),                         # from_last view of "::sm"
    "softmax_ax1_rank4_clast": (_M, lambda b: b.clast(), _sm(1), 4),
    "softmax_ax1_rank4_native": (_M, lambda b: b.native(), _sm(1), 4),
    "softmax_ax1_rank5": (_M, lambda b: b.clast(), _rank5_softmax_ax1, 5),
    "softmax_ax2_rank4_copy": (_M, lambda b: b.clast(), _sm(2), 4),                   # controls: the transpose back is a copy
    "softmax_ax0_rank3_copy": (_S, lambda b: b.seq(), _sm(0), 3),
    # Reduce*: "::kept" -> Squeeze, the pooling route, "::moved" / "::reduced" -> Reshape view
    "reducemean_hw_kd0": (_M, lambda b: b.clast(), _reduce("ReduceMean", [2, 3], 0), 2),
    "reducemean_h_kd0": (_M, lambda b: b.clast(), _reduce("ReduceMean", [2], 0), 3),    # pooling route: a window as tall as the map, "::kept" -> Squeeze
    "reducemean_h_kd1": (_M, lambda b: b.clast(), _reduce("ReduceMean", [2], 1), 4),
    "reducemax_h_kd0": (_M, lambda b: b.clast(), _reduce("ReduceMax", [2], 0), 3),
    "reducemax_h_kd1": (_M, lambda b: b.clast(), _reduce("ReduceMax", [2], 1), 4),
    "reducemax_w_kd0": (_M, lambda b: b.clast(), _reduce("ReduceMax", [3], 0), 3),     # (W is a trailing axis: the plain reduction, as a control)
    "reducesum_c_kd0": (_M, lambda b: b.clast(), _reduce("ReduceSum", [1], 0), 3),
    "reducesum_c_kd1": (_M, lambda b: b.clast(), _reduce("ReduceSum", [1], 1), 4),
    "reducemin_nt_kd1": (_S, lambda b: b.seq(), _reduce("ReduceMin", [0, 1], 1), 3),
    "reducemean_t_kd0": (_S, lambda b: b.seq(), _reduce("ReduceMean", [1], 0), 2),
    # Gather with one index on a device tensor
    "gather_view": (_S, lambda b: b.seq(), _gather(0, 1), 2),                           # batch row: a view of the source
    "gather_copy": (_S, lambda b: b.seq(), _gather(1, 4), 2),                           # a token of every sample: "::gather_slice" copy
    # convolution fallbacks
    "conv_residual_broadcast": (_M, lambda b: b.clast(), _conv_bcast_residual, 4),
    "conv_se_gate_refused": (_M, lambda b: b.clast(12), _conv_se_refused, 4),
    # graph-level views: the source's last direct reader is the view node, the view is read after the clobber
    "view_transpose_to_last": (_M, lambda b: b.clast(), _view("to_last"), 4),
    "view_transpose_from_last": (_M, lambda b: b.native(), _view("from_last"), 4),
    "view_reshape_clast": (_M, lambda b: b.clast(), _view("reshape_clast"), 3),
    "view_reshape_native": (_S, lambda b: b.seq(), _view("reshape_native"), 2),
    "view_squeeze": (_M, lambda b: b.clast(), _view("squeeze"), 3),
    "view_slice": (_S, lambda b: b.seq(), _view("slice"), 3),
    "view_split": (_S, lambda b: b.seq(), _split_first, 3),
}


@pytest.mark.parametrize("case", sorted(LATE_CASES))
def test_decomposed_node_result_survives_until_its_late_reader(case):
    kind, prod, node, rank = LATE_CASES[case]
    _run(_late(kind, prod, node, rank), MAP_SHAPES if kind == _M else SEQ_SHAPES)


def test_dsblock_two_conv_fallback_keeps_its_result(monkeypatch):
    """The DSBlock node (rewrite pass 7) planned as its two convolutions ("::dw"): the fused kernel is refused at plan time."""
    model = _late(_M, lambda b: b.clast(), _dsblock, 4)
    _run(model, MAP_SHAPES)
    _run(model, MAP_SHAPES, setenv_after_load=lambda: monkeypatch.setenv("OAR_FUSE_DSBLOCK", "0"))


# ------------------------------------------------------------------ fusion must step aside
# pattern(b) -> (m, y, rank_m, rank_y): y is what the rewrite pass would produce, m the intermediate it would swallow.
def _p_bn(b):
    t = b.clast()
    m = b.conv(t, 16, 16, k=3)
    r = b.rng
    y = b.op("BatchNormalization", [m] + [b.g.init(v.astype(np.float32)) for v in (1 + 0.1 * r.standard_normal(16), 0.1 * r.standard_normal(16), 0.1 * r.standard_normal(16), 1 + 0.2 * r.random(16))], epsilon=1e-5)
    return m, y, 4, 4


def _p_linear(b):
    m = b.op("MatMul", ["x", b.w(24, 32)])
    return m, b.op("Add", [m, b.g.init((0.1 * b.rng.standard_normal(32)).astype(np.float32))]), 3, 3


def _p_gelu(b):
    s = b.seq()
    m = b.op("Erf", [b.op("Div", [s, b.c(np.sqrt(2.0))])])
    return m, b.op("Mul", [b.op("Mul", [s, b.op("Add", [m, b.c(1.0)])]), b.c(0.5)]), 3, 3


def _p_act(b):
    m = b.conv(b.clast(), 16, 16, k=3)
    return m, b.op("Relu", [m]), 4, 4


def _p_hswish(b):
    m = b.conv(b.clast(), 16, 16)
    hs = b.op("HardSigmoid", [m], alpha=1.0 / 6.0, beta=0.5)
    return hs, b.op("Mul", [m, hs]), 4, 4


def _p_swish(b):
    m = b.conv(b.clast(), 16, 16)
    return m, b.op("Mul", [m, b.op("Sigmoid", [m])]), 4, 4


def _p_residual(b):
    t = b.clast()
    m = b.conv(t, 16, 16, k=3)
    return m, b.op("Add", [m, t]), 4, 4


def _p_attention(b, heads=2):
    s = b.seq()
    hd = 24 // heads
    qkv = b.op("Transpose", [b.op("Reshape", [b.op("MatMul", [s, b.w(24, 72)]), b.i64([0, -1, 3, heads, hd])])], perm=[2, 0, 3, 1, 4])
    q, k, v = b.op("Split", [qkv], n_out=3, axis=0)
    ax0 = b.i64([0])
    q, k, v = b.op("Squeeze", [q, ax0]), b.op("Squeeze", [k, ax0]), b.op("Squeeze", [v, ax0])
    q = b.op("Mul", [q, b.c(hd ** -0.5)])
    m = b.op("Softmax", [b.op("MatMul", [q, b.op("Transpose", [k], perm=[0, 1, 3, 2])])], axis=-1)
    o = b.op("Reshape", [b.op("Transpose", [b.op("MatMul", [m, v])], perm=[0, 2, 1, 3]), b.i64([0, -1, 24])])
    return m, o, 4, 3


def _se_gate(b, p, c):
    return b.op("HardSigmoid", [b.conv(b.op("Relu", [b.conv(p, c, 8)]), 8, c)], alpha=1.0 / 6.0, beta=0.5)


def _p_se_gate(b):
    m = b.op("GlobalAveragePool", [b.clast(16)])
    return m, _se_gate(b, m, 16), 4, 4


def _p_dsblock(b):
    m = b.op("Relu", [b.conv(b.clast(), 16, 16, k=3, group=16)])
    return m, b.conv(m, 16, 24), 4, 4


def _p_se_scale(b):
    t = b.clast(16)
    m = b.op("Mul", [t, _se_gate(b, b.op("GlobalAveragePool", [t]), 16)])
    return m, b.conv(m, 16, 24), 4, 4


def _p_se_pool(b):
    t = b.op("Relu", [b.conv(b.clast(16), 16, 16, k=3, group=16)])
    m = b.op("GlobalAveragePool", [t])
    return m, b.op("Mul", [t, _se_gate(b, m, 16)]), 4, 4


FUSION = {   # pass -> (input kind, pattern, OAR_FUSE_* switch or None)
    "p1_bn_fold": (_M, _p_bn, None),
    "p2_linear_bias": (_S, _p_linear, None),
    "p2b_gelu": (_S, _p_gelu, "OAR_FUSE_GELU"),
    "p3_activation": (_M, _p_act, None),
    "p3_hardswish": (_M, _p_hswish, None),
    "p3_swish": (_M, _p_swish, None),
    "p4_residual": (_M, _p_residual, None),
    "p5_attention": (_S, _p_attention, "OAR_FUSE_ATTENTION"),
    "p6_se_gate": (_M, _p_se_gate, "OAR_FUSE_SE"),
    "p7_dsblock": (_M, _p_dsblock, "OAR_FUSE_DSBLOCK"),
    "p8_se_scale": (_M, _p_se_scale, "OAR_FUSE_SE_SCALE"),
    "p9_se_pool": (_M, _p_se_pool, "OAR_FUSE_SE_POOL"),
}


def _fusion_graph(kind, pattern, where):
    """where = "late": the intermediate m also has a reader after a clobber of fresh maps; "output": m is also a graph output."""
    b = _G(kind)
    m, y, rm, ry = pattern(b)
    outs = [(y, ry)]
    fresh = (lambda: b.clast(16)) if kind == _M else (lambda: b.seq(24))
    z = b.op("Add", [b.op("Relu", [fresh()]), b.op("Relu", [fresh()])])
    outs.append((z, 4 if kind == _M else 3))
    outs.append((b.op("Mul", [m, b.c(1.5)]) if where == "late" else m, rm))
    return b.model(outs)


@pytest.mark.parametrize("where", ["late", "output"])
@pytest.mark.parametrize("rewrite", sorted(FUSION))
def test_fusion_steps_aside_for_a_second_reader(rewrite, where, monkeypatch):
    kind, pattern, switch = FUSION[rewrite]
    model = _fusion_graph(kind, pattern, where)
    shapes = MAP_SHAPES if kind == _M else SEQ_SHAPES
    fused = _run(model, shapes)
    if switch:
        monkeypatch.setenv(switch, "0")           # read per model load: a new engine plans the op-by-op path
        plain = _run(model, shapes)
        _close(fused, [a for _, a in plain], f"{rewrite}: {switch}=0")
