"""Device-side selection in the engine (csrc/index_ops.hip): TopK, Gather with tensor indices, GatherND and GatherElements as single-operator
graphs through Seam A, compared EXACTLY with numpy -- indices with the stable-argsort tie rule (equal values: lowest index first, largest = 1 and 0
alike), values and gathered elements bit for bit."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth.onnx_writer import GraphBuilder, node

pytestmark = pytest.mark.gpu

I64 = 7


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- TopK
def _topk_graph(C, K, largest):
    g = GraphBuilder("topk", 17)
    g.add_input("x", ["R", C])
    g.nodes.append(node("TopK", ["x", g.init(np.array([K], np.int64), "k")], ["v", "i"], axis=-1, largest=largest, sorted=1))
    g.add_output("v", ["R", K])
    g.add_output("i", ["R", K], elem_type=I64)
    return g.model()


def _topk_ref(x, K, largest):
    """ONNX Runtime's rule: sorted, equal values lowest index first (+0.0 == -0.0, +-inf ordinary values)"""
    idx = np.argsort(-x if largest else x, axis=-1, kind="stable")[:, :K]
    return np.take_along_axis(x, idx, -1), idx.astype(np.int64)


def _topk_inputs(rng, rows, C):
    distinct = rng.permutation(rows * C).astype(np.float32).reshape(rows, C) * np.float32(0.37) - np.float32(0.31 * rows * C / 2)     # no two equal
    ties = rng.choice(np.array([-1, 0, 1, 2], np.float32), (rows, C))
    mixed = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1.5, 1.5, -2.0, 3.0, 1e-38, -1e-38], np.float32), (rows, C))
    return {"distinct": distinct, "ties": ties, "mixed": mixed}


@pytest.mark.parametrize("largest", [1, 0])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 8400, 16384])
def test_topk_matches_stable_argsort(C, largest):
    rng = np.random.default_rng(1000 * C + largest)
    data = {rows: _topk_inputs(rng, rows, C) for rows in (1, 3, 70)}
    for K in sorted({1, min(C, 300), C}):
        eng = api.OrtInfer(_topk_graph(C, K, largest))
        for rows, inputs in data.items():
            for kind, x in inputs.items():
                out = dict(eng.infer(x))
                rv, ri = _topk_ref(x, K, largest)
                assert out["i"].dtype == np.int64 and out["i"].shape == (rows, K) and out["v"].shape == (rows, K)
                assert np.array_equal(out["i"], ri), (C, K, largest, rows, kind)
                assert np.array_equal(_bits(out["v"]), _bits(rv)), (C, K, largest, rows, kind)
        eng.close()


def test_topk_values_of_a_leading_batch_axis():
    """rank 3: the rows are every leading index"""
    rng = np.random.default_rng(3)
    g = GraphBuilder("topk3", 17)
    g.add_input("x", ["N", 5, 37])
    g.nodes.append(node("TopK", ["x", g.init(np.array([9], np.int64), "k")], ["v", "i"], axis=2, largest=1, sorted=1))
    g.add_output("v", ["N", 5, 9])
    g.add_output("i", ["N", 5, 9], elem_type=I64)
    x = rng.integers(-4, 5, (2, 5, 37)).astype(np.float32)
    out = dict(api.OrtInfer(g.model()).infer(x))
    rv, ri = _topk_ref(x.reshape(10, 37), 9, 1)
    assert np.array_equal(out["i"], ri.reshape(2, 5, 9)) and np.array_equal(_bits(out["v"]), _bits(rv.reshape(2, 5, 9)))


def test_topk_limits_are_plan_time_errors():
    x = np.zeros((1, 16385), np.float32)
    with pytest.raises(api.OCRError) as e:
        api.OrtInfer(_topk_graph(16385, 300, 1)).infer(x)
    assert e.value.code == api.OAR_UNSUPPORTED_OP and "16384" in e.value.message
    for C, K in ((64, 65), (64, 0)):
        with pytest.raises(api.OCRError) as e:
            api.OrtInfer(_topk_graph(C, K, 1)).infer(np.zeros((2, C), np.float32))
        assert e.value.code == api.OAR_SHAPE_MISMATCH, (C, K)
    g = GraphBuilder("topk_axis", 17)
    g.add_input("x", ["R", 8, 8])
    g.nodes.append(node("TopK", ["x", g.init(np.array([2], np.int64), "k")], ["v", "i"], axis=1))
    g.add_output("v", ["R", 2, 8])
    g.add_output("i", ["R", 2, 8], elem_type=I64)
    with pytest.raises(api.OCRError) as e:
        api.OrtInfer(g.model()).infer(np.zeros((1, 8, 8), np.float32))
    assert e.value.code == api.OAR_UNSUPPORTED_OP


# ---------------------------------------------------------------------------------------------- gathers
class _G:
    """x (the data, primary input) plus index operands that are either host constants or produced on the device:
    ArgMax over a one-hot input of 2 * D columns, minus D -- any wanted index in [-D, D), duplicates included."""

    def __init__(self, name, x):
        self.g = GraphBuilder(name, 17)
        self.g.add_input("x", list(x.shape))
        self.feeds = [("x", x)]

    def index(self, want, D, device, last_axis_tuples=False):
        want = np.asarray(want, np.int64)
        assert want.min() >= -D and want.max() < D
        g = self.g
        if not device:
            return g.init(want, "idx")
        nm = f"sel{len(self.feeds)}"
        onehot = np.zeros(want.shape + (2 * D,), np.float32)
        np.put_along_axis(onehot, (want + D)[..., None], 1.0, -1)
        g.add_input(nm, list(onehot.shape))
        self.feeds.append((nm, onehot))
        am = g.op("ArgMax", [nm], axis=-1, keepdims=0)
        return g.op("Sub", [am, g.init(np.array(D, np.int64), "d")])

    def run(self, y, shape):
        self.g.add_output(y, list(shape))
        return dict(api.OrtInfer(self.g.model()).infer(self.feeds))[y]


def _data(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    flat[:: 7] = np.float32(-0.0)
    flat[3:: 11] = np.float32(np.inf)
    return x


GATHER_SHAPES = [(2, 7, 5), (2, 7, 3), (2, 7, 4), (3, 336, 64)]   # inner runs 35 / 5 / 1, 3, 4 and 64 (16-byte path) / 21504


@pytest.mark.parametrize("device", [True, False], ids=["device-indices", "host-indices"])
@pytest.mark.parametrize("shape", GATHER_SHAPES)
def test_gather_tensor_indices(shape, device):
    rng = np.random.default_rng(sum(shape))
    x = _data(rng, shape)
    for axis in range(len(shape)):
        D = shape[axis]
        for ishape in ((5,), (3, 2)):
            want = rng.integers(-D, D, ishape)
            want.reshape(-1)[:2] = [-1, -1]                                  # a duplicate and a negative for sure
            b = _G("gather", x)
            y = b.g.op("Gather", ["x", b.index(want, D, device)], axis=axis - len(shape) if axis == 1 else axis)
            ref = np.take(x, np.where(want < 0, want + D, want), axis=axis)
            got = b.run(y, ref.shape)
            assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), (shape, axis, ishape, device)


@pytest.mark.parametrize("device", [True, False], ids=["device-indices", "host-indices"])
@pytest.mark.parametrize("shape", [(2, 7, 5), (3, 336, 64)])
def test_gather_elements(shape, device):
    rng = np.random.default_rng(sum(shape) + 1)
    x = _data(rng, shape)
    for axis in range(len(shape)):
        D = shape[axis]
        ishape = list(shape)
        ishape[axis] = 4                                                     # its own length along the axis
        if axis != 0:
            ishape[0] = shape[0] - 1                                         # and smaller than the data elsewhere
        want = rng.integers(-D, D, ishape)
        want.reshape(-1)[:2] = [D - 1, D - 1]
        b = _G("gather_elements", x)
        y = b.g.op("GatherElements", ["x", b.index(want, D, device)], axis=axis)
        sub = x[tuple(slice(0, (shape[d] if d == axis else ishape[d])) for d in range(len(shape)))]
        ref = np.take_along_axis(sub, np.where(want < 0, want + D, want), axis=axis)
        got = b.run(y, ref.shape)
        assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), (shape, axis, device)


@pytest.mark.parametrize("device", [True, False], ids=["device-indices", "host-indices"])
@pytest.mark.parametrize("shape", [(2, 7, 5), (3, 336, 64)])
@pytest.mark.parametrize("batch_dims,m", [(0, 1), (0, 2), (1, 1), (1, 2), (0, 3)])
def test_gather_nd(shape, batch_dims, m, device):
    rng = np.random.default_rng(sum(shape) + 10 * batch_dims + m)
    x = _data(rng, shape)
    lead = (shape[0], 6) if batch_dims else (4, 3)                           # indices [..., m]
    cols = []
    for q in range(m):
        D = shape[batch_dims + q]
        c = rng.integers(-D, D, lead)
        c.reshape(-1)[:2] = [-1, -1]
        cols.append(c)
    b = _G("gather_nd", x)
    if device:   # one ArgMax per tuple position, unsqueezed and concatenated: the index tensor is assembled on the device
        parts = [b.g.op("Unsqueeze", [b.index(c, shape[batch_dims + q], True), b.g.init(np.array([-1], np.int64), "axes")]) for q, c in enumerate(cols)]
        idx = parts[0] if m == 1 else b.g.op("Concat", parts, axis=-1)
    else:
        idx = b.g.init(np.stack(cols, -1).astype(np.int64), "idx")
    y = b.g.op("GatherND", ["x", idx], batch_dims=batch_dims)
    pos = [np.where(c < 0, c + shape[batch_dims + q], c) for q, c in enumerate(cols)]
    ref = x[(np.arange(shape[0])[:, None],) + tuple(pos)] if batch_dims else x[tuple(pos)]
    got = b.run(y, ref.shape)
    assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), (shape, batch_dims, m, device)


def test_index_tensor_survives_views_and_leaves_as_i64():
    """TopK indices through Unsqueeze / Expand / Reshape / Tile / Concat / Cast stay an index tensor: they leave as I64 and still gather"""
    rng = np.random.default_rng(8)
    x = rng.permutation(3 * 40).astype(np.float32).reshape(3, 40)
    g = GraphBuilder("views", 17)
    g.add_input("x", [3, 40])
    v, i = g.op("TopK", ["x", g.init(np.array([6], np.int64), "k")], n_out=2, axis=-1)
    u = g.op("Unsqueeze", [i, g.init(np.array([2], np.int64), "axes")])                  # [3, 6, 1]
    e = g.op("Expand", [u, g.init(np.array([3, 6, 2], np.int64), "shape")])              # [3, 6, 2]
    r = g.op("Reshape", [e, g.init(np.array([3, 12], np.int64), "shape")])               # [3, 12]
    t = g.op("Tile", [r, g.init(np.array([1, 2], np.int64), "reps")])                    # [3, 24]
    c = g.op("Concat", [t, i], axis=1)                                                   # [3, 30]
    k = g.op("Cast", [c], to=7)
    ge = g.op("GatherElements", ["x", k], axis=1)
    for nm, el in ((v, 1), (k, I64), (ge, 1)):
        g.add_output(nm, [3, 6 if nm == v else 30], elem_type=el)
    out = dict(api.OrtInfer(g.model()).infer(x))
    rv, ri = _topk_ref(x, 6, 1)
    rk = np.concatenate([np.tile(np.repeat(ri, 2, axis=1), (1, 2)), ri], 1)
    assert out[k].dtype == np.int64 and np.array_equal(out[k], rk)
    assert np.array_equal(_bits(out[ge]), _bits(np.take_along_axis(x, rk, 1))) and np.array_equal(_bits(out[v]), _bits(rv))


def test_cost_counts_selection_steps_with_bytes_and_no_flops():
    eng = api.OrtInfer(_topk_graph(1000, 300, 1))
    flops, nbytes, kernels = eng.cost((3, 1000))
    assert flops == 0 and kernels == 1 and nbytes >= 4 * 3 * (1000 + 2 * 300)
