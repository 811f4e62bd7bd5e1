"""GPU parity of the network forward (Seam A, the OrtInfer stand-in) against the torch-CPU ONNX oracle.
Tolerance: north_star allows 1e-3 on float scores/logits; f32 MFMA kernels are held to 2e-4 here."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models, pages, x6_cases
from oar_ocr_amd.synth.child_run import infer_in_child
from oar_ocr_amd.synth.onnx_writer import GraphBuilder
from oracle import cpu_ref as R
from oracle import onnx_ref

pytestmark = pytest.mark.gpu
TOL = 2e-4


def _check(model_bytes, x, tol=TOL):
    eng = api.OrtInfer(model_bytes)
    got = eng.infer(x)
    ref = onnx_ref.run(model_bytes, {eng.input_name(): x})
    assert len(got) == len(ref)
    for (name, g), r in zip(got, ref):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        d = np.abs(g - r).max() if g.size else 0.0
        scale = max(1.0, float(np.abs(r).max())) if r.size else 1.0
        assert d <= tol * scale, (name, d, scale)
    return got, ref


def test_detector_graph_matches_oracle():
    det, _ = models.build_det("tiny", seed=0)
    page = pages.make_page(1, (160, 224), lines=3)
    x, _ = R.det_preprocess(page)
    (name, g), = _check(det, x[None])[0]
    assert g.shape == (1, 1, 160, 224)
    assert g.min() >= 0.0 and g.max() <= 1.0          # ScoreValidator range (utils/validation.rs:51-53)


def test_engine_matches_the_torch_free_oracle_too():
    """The same two graphs against oracle/onnx_np.py (numpy / float64, no torch kernel): the engine is not only close to ONE evaluator."""
    from oracle import onnx_np
    det, _ = models.build_det("tiny", seed=0)
    x, _ = R.det_preprocess(pages.make_page(5, (96, 160), lines=2))
    got = api.OrtInfer(det).infer(x[None])[0][1]
    ref = onnx_np.run(det, {"x": x[None]})[0]
    assert got.shape == ref.shape and np.abs(got - ref).max() <= TOL
    rec, _ = models.build_rec("tiny", vocab=301, seed=1)
    xr = R.rec_preprocess([pages.make_crop(i, w, 48) for i, w in enumerate((200, 131, 96))])
    eng = api.OrtInfer(rec)
    got = eng.infer(xr)[0][1]
    ref = onnx_np.run(rec, {eng.input_name(): xr})[0]
    assert got.shape == ref.shape and np.abs(got - ref).max() <= TOL and np.array_equal(got.argmax(-1), ref.argmax(-1))


def test_detector_batch_and_shapes():
    det, _ = models.build_det("tiny", seed=0)
    rng = np.random.default_rng(0)
    for shape in [(2, 3, 96, 128), (3, 3, 64, 64), (1, 3, 32, 32)]:
        _check(det, rng.standard_normal(shape).astype(np.float32))


def test_recognizer_graph_matches_oracle():
    rec, _ = models.build_rec("tiny", vocab=6906, seed=1)
    crops = [pages.make_crop(i, w, 48) for i, w in enumerate((320, 200, 411))]
    x = R.rec_preprocess(crops)
    (name, g), = _check(rec, x)[0]
    assert g.shape == (3, x.shape[3] // 8, 6906)
    assert np.all(g >= 0.0) and np.all(g <= 1.0)
    assert np.allclose(g.sum(-1), 1.0, atol=1e-4)


def test_config1_single_crop_48x320():
    # BASELINE config 1: examples/text_recognition.rs, one 48x320 line -> [1,3,48,320] -> [1,T,V]
    rec, _ = models.build_rec("tiny", vocab=6906, seed=1)
    x = R.rec_preprocess([pages.make_crop(0, 320, 48)])
    assert x.shape == (1, 3, 48, 320)
    _check(rec, x)


# ------------------------------------------------------------------ op-level graphs (one per kernel family)
def _single_op_graph(build):
    g = GraphBuilder("op_test")
    out_name, out_shape = build(g)
    g.add_output(out_name, out_shape)
    return g.model()


@pytest.mark.parametrize("cfg", [
    dict(cin=8, cout=24, k=3, s=1, p=1, g=1), dict(cin=16, cout=16, k=3, s=2, p=1, g=16), dict(cin=32, cout=32, k=5, s=1, p=2, g=32),
    dict(cin=3, cout=16, k=3, s=2, p=1, g=1), dict(cin=16, cout=40, k=1, s=1, p=0, g=1), dict(cin=12, cout=20, k=3, s=1, p=1, g=4),
    dict(cin=64, cout=100, k=3, s=(2, 1), p=1, g=1), dict(cin=20, cout=6, k=(1, 3), s=1, p=(0, 1), g=1), dict(cin=8, cout=8, k=9, s=1, p=4, g=1),
    # k x 1 kernels (round 6: the tap decode divided by kw = 1 through a magic number that does not exist for 1 -- every tap read row 0; found by tools/op_fuzz.py)
    dict(cin=16, cout=12, k=(3, 1), s=1, p=(1, 0), g=1), dict(cin=24, cout=40, k=(7, 1), s=(2, 1), p=(3, 0), g=1), dict(cin=128, cout=128, k=(5, 1), s=1, p=(2, 0), g=1)])
def test_conv_variants(cfg):
    rng = np.random.default_rng(7)
    kh, kw = (cfg["k"], cfg["k"]) if isinstance(cfg["k"], int) else cfg["k"]
    sh, sw = (cfg["s"], cfg["s"]) if isinstance(cfg["s"], int) else cfg["s"]
    ph, pw = (cfg["p"], cfg["p"]) if isinstance(cfg["p"], int) else cfg["p"]

    def build(g):
        g.add_input("x", ["N", cfg["cin"], "H", "W"])
        w = rng.standard_normal((cfg["cout"], cfg["cin"] // cfg["g"], kh, kw)).astype(np.float32) * 0.2
        b = rng.standard_normal(cfg["cout"]).astype(np.float32)
        y = g.op("Conv", ["x", g.init(w), g.init(b)], kernel_shape=[kh, kw], strides=[sh, sw], pads=[ph, pw, ph, pw], group=cfg["g"], dilations=[1, 1])
        y = g.op("HardSwish", [y])
        return y, ["N", cfg["cout"], "H", "W"]

    _check(_single_op_graph(build), rng.standard_normal((2, cfg["cin"], 19, 23)).astype(np.float32))


def test_convtranspose_pool_resize_concat():
    rng = np.random.default_rng(8)

    def build(g):
        g.add_input("x", ["N", 8, "H", "W"])
        w = rng.standard_normal((8, 12, 2, 2)).astype(np.float32) * 0.3
        y = g.op("ConvTranspose", ["x", g.init(w), g.init(rng.standard_normal(12).astype(np.float32))], kernel_shape=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
        y = g.op("Relu", [y])
        w3 = rng.standard_normal((12, 5, 3, 3)).astype(np.float32) * 0.2
        z = g.op("ConvTranspose", [y, g.init(w3)], kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1], output_padding=[1, 1], group=1, dilations=[1, 1])
        p1 = g.op("MaxPool", [y], kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1])
        p2 = g.op("AveragePool", [y], kernel_shape=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0])
        u = g.op("Resize", [p1, "", g.init(np.array([1, 1, 2, 2], np.float32))], mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor")
        v = g.op("Resize", [p2, "", g.init(np.array([1, 1, 2, 2], np.float32))], mode="linear", coordinate_transformation_mode="half_pixel")
        c = g.op("Concat", [u, v, y], axis=1)
        gp = g.op("GlobalAveragePool", [c])
        s = g.op("Sigmoid", [gp])
        m = g.op("Mul", [c, s])
        g.add_output(z, ["N", 5, "H", "W"])
        return m, ["N", 36, "H", "W"]

    _check(_single_op_graph(build), rng.standard_normal((2, 8, 10, 14)).astype(np.float32))


def test_ceil_mode_pools_divide_by_the_window_clipped_to_the_padded_extent():
    """Round 6 (found by tools/op_fuzz.py): AveragePool with ceil_mode = 1 and count_include_pad = 1 divided the overhanging last windows by kh * kw; the
    divisor counts padding but not the overhang beyond it (ONNX since opset 19, torch).  Also the output-size rule that drops a window starting past the input."""
    rng = np.random.default_rng(18)

    def build(g):
        g.add_input("x", ["N", 8, "H", "W"])
        outs = [g.op("AveragePool", ["x"], kernel_shape=[3, 2], strides=[3, 2], pads=[0, 0, 0, 0], ceil_mode=1, count_include_pad=1),
                g.op("AveragePool", ["x"], kernel_shape=[3, 1], strides=[2, 1], pads=[1, 0, 1, 0], ceil_mode=1, count_include_pad=1),
                g.op("AveragePool", ["x"], kernel_shape=[4, 3], strides=[3, 2], pads=[2, 1, 2, 1], ceil_mode=1, count_include_pad=0),
                g.op("AveragePool", ["x"], kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1], ceil_mode=0, count_include_pad=1),
                g.op("MaxPool", ["x"], kernel_shape=[3, 4], strides=[3, 2], pads=[0, 2, 0, 2], ceil_mode=1)]
        for o in outs[:-1]:
            g.add_output(o, ["N", 8, "Ho", "Wo"])
        return outs[-1], ["N", 8, "Ho", "Wo"]

    for shape in ((1, 8, 4, 49), (3, 8, 16, 113), (2, 8, 10, 14)):
        _check(_single_op_graph(build), rng.standard_normal(shape).astype(np.float32))


def test_reduce_and_softmax_over_any_axis():
    """Round 6: Reduce* over axis sets that are not trailing (channels of a map, the token axis of a sequence, H and W without keepdims) and Softmax over an inner axis
    used to be refused; they run as Transpose -> trailing kernel -> view.  Against torch-CPU."""
    rng = np.random.default_rng(19)

    def maps(g):
        g.add_input("x", ["N", 10, "H", "W"])
        outs = [g.op("ReduceSum", ["x"], axes=[1], keepdims=0), g.op("ReduceMin", ["x"], axes=[1, 3], keepdims=1), g.op("ReduceMax", ["x"], axes=[2], keepdims=1),
                g.op("ReduceMean", ["x"], axes=[2, 3], keepdims=0), g.op("ReduceMean", ["x"], axes=[1, 2], keepdims=1), g.op("Softmax", ["x"], axis=1)]
        for o in outs[:-1]:
            g.add_output(o, ["A", "B", "C", "D"])
        return outs[-1], ["N", 10, "H", "W"]

    def seq(g):
        g.add_input("x", ["N", "T", 24])
        outs = [g.op("ReduceMax", ["x"], axes=[1], keepdims=0), g.op("ReduceMean", ["x"], axes=[0, 2], keepdims=1), g.op("Softmax", ["x"], axis=1)]
        for o in outs[:-1]:
            g.add_output(o, ["A", "B", "C"])
        return outs[-1], ["N", "T", 24]

    _check(_single_op_graph(maps), rng.standard_normal((3, 10, 7, 12)).astype(np.float32))
    _check(_single_op_graph(seq), rng.standard_normal((4, 9, 24)).astype(np.float32))


def test_sequence_ops_layernorm_attention():
    rng = np.random.default_rng(9)
    C, heads = 32, 4

    def build(g):
        g.add_input("x", ["N", C, 1, "T"])
        z = g.op("Squeeze", ["x", g.init(np.array([2], np.int64))])
        z = g.op("Transpose", [z], perm=[0, 2, 1])
        ln = g.op("LayerNormalization", [z, g.init(rng.standard_normal(C).astype(np.float32)), g.init(rng.standard_normal(C).astype(np.float32))], axis=-1, epsilon=1e-5)
        w = rng.standard_normal((C, 3 * C)).astype(np.float32) * 0.2
        qkv = g.op("Add", [g.op("MatMul", [ln, g.init(w)]), g.init(rng.standard_normal(3 * C).astype(np.float32))])
        qkv = g.op("Reshape", [qkv, g.init(np.array([0, -1, 3, heads, C // heads], np.int64))])
        qkv = g.op("Transpose", [qkv], perm=[2, 0, 3, 1, 4])
        q, k, v = g.op("Split", [qkv], n_out=3, axis=0)
        ax0 = g.init(np.array([0], np.int64))
        q, k, v = g.op("Squeeze", [q, ax0]), g.op("Squeeze", [k, ax0]), g.op("Squeeze", [v, ax0])
        att = g.op("Softmax", [g.op("MatMul", [g.op("Mul", [q, g.init(np.array(0.35, np.float32))]), g.op("Transpose", [k], perm=[0, 1, 3, 2])])], axis=-1)
        o = g.op("Reshape", [g.op("Transpose", [g.op("MatMul", [att, v])], perm=[0, 2, 1, 3]), g.init(np.array([0, -1, C], np.int64))])
        z2 = g.op("Add", [z, o])
        z3 = g.op("Transpose", [z2], perm=[0, 2, 1])
        z3 = g.op("Unsqueeze", [z3, g.init(np.array([2], np.int64))])
        wc = rng.standard_normal((16, C, 1, 1)).astype(np.float32) * 0.2
        y = g.op("Conv", [z3, g.init(wc)], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
        g.add_output(z2, ["N", "T", C])
        return y, ["N", 16, 1, "T"]

    _check(_single_op_graph(build), rng.standard_normal((3, C, 1, 21)).astype(np.float32))


def test_elementwise_math_prelu_reducemean():
    """Ops of decomposed GELU / LayerNorm exports and of UVDoc's blocks."""
    rng = np.random.default_rng(11)
    C = 12

    def build(g):
        g.add_input("x", ["N", C, "H", "W"])
        w = rng.standard_normal((C, C, 3, 3)).astype(np.float32) * 0.2
        y = g.op("Conv", ["x", g.init(w)], kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1], group=1, dilations=[1, 1])
        y = g.op("PRelu", [y, g.init((0.1 + 0.3 * rng.random((C, 1, 1))).astype(np.float32))])
        gelu = g.op("Mul", [g.op("Mul", [y, g.init(np.array(0.5, np.float32))]),
                            g.op("Add", [g.op("Erf", [g.op("Div", [y, g.init(np.array(np.sqrt(2.0), np.float32))])]), g.init(np.array(1.0, np.float32))])])
        z = g.op("Add", [g.op("Sqrt", [g.op("Abs", [gelu])]), g.op("Exp", [g.op("Neg", [g.op("Abs", [y])])])])
        z = g.op("Add", [z, g.op("Reciprocal", [g.op("Add", [g.op("Softplus", [y]), g.init(np.array(1.0, np.float32))])])])
        z = g.op("Add", [z, g.op("Log", [g.op("Add", [g.op("Abs", [y]), g.init(np.array(1.0, np.float32))])])])
        z = g.op("Add", [z, g.op("Gelu", [y], approximate="tanh")])
        m = g.op("ReduceMean", [z], axes=[2, 3], keepdims=1)                    # == GlobalAveragePool
        z = g.op("Mul", [z, g.op("Sigmoid", [m])])
        t = g.op("Transpose", [g.op("Reshape", [z, g.init(np.array([0, C, -1], np.int64))])], perm=[0, 2, 1])   # [N, HW, C]
        mu = g.op("ReduceMean", [t], axes=[-1], keepdims=1)                      # decomposed LayerNorm
        d = g.op("Sub", [t, mu])
        var = g.op("ReduceMean", [g.op("Mul", [d, d])], axes=[-1], keepdims=1)
        ln = g.op("Div", [d, g.op("Sqrt", [g.op("Add", [var, g.init(np.array(1e-5, np.float32))])])])
        g.add_output(g.op("ReduceMean", [t], axes=[2], keepdims=0), ["N", "HW"])
        return ln, ["N", "HW", C]

    _check(_single_op_graph(build), rng.standard_normal((2, C, 9, 11)).astype(np.float32))


@pytest.mark.parametrize("cfg", [("linear", "zeros", 0), ("linear", "border", 1), ("linear", "reflection", 0), ("nearest", "zeros", 0),
                                 ("linear", "reflection", 1)])
def test_grid_sample(cfg):
    """UVDoc's final un-warp: a conv predicts the sampling grid, GridSample reads the image through it."""
    mode, pad, align = cfg
    rng = np.random.default_rng(12)

    def build(g):
        g.add_input("x", ["N", 3, "H", "W"])
        w = rng.standard_normal((2, 3, 3, 3)).astype(np.float32) * 0.4
        grid = g.op("Tanh", [g.op("Conv", ["x", g.init(w)], kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1], group=1, dilations=[1, 1])])
        grid = g.op("Mul", [grid, g.init(np.array(1.3, np.float32))])                  # leaves [-1, 1]: exercises the padding modes
        grid = g.op("Transpose", [grid], perm=[0, 2, 3, 1])                             # [N, Ho, Wo, 2]
        y = g.op("GridSample", ["x", grid], mode=mode, padding_mode=pad, align_corners=align)
        return y, ["N", 3, "Ho", "Wo"]

    tol = TOL if mode == "linear" else 1.0     # nearest: a coordinate within float noise of .5 may legitimately pick the other pixel
    x = rng.standard_normal((2, 3, 20, 26)).astype(np.float32)
    got, ref = _check(_single_op_graph(build), x, tol=tol)
    if mode == "nearest":
        assert (np.abs(got[0][1] - ref[0]) > 1e-4).mean() < 0.02


@pytest.mark.parametrize("mode", ["reflect", "edge", "constant"])
def test_pad_modes(mode):
    """UVDoc's reflect-padded convolutions export as Pad + Conv; Pad runs on whichever layout its input has."""
    rng = np.random.default_rng(14)

    def build(g):
        g.add_input("x", ["N", 4, "H", "W"])
        w = rng.standard_normal((8, 4, 3, 3)).astype(np.float32) * 0.3
        a = g.op("Relu", [g.op("Conv", ["x", g.init(w)], kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1], group=1, dilations=[1, 1])])   # channels-last value
        extra = {"value": 0.75} if mode == "constant" else {}
        padded = g.op("Pad", [a, g.init(np.array([0, 0, 2, 3, 0, 0, 1, 2], np.int64), "pads")], mode=mode, **extra)
        w2 = rng.standard_normal((6, 8, 3, 3)).astype(np.float32) * 0.2
        y = g.op("Conv", [padded, g.init(w2)], kernel_shape=[3, 3], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
        flat = g.op("Pad", [g.op("Reshape", ["x", g.init(np.array([0, -1], np.int64), "shape")]), g.init(np.array([0, 2, 0, 1], np.int64), "pads2")], mode=mode)   # rank-2, native layout
        g.add_output(flat, ["N", "L"])
        return y, ["N", 6, "Ho", "Wo"]

    _check(_single_op_graph(build), rng.standard_normal((2, 4, 9, 11)).astype(np.float32))


@pytest.mark.parametrize("C,R,N", [(48, 12, 5), (192, 48, 130), (768, 192, 3), (1100, 70, 2), (20, 6, 40)])
def test_squeeze_excite_gate_is_one_kernel(C, R, N):
    """Rewrite pass 6: GlobalAveragePool -> Conv 1x1 + ReLU -> Conv 1x1 + HardSigmoid -> Mul (PP-LCNet's SE block).  The shapes walk
    se_fc's launch geometry: one workgroup per image (many images), several per image with output slices (few images, wide
    layers), slices of > 1 x 64 outputs, a hidden axis cut into parts, channel counts that are no multiple of anything."""
    rng = np.random.default_rng(13)

    def build(g):
        g.add_input("x", ["N", C, "H", "W"])
        p = g.op("GlobalAveragePool", ["x"])
        w1, b1 = rng.standard_normal((R, C, 1, 1)).astype(np.float32) * 0.3, rng.standard_normal(R).astype(np.float32) * 0.1
        w2, b2 = rng.standard_normal((C, R, 1, 1)).astype(np.float32) * 0.3, rng.standard_normal(C).astype(np.float32) * 0.1
        h = g.op("Relu", [g.op("Conv", [p, g.init(w1), g.init(b1)], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])])
        s = g.op("HardSigmoid", [g.op("Conv", [h, g.init(w2), g.init(b2)], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])], alpha=0.2, beta=0.5)
        return g.op("Mul", ["x", s]), ["N", C, "H", "W"]

    model = _single_op_graph(build)
    _check(model, rng.standard_normal((N, C, 3, 5)).astype(np.float32))
    assert api.OrtInfer(model).cost((N, C, 3, 5))[2] <= 5      # layout copy in, pool, gate, scale, layout copy out


def test_unsupported_operator_is_an_error_not_a_fallback():
    def build(g):
        g.add_input("x", ["N", 4])
        return g.op("Det", ["x"]), ["N"]
    eng = api.OrtInfer(_single_op_graph(build))
    with pytest.raises(api.OCRError) as e:
        eng.infer(np.zeros((2, 4), np.float32))
    assert e.value.code == api.OAR_UNSUPPORTED_OP


def test_config3_server_size_graphs_match_oracle():
    """BASELINE config 3 (v5-server-class det + SVTRv2-class rec, vocab 18710): the wide layers take the weight-stationary
    f32 / bf16x6 kernels at larger K and N than the tiny graphs exercise.  Small inputs keep the torch-CPU oracle fast."""
    det, dinfo = models.build_det("server", seed=2)
    page = pages.make_page(3, (256, 320), lines=4)
    x, _ = R.det_preprocess(page)
    (name, g), = _check(det, np.stack([x, x[:, ::-1].copy()]), tol=5e-4)[0]
    assert g.shape == (2, 1, 256, 320)
    rec, rinfo = models.build_rec("server", vocab=18710, seed=3)
    crops = [pages.make_crop(10 + i, w, 48) for i, w in enumerate((320, 280, 512, 96))]
    xr = R.rec_preprocess(crops)
    (name, p), = _check(rec, xr, tol=5e-4)[0]
    assert p.shape == (4, xr.shape[3] // 8, 18710)
    assert np.allclose(p.sum(-1), 1.0, atol=1e-4)


def _conv_graph(cin, cout, k, seed, relu=True, group=1, strides=(1, 1)):
    g = GraphBuilder("conv")
    rng = np.random.default_rng(seed)
    g.add_input("x", ["N", cin, "H", "W"])
    w = (rng.standard_normal((cout, cin // group, k, k)) * (1.0 / np.sqrt(cin // group * k * k))).astype(np.float32)
    y = g.op("Conv", ["x", g.init(w), g.init(rng.standard_normal(cout).astype(np.float32))], kernel_shape=[k, k], strides=list(strides),
             pads=[k // 2] * 4, group=group, dilations=[1, 1])
    if relu:
        y = g.op("Relu", [y])
    g.add_output(y, ["N", cout, "H", "W"])
    return g.model()


def _check_ran(model, x, cls):
    """_check, and the profiler class `cls` ran (the name every case id promises)"""
    _check(model, x)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_enable(True); api.prof_reset()
        eng.infer(x)
        names = {e["name"] for e in api.prof_snapshot() if e["launches"]}
    finally:
        api.prof_enable(False)
        eng.close()
    assert cls in names, (cls, sorted(names))


@pytest.mark.parametrize("case", [
    ("ws_x6 1x1 192->192", 37, 192, 192, 12, 80, 1, "conv_igemm_ws_x6"),       # bf16x6 weight-stationary kernel (K, N >= 96, many pixels)
    ("ws_x6 1x1 104->96 K tail", 80, 104, 96, 12, 80, 1, "conv_igemm_ws_x6"),   # K = 104: zero-padded tail of the last 32-deep chunk
    ("ws f32 1x1 48->96", 128, 48, 96, 12, 80, 1, "conv_igemm_ws"),            # f32 weight-stationary kernel (N >= 96, K < 96)
    ("rs3_x6 3x3 64->16 (ws3 before the row-streaming kernel)", 2, 64, 16, 240, 240, 3, "conv_rs3_x6"),   # Cin 64, Cout <= 16, M >= 100000: a bf16x6 layer since igemm_rs3_x6.hip; ws3 at this shape: tests/test_gpu_f32_conv_kernels.py "ws3 NT1 64->8 (rs3 off) relu"
    ("ws3 3x3 32->32 ragged", 3, 32, 32, 150, 231, 3, "conv_igemm_ws"),        # 3x3 same conv with DPP tap reuse (M >= 100000): two cout fragments, row length not a multiple of the tile
    ("per-tile 1x1 24->32", 2, 24, 32, 240, 240, 1, "conv_igemm"),             # per-wave-tile kernel, K not a multiple of 16
])
def test_igemm_kernels_at_bench_shapes(case):
    """Each implicit-GEMM kernel at a shape large enough to select it (see conv_igemm's rules), against torch-CPU conv2d; the profiler class the id names
    ran.  (Which variant inside a class -- ws / ws3, tile / small, NT, PF -- is asserted in tests/test_gpu_f32_conv_kernels.py, where a child process
    runs with per-variant profiler names.)"""
    name, n, cin, cout, h, w, k, cls = case
    x = np.random.default_rng(len(name)).standard_normal((n, cin, h, w)).astype(np.float32)
    _check_ran(_conv_graph(cin, cout, k, seed=n + cin), x, cls)


@pytest.mark.parametrize("case", [
    ("rs3_x6 3x3 64->16", 2, 64, 16, 240, 240, "relu"),              # the DB head's convolution (igemm_rs3_x6.hip)
    ("rs3_x6 3x3 64->16 ragged", 3, 64, 16, 150, 231, "hswish"),     # strips hang over the row, segments over the image, 3 images
    ("rs3_x6 3x3 32->8", 2, 32, 8, 240, 241, None),                  # one k-step per tap, two idle lane groups in the store
    ("rs3_x6 3x3 64->12 tall", 1, 64, 12, 700, 150, "relu"),         # long segments, Cout not a multiple of 8
    ("rs3_x6 3x3 96->16 two passes", 2, 96, 16, 240, 240, "hswish"), # round 6: slices of 64 + 32 channels, the second pass adds to y (the 0.447 M detector's neck)
    ("rs3_x6 3x3 160->8 three passes", 1, 160, 8, 400, 260, None),   # 64 + 64 + 32, bias in the first pass only
])
def test_row_streaming_3x3_x6_kernel(case, tmp_path):
    """igemm_rs3_x6.hip (3x3 same convolution, <= 16 output channels, bf16x6 from packed planes in LDS) against torch-CPU conv2d, and against the
    f32 kernel it replaced (OAR_IGEMM_RS3=0: conv_igemm_ws3_kernel).  The switch is read once per process, so the f32 kernel runs the same graph and input in
    a child process; both kernels are held to float64 within tol_S of the layer's own sample (synth/x6_cases.py); a HardSwish layer in
    front of its activation (the same weights without it), where the bound is defined."""
    name, n, cin, cout, h, w, act = case
    rng = np.random.default_rng(len(name) + cout)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * (1.0 / np.sqrt(cin * 9))).astype(np.float32)
    bias_v = rng.standard_normal(cout).astype(np.float32)

    def build(act):
        g = GraphBuilder("conv")
        g.add_input("x", ["N", cin, "H", "W"])
        y = g.op("Conv", ["x", g.init(wt), g.init(bias_v)], kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1], group=1, dilations=[1, 1])
        if act == "relu":
            y = g.op("Relu", [y])
        elif act == "hswish":
            y = g.op("HardSwish", [y])
        g.add_output(y, ["N", cout, "H", "W"])
        return g.model()

    def run_x6(model):
        eng = api.OrtInfer(model, profile=True)
        api.prof_reset()
        out = eng.infer(x)[0][1]
        assert any(e["name"] == "conv_rs3_x6" for e in api.prof_snapshot()), "the layer did not select the row-streaming kernel"
        api.prof_enable(False)
        eng.close()
        return out

    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    m = build(act)
    _check(m, x)
    y6 = run_x6(m)
    # against float64: Relu does not enlarge an error, HardSwish does (slope up to 1.5) -- those layers are compared in front of their activation
    lin = build(None) if act == "hswish" else m
    if act == "hswish":
        y6 = run_x6(lin)
    y32, names = infer_in_child(lin, x, {"OAR_IGEMM_RS3": "0"}, tmp_path)
    assert "conv_rs3_x6" not in names and names & {"conv_igemm_ws", "conv_igemm"}, sorted(names)   # the f32 kernel class ran instead
    xc = x6_cases.Case(name, "conv_rs3_x6", n, cin, cout, h, w, k=3, order="class")
    bundle = x6_cases.reference_bundle(xc, x, wt, bias_v)
    f64 = np.maximum(bundle["f64"], 0.0) if act == "relu" else bundle["f64"]
    for label, y in (("bf16x6", y6), ("f32", y32)):
        err = float((np.abs(y.astype(np.float64) - f64) / bundle["S"]).max())
        print(f"\n[x6] {name} | {label} | noise_S 2^{np.log2(bundle['noise_S']):.1f} | emu_S 2^{np.log2(bundle['emu_S']):.1f} | tol_S 2^{np.log2(bundle['tol_S']):.1f} | err_S 2^{np.log2(err):.1f}")
        assert err <= bundle["tol_S"], (label, err, bundle["tol_S"])


@pytest.mark.parametrize("case", [
    ("os_x6 3x3 64->64", 2, 64, 64, 192, 192, 3, (1, 1), 1),            # K = 576: k x k conv on the output-stationary bf16x6 kernel
    ("os_x6 1x1 512->128", 1, 512, 128, 256, 256, 1, (1, 1), 1),        # long-K 1x1: the weights do not fit the weight-stationary LDS tile
    ("os_x6 3x3 s2 32->96 ragged", 1, 32, 96, 514, 514, 3, (2, 2), 1),  # stride 2, 66049 output pixels (not a multiple of the 256-pixel tile), 6 cout fragments
    ("os_x6 3x3 40->64 K tail", 1, 40, 64, 260, 260, 3, (1, 1), 1),     # K = 360: zero-padded tail of the last 32-deep chunk, Cin not a multiple of 32
    ("os_x6 3x3 dilated 64->80", 1, 64, 80, 264, 264, 3, (1, 1), 2),    # dilation 2 (padding 2), 5 cout fragments -> tile of 8 with 3 idle
    ("os_x6 5x5 16->64", 1, 16, 64, 272, 272, 5, (1, 1), 1),            # K = 400, taps straddle the 32-deep chunks
    ("os_x6 1x1 512->512 few pixels", 1, 512, 512, 200, 192, 1, (1, 1), 1),   # M = 38400: eligible through the width of the layer
    ("os_x6 1x1 1024->1024 fewer pixels", 1, 1024, 1024, 96, 100, 1, (1, 1), 1),   # M = 9600, 38 pixel tiles x 8 cout tiles
])
def test_output_stationary_x6_kernel(case):
    """igemm_os_x6.hip (the layers whose weights do not fit LDS) against torch-CPU conv2d: image borders (zero taps), strides,
    dilation, ragged pixel / cout / K tails."""
    name, n, cin, cout, h, w, k, strides, dil = case
    g = GraphBuilder("conv")
    rng = np.random.default_rng(len(name))
    g.add_input("x", ["N", cin, "H", "W"])
    wt = (rng.standard_normal((cout, cin, k, k)) * (1.0 / np.sqrt(cin * k * k))).astype(np.float32)
    pad = dil * (k // 2)
    y = g.op("Conv", ["x", g.init(wt), g.init(rng.standard_normal(cout).astype(np.float32))], kernel_shape=[k, k], strides=list(strides),
             pads=[pad] * 4, group=1, dilations=[dil, dil])
    y = g.op("HardSwish", [y])
    g.add_output(y, ["N", cout, "H", "W"])
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    m = g.model()
    _check(m, x)
    eng = api.OrtInfer(m, profile=True)
    api.prof_reset()
    eng.infer(x)
    assert any(e["name"] == "conv_igemm_os_x6" for e in api.prof_snapshot()), "the layer did not select the output-stationary kernel"
    api.prof_enable(False)
    eng.close()


@pytest.mark.parametrize("case", [
    ("5x5 s1 H=6", 16, 192, 6, 160, 5, (1, 1)),            # recognizer shapes: the whole height in three 2-row tiles
    ("5x5 s(2,1) H=6", 16, 192, 6, 160, 5, (2, 1)),
    ("5x5 s1 ragged", 3, 128, 61, 75, 5, (1, 1)),          # partial tiles in both directions
    ("5x5 s2", 2, 64, 90, 90, 5, (2, 2)),
    ("3x3 s1 C=48", 2, 48, 120, 120, 3, (1, 1)),
    ("5x5 one row per thread", 1, 128, 20, 20, 5, (1, 1)), # too few threads for 2-row tiles (rows per thread are visible in the per-variant names only: asserted in tests/test_gpu_f32_conv_kernels.py, "dw ... TH1" / "TH2")
])
def test_depthwise_kernels_at_bench_shapes(case):
    """The register-tiled depthwise kernel (kernels.hip) at the bench's layer shapes, against torch-CPU conv2d; the conv_dw class ran (tiled or generic,
    one or two rows per thread: tests/test_gpu_f32_conv_kernels.py)."""
    name, n, c, h, w, k, strides = case
    x = np.random.default_rng(len(name)).standard_normal((n, c, h, w)).astype(np.float32)
    _check_ran(_conv_graph(c, c, k, seed=n + c, group=c, strides=strides), x, "conv_dw")


def _attention_graph(dim, heads, seed, scaled=True):
    """LayerNorm-free SVTR attention block exactly as the recognizer graphs emit it (synth/models.py)."""
    g = GraphBuilder("attn")
    rng = np.random.default_rng(seed)
    hd = dim // heads
    g.add_input("x", ["N", "T", dim])
    w = (rng.standard_normal((dim, 3 * dim)) / np.sqrt(dim)).astype(np.float32)
    qkv = g.op("MatMul", ["x", g.init(w)])
    qkv = g.op("Add", [qkv, g.init((0.1 * rng.standard_normal(3 * dim)).astype(np.float32))])
    qkv = g.op("Reshape", [qkv, g.init(np.array([0, -1, 3, heads, hd], np.int64), "shape")])
    qkv = g.op("Transpose", [qkv], perm=[2, 0, 3, 1, 4])
    q, k, v = g.op("Split", [qkv], n_out=3, axis=0)
    ax0 = g.init(np.array([0], np.int64), "axes")
    q, k, v = g.op("Squeeze", [q, ax0]), g.op("Squeeze", [k, ax0]), g.op("Squeeze", [v, ax0])
    if scaled:
        q = g.op("Mul", [q, g.init(np.array(hd ** -0.5, np.float32), "scale")])
    att = g.op("Softmax", [g.op("MatMul", [q, g.op("Transpose", [k], perm=[0, 1, 3, 2])])], axis=-1)
    o = g.op("Transpose", [g.op("MatMul", [att, v])], perm=[0, 2, 1, 3])
    o = g.op("Reshape", [o, g.init(np.array([0, -1, dim], np.int64), "shape")])
    g.add_output(o, ["N", "T", dim])
    return g.model()


@pytest.mark.parametrize("case", [
    ("tiny rec head", 64, 4, 7, 40, True),
    ("server rec head", 192, 6, 3, 100, True),
    ("odd head_dim, no scale", 45, 3, 2, 37, False),       # head_dim 15: zero-padded to 16 in LDS
    ("long line", 64, 1, 2, 300, True),                    # head_dim 64, query loop (T > 256), 150 KB of K / V
])
def test_fused_attention_matches_oracle(case):
    """Rewrite pass 5: the whole q / k / v split -> softmax(q k^T) v -> merge block runs as one kernel after the projection."""
    name, dim, heads, n, T, scaled = case
    model = _attention_graph(dim, heads, seed=len(name), scaled=scaled)
    x = np.random.default_rng(n + T).standard_normal((n, T, dim)).astype(np.float32)
    _check(model, x)
    assert api.OrtInfer(model).cost((n, T, dim))[2] <= 3       # Linear + Attention (+ output copy); 14 op by op


# ------------------------------------------------------------------------------------------------ exporter-shaped graph
@pytest.mark.parametrize("shape", [(1, 3, 32, 64), (3, 3, 32, 200), (2, 3, 32, 320)])
def test_exporter_shaped_fixture_matches_oracle(shape):
    """Seam A on a graph written the way Paddle2ONNX / torch.onnx write real exports (unfolded BN, decomposed
    HardSwish / HardSigmoid / LayerNorm / softmax, Shape-Gather-Concat reshape plumbing, dynamic Resize sizes, Where / Equal,
    ConstantOfShape / Expand / Tile / Range, ReduceSum / ReduceMax, Max / Min, Greater) -- oar_ocr_amd/synth/models.py
    build_p2o_fixture -- against the torch-CPU interpreter, for several input shapes (every shape re-evaluates the host-side
    shape arithmetic)."""
    m, _ = models.build_p2o_fixture()
    assert "!" not in api.onnx_inspect(m)
    x = np.random.default_rng(shape[3]).standard_normal(shape).astype(np.float32)
    eng = api.OrtInfer(m)
    (name, got), = eng.infer(x)
    want = onnx_ref.run(m, {"x": x})[0]
    assert name == "probs" and got.shape == want.shape == (shape[0], shape[3] // 4, 37)
    assert np.abs(got - want).max() < 2e-4 and np.abs(got.sum(-1) - 1).max() < 1e-5
    assert np.array_equal(got.argmax(-1), want.argmax(-1)) or np.abs(np.sort(want, -1)[..., -1] - np.sort(want, -1)[..., -2]).min() < 1e-5
    eng.close()


# ------------------------------------------------------------------------------------------------ Seam A: the rest of OrtInfer
def _multi_io_feeds(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return {"image": rng.standard_normal((n, 3, h, w)).astype(np.float32),
            "scale_factor": rng.uniform(0.5, 2.0, (n, 2)).astype(np.float32),
            "im_shape": np.tile(np.array([[h, w]], np.float32), (n, 1))}


@pytest.mark.parametrize("shape", [(1, 32, 48), (3, 64, 40)])
def test_named_inputs_and_i64_outputs_match_oracle(shape):
    """OrtInfer::infer with several named inputs (ort_infer_execution.rs:121-219) and TensorOutput::I64 (tensor_output.rs:16-21):
    three inputs given in a DIFFERENT order than the model declares them; outputs f32 (device), i64 from the device (ArgMax)
    and i64 from a plan-time host value (Shape)."""
    m, _ = models.build_multi_io_fixture()
    feeds = _multi_io_feeds(*shape)
    eng = api.OrtInfer(m)
    outs = eng.infer([("im_shape", feeds["im_shape"]), ("image", feeds["image"]), ("scale_factor", feeds["scale_factor"])])
    want = onnx_ref.run(m, feeds)
    assert [n for n, _ in outs] == ["boxes", "ids", "dims"]
    boxes, ids, dims = (a for _, a in outs)
    assert boxes.dtype == np.float32 and ids.dtype == np.int64 and dims.dtype == np.int64
    assert np.abs(boxes - want[0]).max() < 1e-4
    assert ids.shape == want[1].shape == (shape[0], shape[1] // 4) and np.array_equal(ids, want[1])
    assert np.array_equal(dims, np.array([shape[0], 3, shape[1], shape[2]]))
    eng.close()


def test_named_input_errors_read_like_the_reference():
    m, _ = models.build_multi_io_fixture()
    feeds = _multi_io_feeds(1, 32, 32)
    eng = api.OrtInfer(m)
    with pytest.raises(api.OCRError, match="No inputs provided"):                 # ort_infer_execution.rs:125-129
        eng.infer([])
    with pytest.raises(api.OCRError, match="3 input"):
        eng.infer([("image", feeds["image"])])
    with pytest.raises(api.OCRError, match="no input named 'bogus'"):
        eng.infer([("image", feeds["image"]), ("bogus", feeds["im_shape"]), ("scale_factor", feeds["scale_factor"])])
    with pytest.raises(api.OCRError, match="given twice"):
        eng.infer([("image", feeds["image"]), ("im_shape", feeds["im_shape"]), ("im_shape", feeds["im_shape"])])
    with pytest.raises(api.OCRError, match="several inputs"):
        eng.infer(feeds["image"])
    eng.close()


def test_declared_io_metadata():
    """input_names_from_model / primary_input_shape / output_shapes (core/inference/mod.rs:66-112): dynamic dims are -1."""
    m, _ = models.build_multi_io_fixture()
    eng = api.OrtInfer(m)
    assert eng.input_names_from_model() == ["image", "scale_factor", "im_shape"]
    assert eng.primary_input_shape() == [-1, 3, -1, -1]
    assert eng.output_shapes() == [("boxes", [-1, 2]), ("ids", [-1, -1]), ("dims", [4])]
    eng.close()
    det, _ = models.build_det()
    eng = api.OrtInfer(det)
    assert eng.input_names_from_model() == [eng.input_name()] and eng.primary_input_shape()[1] == 3
    eng.close()


def test_borrowed_first_output_view():
    """infer_first_output_f32 (ort_infer_execution.rs:234-306): the closure sees (shape, data) of output 0 without an owned
    copy; its result is returned; an f32 view of a non-f32 first output is an error; a failing closure propagates."""
    m, _ = models.build_p2o_fixture()
    x = np.random.default_rng(1).standard_normal((2, 3, 32, 96)).astype(np.float32)
    eng = api.OrtInfer(m)
    owned = eng.infer(x)[0][1]
    seen = eng.infer_first_output_f32(x, lambda shape, data: (shape, data.copy(), float(data.sum())))
    assert seen[0] == owned.shape and np.array_equal(seen[1], owned) and abs(seen[2] - owned.sum()) < 1e-3
    seen2 = eng.infer_first_output_f32([(eng.input_name(), x)], lambda shape, data: data.argmax(-1))
    assert np.array_equal(seen2, owned.argmax(-1))

    class Boom(RuntimeError):
        pass

    def bad(shape, data):
        raise Boom("closure failed")
    with pytest.raises(Boom):
        eng.infer_first_output_f32(x, bad)
    assert np.array_equal(eng.infer(x)[0][1], owned)           # the engine is still usable afterwards
    eng.close()


def test_plan_cache_is_lru_bounded(monkeypatch):
    """plans_ grew without bound (one plan per input shape).  With OAR_PLAN_CACHE=4 ten different widths leave 4
    cached plans and 6+ evictions, and a re-run of an evicted shape still gives the first run's result."""
    monkeypatch.setenv("OAR_PLAN_CACHE", "4")
    m, _ = models.build_p2o_fixture()
    eng = api.OrtInfer(m)
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal((1, 3, 32, 32 + 8 * i)).astype(np.float32) for i in range(10)]
    first = [eng.infer(x)[0][1] for x in xs]
    cached, evicted = eng.cache_stats()
    assert cached <= 4 and evicted >= 6
    again = [eng.infer(x)[0][1] for x in xs]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    eng.close()


# ------------------------------------------------------------------------------------------------ fused depthwise-separable block
DS_CASES = [  # (C, Cout, k, stride, N, H, W, act, residual)
    (16, 24, 3, (1, 1), 2, 24, 40, "hswish", False), (24, 48, 3, (1, 1), 1, 24, 33, "hswish", False), (48, 48, 3, (1, 1), 3, 12, 80, "relu", True),
    (48, 96, 3, (2, 1), 2, 24, 50, "hswish", False), (96, 192, 3, (1, 2), 2, 12, 64, "hswish", False), (192, 192, 5, (1, 1), 3, 12, 40, "hswish", False),
    (64, 128, 5, (2, 2), 2, 30, 46, "hswish", False), (128, 128, 5, (1, 1), 2, 15, 23, "hswish", True), (32, 64, 3, (2, 2), 1, 37, 61, "relu", False),
    (192, 256, 5, (2, 1), 2, 12, 40, "swish", False), (8, 16, 3, (1, 1), 1, 9, 17, "hswish", False), (72, 40, 5, (1, 1), 1, 20, 36, None, False),
    # round 3, the wave-autonomous kernel (dsblock_wa.inc: 3x3 stride 1): every instantiated fragment count, partial channel chunks, image
    # borders on all four sides, many tiles per XCD band, the generic activation path, residual
    (96, 96, 3, (1, 1), 2, 12, 160, "hswish", False), (64, 64, 3, (1, 1), 2, 30, 30, "hswish", True), (80, 80, 3, (1, 1), 1, 17, 35, "relu", False),
    (32, 128, 3, (1, 1), 1, 21, 50, "hswish", False), (96, 192, 3, (1, 1), 2, 12, 70, "hswish", False), (20, 12, 3, (1, 1), 1, 40, 19, "swish", False),
    (16, 24, 3, (1, 1), 3, 120, 136, "hswish", False), (48, 48, 3, (1, 1), 1, 3, 5, None, False),
    # round 4, the chunk-streamed kernel (dsblock_cs.inc: the wide blocks): ragged rows / columns, more items than one round of waves, run-time activations
    (192, 192, 5, (1, 1), 5, 13, 50, "hswish", False), (96, 192, 3, (1, 2), 3, 12, 161, "relu", False), (128, 128, 5, (1, 1), 2, 15, 23, "hswish", False),
    (192, 192, 5, (1, 1), 40, 12, 80, None, False), (128, 128, 3, (1, 1), 3, 13, 50, "hswish", False),
    (256, 256, 3, (1, 1), 3, 11, 37, "hswish", False), (128, 256, 3, (2, 2), 2, 25, 61, "relu", False),   # two-row tiles (16 cout fragments), stride 2 both ways
]


DS2_CASES = [  # (C1, C2, C3, N, H, W, act): two consecutive 3x3 / stride-1 blocks -> one launch (csrc/dsblock_rs2.inc)
    (24, 48, 48, 3, 24, 50, "hswish"), (24, 48, 48, 2, 24, 14, "relu"), (24, 48, 48, 1, 1, 5, "hswish"), (24, 48, 48, 2, 70, 29, None),
    (16, 24, 48, 3, 13, 33, "hswish"), (16, 24, 48, 1, 24, 160, "hswish"), (16, 24, 48, 40, 24, 43, "relu"),
]


@pytest.mark.parametrize("case", DS2_CASES, ids=[f"C{c[0]}-{c[1]}-{c[2]}-H{c[4]}W{c[5]}" for c in DS2_CASES])
def test_two_fused_dsblocks_match_oracle_and_the_two_launch_path(case, monkeypatch):
    """Block -> block with the tensor between them never written (dsblock_rs2.inc): strips of 14 columns with one recomputed halo column per side,
    intermediate rows / columns outside the image zeroed (block 2's padding), pipeline fill and drain per item, ragged last strip, one-row images,
    several row segments, run-time activations -- against the torch-CPU interpreter and against the same graph as two launches (OAR_DSBLOCK_RS2=0)."""
    C1, C2, C3, N, H, W, act = case
    net = models._Net("ds2", seed=C1 * 5 + C3 + H, decomposed_hswish=False)
    g = net.g
    g.add_input("x", ["N", C1, "H", "W"])
    t = net.ds_block("x", C1, C2, 3, 1, act=act)
    z = net.ds_block(t, C2, C3, 3, 1, act=act)
    g.nodes.append(models.node("Identity", [z], ["out"]))
    g.add_output("out", ["N", C3, "H", "W"])
    m = g.model()
    x = np.random.default_rng(2).standard_normal((N, C1, H, W)).astype(np.float32)
    api.prof_enable(True); api.prof_reset()
    got, ref = _check(m, x, tol=2e-4)
    launches = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["launches"]}
    api.prof_enable(False)
    assert launches.get("dsblock_rs") == 1 and not any("conv" in n for n in launches), launches   # the pair ran as ONE launch of the row-streaming family
    monkeypatch.setenv("OAR_DSBLOCK_RS2", "0")
    two = api.OrtInfer(m).infer(x)[0][1]
    assert np.abs(two - got[0][1]).max() <= 2e-4 * max(1.0, float(np.abs(two).max()))


@pytest.mark.parametrize("case", DS_CASES, ids=[f"C{c[0]}-N{c[1]}-k{c[2]}-s{c[3][0]}{c[3][1]}" for c in DS_CASES])
def test_fused_dsblock_matches_oracle(case, monkeypatch):
    """Conv(depthwise k x k) + act -> Conv(1 x 1) + act (+ residual) runs as one kernel (csrc/dsblock_rs.inc: rolling depthwise sums in
    registers feeding the f32 matrix pipe; csrc/dsblock.inc / dsblock_wa.inc: depthwise into bf16x6 MFMA operand fragments).  Every wave layout, both kernel sizes, all four
    stride combinations, partial edge tiles and channel counts that are not multiples of 32 / 16 -- against the torch-CPU
    interpreter, and against the same graph with the fusion switched off (OAR_FUSE_DSBLOCK=0)."""
    C, Cout, k, stride, N, H, W, act, residual = case
    net = models._Net("ds", seed=C * 7 + Cout, decomposed_hswish=False)
    g = net.g
    g.add_input("x", ["N", C, "H", "W"])
    y = net.conv("x", C, C, k, stride, groups=C, act=act)
    z = net.conv(y, C, Cout, 1, 1, act=None if residual else act)
    if residual:
        r = net.conv("x", C, Cout, 1, stride)              # a second branch with the output's shape
        z = g.op("Relu", [g.op("Add", [z, r])])
    g.nodes.append(models.node("Identity", [z], ["out"]))
    g.add_output("out", ["N", Cout, "H", "W"])
    m = g.model()
    x = np.random.default_rng(1).standard_normal((N, C, H, W)).astype(np.float32)
    got, ref = _check(m, x, tol=2e-4)
    monkeypatch.setenv("OAR_FUSE_DSBLOCK", "0")
    plain = api.OrtInfer(m).infer(x)[0][1]
    assert np.abs(plain - got[0][1]).max() <= 2e-4 * max(1.0, float(np.abs(plain).max()))
    monkeypatch.delenv("OAR_FUSE_DSBLOCK")
    # round 4: the row-streaming kernel (dsblock_rs.inc, f32 matrix pipe) takes the 3x3 blocks it has an instantiation for; the bf16x6
    # kernels it replaced must still agree with the oracle on the same graph (they keep the shapes it does not take)
    monkeypatch.setenv("OAR_DSBLOCK_RS", "0")
    wa = api.OrtInfer(m).infer(x)[0][1]
    assert np.abs(wa - ref[0]).max() <= 2e-4 * max(1.0, float(np.abs(ref[0]).max()))
    if k == 3 and stride == (1, 1):
        # dsblock_wa and dsblock share their arithmetic (FMA chain, exact bf16 split, order of the six products): bit-identical
        monkeypatch.setenv("OAR_DSBLOCK_WA", "0")
        old = api.OrtInfer(m).infer(x)[0][1]
        assert np.array_equal(old, wa)
        monkeypatch.delenv("OAR_DSBLOCK_WA")
    # the chunk-streamed kernel wherever it has an instantiation (OAR_DSBLOCK_CS=2), and the build without it (=0: the wide 5x5 blocks fall back to two
    # convolutions, 96 -> 192 stride (1, 2) to dsblock.inc)
    monkeypatch.delenv("OAR_DSBLOCK_RS")
    for v in ("2", "0"):
        monkeypatch.setenv("OAR_DSBLOCK_CS", v)
        alt = api.OrtInfer(m).infer(x)[0][1]
        assert np.abs(alt - ref[0]).max() <= 2e-4 * max(1.0, float(np.abs(ref[0]).max())), v


@pytest.mark.parametrize("case", ["fpn", "fallbacks"])
def test_deferred_resize_is_absorbed_or_run_in_place(case):
    """A nearest Resize with one consumer runs AT that consumer (engine.cc PendingResize): a channel Concat lets it write into its
    slot, an Add reads the low-resolution operand through the index map (integer factors only), anything else runs it first.
    Same numbers as the oracle either way; the absorbed forms launch no `resize` / `copy2d` for those tensors (round 5: a concat whose
    resized inputs are all integer-factor upsamplings is one `concat_gather` launch)."""
    rng = np.random.default_rng(31)
    sc = lambda f: np.array([1, 1, f, f], np.float32)

    def build(g):
        g.add_input("x", ["N", 8, "H", "W"])
        conv = lambda t, cin, cout, k=1, s=1: g.op("Conv", [t, g.init(rng.standard_normal((cout, cin, k, k)).astype(np.float32) * 0.2), g.init(rng.standard_normal(cout).astype(np.float32) * 0.1)],
                                                     kernel_shape=[k, k], strides=[s, s], pads=[k // 2] * 4, group=1, dilations=[1, 1])
        f2 = conv("x", 8, 16, 3, 1)
        f3 = conv(f2, 16, 16, 3, 2)
        f4 = conv(f3, 16, 16, 3, 2)
        up = lambda t, f, **kw: g.op("Resize", [t, "", g.init(sc(f))], mode="nearest", **(kw or dict(coordinate_transformation_mode="asymmetric", nearest_mode="floor")))
        if case == "fpn":
            o3 = g.op("Add", [f3, up(f4, 2)])                                   # absorbed by the sum (operand order: resize second)
            o2 = g.op("Add", [up(o3, 2, coordinate_transformation_mode="half_pixel", nearest_mode="round_prefer_floor"), f2])   # resize first; another map = o / 2
            p4 = conv(f4, 16, 8)
            p3 = conv(o3, 16, 8)
            p2 = conv(o2, 16, 8)
            cat = g.op("Concat", [up(p4, 4), up(p3, 2), p2], axis=1)           # two resizes write into the concat, one copy
            y = conv(cat, 24, 4, 3, 1)
            return y, ["N", 4, "H", "W"]
        a = g.op("Relu", [up(f4, 2)])                                           # consumer that absorbs nothing: runs in place
        b = g.op("Mul", [f3, up(f4, 2)])                                        # Mul is not absorbed
        u15 = g.op("Resize", [f4, "", g.init(np.array([1, 1, 1.5, 1.5], np.float32))], mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor")
        c = g.op("Add", [u15, g.op("Resize", [f3, "", g.init(np.array([1, 1, 0.75, 0.75], np.float32))], mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor")])
        d = g.op("Concat", [up(f4, 2), f3], axis=2)                             # not the channel axis: materialised, then copied
        g.add_output(c, ["N", 16, "H", "W"])
        g.add_output(d, ["N", 16, "H", "W"])
        return g.op("Add", [a, b]), ["N", 16, "H", "W"]

    model = _single_op_graph(build)
    x = rng.standard_normal((2, 8, 32, 48)).astype(np.float32)
    _check(model, x)
    if case == "fpn":
        eng = api.OrtInfer(model)
        eng.infer(x)
        api.prof_enable(True); api.prof_reset()
        eng.infer(x)
        names = {e["name"]: e["launches"] for e in api.prof_snapshot()}
        api.prof_enable(False)
        assert names.get("resize", 0) == 1, names        # round 5: the concat's two upsamplings and p2's copy are ONE gather launch (class "resize"); the sums absorbed theirs
        assert names.get("copy2d", 0) == 0, names


@pytest.mark.parametrize("case", [("tiny head 64->16->16->1", 64, 16, 1, "Relu"), ("24 mid channels, 2 outputs", 32, 24, 2, "HardSwish"), ("not a pair shape (12 mid channels)", 16, 12, 1, "Relu")])
def test_stacked_convtranspose_pair_is_one_kernel(case):
    """The DB head ends in ConvTranspose 2x2 s2 -> act -> ConvTranspose 2x2 s2 -> Sigmoid: run as ONE kernel (k::convt2x2_pair; the
    4x-pixels intermediate map stays in registers) when the channel counts fit, as two launches otherwise; same numbers as the
    oracle either way, and a first layer with a second consumer is never held back."""
    name, c0, c1, c2, act = case
    rng = np.random.default_rng(len(name))

    def build(g):
        g.add_input("x", ["N", 8, "H", "W"])
        f = g.op("Relu", [g.op("Conv", ["x", g.init(rng.standard_normal((c0, 8, 3, 3)).astype(np.float32) * 0.2), g.init(rng.standard_normal(c0).astype(np.float32) * 0.1)],
                               kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1], group=1, dilations=[1, 1])])
        ct = lambda t, ci, co: g.op("ConvTranspose", [t, g.init((rng.standard_normal((ci, co, 2, 2)) * (1.0 / np.sqrt(ci))).astype(np.float32)), g.init(rng.standard_normal(co).astype(np.float32) * 0.1)],
                                    kernel_shape=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
        a = g.op(act, [ct(f, c0, c1)])
        y = g.op("Sigmoid", [ct(a, c1, c2)])
        # a second branch whose first layer feeds two consumers: must run unfused
        a2 = g.op("Relu", [ct(f, c0, 16)])
        z = g.op("Add", [g.op("Sigmoid", [ct(a2, 16, 1)]), g.op("Sigmoid", [ct(a2, 16, 1)])])
        g.add_output(z, ["N", 1, "H", "W"])
        return y, ["N", c2, "H", "W"]

    model = _single_op_graph(build)
    x = rng.standard_normal((2, 8, 24, 40)).astype(np.float32)
    _check(model, x)
    eng = api.OrtInfer(model)
    eng.infer(x)
    api.prof_enable(True); api.prof_reset()
    eng.infer(x)
    names = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    api.prof_enable(False)
    assert names.get("convt_pair", 0) == (1 if c1 != 12 else 0), names


@pytest.mark.parametrize("n,W", [(5, 320), (3, 184), (1, 8), (3, 480), (2, 520), (2, 1100)])   # W = 480: four token tiles = two per work item (ch_gemm_lds<2>)
@pytest.mark.parametrize("mode", ["lds", "arena"])
def test_sample_local_chain_matches_oracle_and_the_unfused_path(n, W, mode, monkeypatch):
    """The recognizer's SVTR neck (1 x 3 conv, 1 x 1 convs, LayerNorm, QKV / attention / projection, FFN, concat) runs as ONE launch
    (csrc/chain.hip: a workgroup per text line walks the operator table; Planner::fuse_chains).  Same numbers as the torch oracle
    and, to f32 rounding, as the operator-by-operator path (OAR_FUSE_CHAIN=0); argmax identical.  T = W / 8 covers one to three token
    tiles (matrix-pipe attention), T = 65 (two token groups, attention on the any-T path, tensors that no longer all fit LDS) and
    T = 137; `arena` keeps every tensor in HBM (OAR_CHAIN_LDS=0: the general product path)."""
    rec, _ = models.build_rec("tiny", vocab=6906, seed=1)
    x = np.random.default_rng(n * 1000 + W).standard_normal((n, 3, 48, W)).astype(np.float32)
    monkeypatch.setenv("OAR_FUSE_CHAIN", "0")
    plain_eng = api.OrtInfer(rec, profile=True)
    plain = plain_eng.infer(x)[0][1]
    monkeypatch.setenv("OAR_FUSE_CHAIN", "1")
    monkeypatch.setenv("OAR_CHAIN_MAX_MFLOP", "1000")   # (the planner's default cap of 32 MFLOP per line would leave the T = 137 case unfused)
    if mode == "arena":
        monkeypatch.setenv("OAR_CHAIN_LDS", "0")
    eng = api.OrtInfer(rec, profile=True)
    api.prof_enable(True); api.prof_reset()
    got = eng.infer(x)[0][1]
    snap = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    api.prof_enable(False)
    assert snap.get("chain", 0) == 1 and not snap.get("attention", 0) and not snap.get("layernorm", 0), snap
    assert not snap.get("pool2d", 0), snap     # round 5: the [6, 2] average pool in front of the neck is the chain's first operator (CH_POOL)
    ref = onnx_ref.run(rec, {eng.input_name(): x})[0]
    assert np.abs(got - ref).max() <= TOL
    assert np.abs(got - plain).max() <= 5e-5
    assert np.array_equal(got.argmax(-1), plain.argmax(-1)) and np.array_equal(got.argmax(-1), ref.argmax(-1))


def test_non_f32_declared_inputs_and_oversized_integer_outputs_are_errors():
    """oar_input binds f32 only: a model that declares an int64 secondary input is refused instead of being fed reinterpreted floats;
    an integer-typed output whose value does not fit the engine's f32 device tensors (> 2^24) fails instead of coming back rounded."""
    g = GraphBuilder("i64_in")
    g.add_input("x", ["N", 4])
    g.add_input("idx", ["N", 4], elem_type=7)
    y = g.op("Add", ["x", g.op("Cast", ["idx"], to=1)])
    g.add_output(y, ["N", 4])
    eng = api.OrtInfer(g.model())
    with pytest.raises(api.OCRError, match="only f32 inputs"):
        eng.infer([("x", np.zeros((1, 4), np.float32)), ("idx", np.zeros((1, 4), np.float32))])
    eng.close()
    g = GraphBuilder("big_int_out")
    g.add_input("x", ["N", 4])
    big = g.op("Floor", [g.op("Mul", ["x", g.init(np.array(3.0e7, np.float32))])])
    g.add_output(big, ["N", 4], elem_type=7)      # declared int64: comes back as TensorOutput::I64
    eng = api.OrtInfer(g.model())
    with pytest.raises(api.OCRError, match="2\\^24"):
        eng.infer(np.ones((1, 4), np.float32))
    small = eng.infer(np.full((1, 4), 1e-4, np.float32))[0][1]     # 3000: exact
    assert small.dtype == np.int64 and np.all(small == 3000)
    eng.close()


def test_squeeze_excite_scale_rides_on_the_pointwise_conv(monkeypatch):
    """Mul(x, SEGate) -> Conv 1x1 (the tail of a PP-LCNet squeeze-excite block): on layers the bf16x6 weight-stationary kernel takes,
    the gate is multiplied into the pixels as they are loaded (engine_rewrite.cc pass 8, igemm_ws_x6.hip SE variant) -- no `binary` launch, the
    scaled map never reaches HBM -- and the result is BIT-identical to running the Mul (same v_mul_f32, then the same split); layers
    the kernel does not take (the detector's 30 x 30 maps) run the Mul after all.  Both against the torch oracle."""
    rec, _ = models.build_rec("tiny", vocab=6906, seed=1)
    # 160 lines of 48 x 200: 300 pixels per image at the gated layers (not a multiple of the 16-pixel tile: tiles straddle images)
    x = np.random.default_rng(77).standard_normal((160, 3, 48, 200)).astype(np.float32)
    monkeypatch.setenv("OAR_FUSE_SE_SCALE", "0")
    plain = api.OrtInfer(rec).infer(x)[0][1]
    monkeypatch.delenv("OAR_FUSE_SE_SCALE")
    eng = api.OrtInfer(rec, profile=True)
    api.prof_enable(True); api.prof_reset()
    got = eng.infer(x)[0][1]
    snap = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    api.prof_enable(False)
    assert not snap.get("binary", 0), snap
    assert np.array_equal(got, plain)
    ref = onnx_ref.run(rec, {eng.input_name(): x})[0]
    assert np.abs(got - ref).max() <= TOL
    det, _ = models.build_det("tiny", seed=0)
    xd = np.random.default_rng(5).standard_normal((2, 3, 320, 480)).astype(np.float32)
    _check(det, xd)
    # round 5: the detector's gated pointwise convs run on the latency variant of the f32 kernel, which multiplies the gate into its pixel
    # fragments as well: no Mul launch left, bit-identical to running it
    def run_det():
        e = api.OrtInfer(det, profile=True)
        e.infer(xd)
        api.prof_enable(True); api.prof_reset()
        out = e.infer(xd)[0][1]
        sn = {q["name"]: q["launches"] for q in api.prof_snapshot()}
        api.prof_enable(False)
        e.close()
        return out, sn
    monkeypatch.setenv("OAR_FUSE_SE_SCALE_SMALL", "0")
    d0, s0 = run_det()
    monkeypatch.delenv("OAR_FUSE_SE_SCALE_SMALL")
    d1, s1 = run_det()
    assert np.array_equal(d0, d1)
    assert s1.get("binary", 0) == s0.get("binary", 0) - 2, (s0, s1)   # the two squeeze-excite blocks of the stride-32 stage


def test_squeeze_excite_pool_comes_from_the_depthwise_epilogue(monkeypatch):
    """GlobalAveragePool(depthwise conv) (the squeeze of an SE block): the 5 x 5 depthwise kernel writes per-tile sums of its activated
    output and `global_avgpool_finish` -- since round 5 the squeeze-excite gate kernel itself, when the pooled vector feeds nothing else --
    reduces them (engine_rewrite.cc pass 9): the feature map is not read a second time.  Same numbers as the
    oracle, equal to the separate pool to f32 rounding (another summation order: tile sums first), argmax unchanged; 3 x 3 depthwise
    convs (no pooled variant) pool separately."""
    rec, _ = models.build_rec("tiny", vocab=6906, seed=1)
    x = np.random.default_rng(78).standard_normal((160, 3, 48, 200)).astype(np.float32)
    monkeypatch.setenv("OAR_FUSE_SE_POOL", "0")
    plain_eng = api.OrtInfer(rec, profile=True)
    api.prof_enable(True); api.prof_reset()
    plain = plain_eng.infer(x)[0][1]
    before = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    monkeypatch.setenv("OAR_FUSE_SE_POOL", "1")                       # round 4: tile sums + a finishing launch of the pool kernel
    fin_eng = api.OrtInfer(rec, profile=True)
    api.prof_reset()
    fin = fin_eng.infer(x)[0][1]
    mid = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    monkeypatch.delenv("OAR_FUSE_SE_POOL")
    eng = api.OrtInfer(rec, profile=True)                             # round 5 default: the SE gate kernel reduces the tile sums itself
    api.prof_reset()
    got = eng.infer(x)[0][1]
    snap = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    api.prof_enable(False)
    assert mid.get("global_avgpool", 0) == before.get("global_avgpool", 0) and mid.get("conv_dw", 0) == before.get("conv_dw", 0), (before, mid)   # (the finish pass keeps the class name)
    assert snap.get("conv_dw", 0) == before.get("conv_dw", 0) and snap.get("se_fc", 0) == before.get("se_fc", 0) > 0
    assert snap.get("global_avgpool", 0) == before.get("global_avgpool", 0) - snap["se_fc"], (before, snap)   # every squeeze of this graph feeds a gate: no pool launch left for them
    assert np.array_equal(got, fin)                                   # same reduction order inside se_fc as in the finishing launch
    assert np.abs(got - plain).max() <= 2e-5 and np.array_equal(got.argmax(-1), plain.argmax(-1))
    ref = onnx_ref.run(rec, {eng.input_name(): x})[0]
    assert np.abs(got - ref).max() <= TOL
    # a 3 x 3 depthwise conv under a pool: no pooled kernel variant, the planner pools separately
    rng = np.random.default_rng(12)

    def build(g):
        g.add_input("x", ["N", 16, "H", "W"])
        d = g.op("Conv", ["x", g.init(rng.standard_normal((16, 1, 3, 3)).astype(np.float32) * 0.3), g.init(rng.standard_normal(16).astype(np.float32) * 0.1)],
                 kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1], group=16, dilations=[1, 1])
        d = g.op("Relu", [d])
        p = g.op("GlobalAveragePool", [d])
        return g.op("Mul", [d, p]), ["N", 16, "H", "W"]

    _check(_single_op_graph(build), rng.standard_normal((3, 16, 20, 28)).astype(np.float32))
    # and a 5 x 5 one, stride 2, odd sizes (partial tiles at the right / bottom edge)
    def build5(g):
        g.add_input("x", ["N", 24, "H", "W"])
        d = g.op("Conv", ["x", g.init(rng.standard_normal((24, 1, 5, 5)).astype(np.float32) * 0.2), g.init(rng.standard_normal(24).astype(np.float32) * 0.1)],
                 kernel_shape=[5, 5], strides=[2, 2], pads=[2, 2, 2, 2], group=24, dilations=[1, 1])
        d = g.op("HardSwish", [d])
        p = g.op("GlobalAveragePool", [d])
        return g.op("Mul", [d, p]), ["N", 24, "H", "W"]

    _check(_single_op_graph(build5), rng.standard_normal((5, 24, 37, 51)).astype(np.float32))


def test_fpn_sum_reads_the_low_resolution_operand_in_the_conv_epilogue(monkeypatch):
    """lateral 1 x 1 conv + nearest-upsampled top-down tensor (FPN): the folded Add's other operand is a deferred integer-factor Resize,
    so the conv's epilogue reads the LOW-resolution tensor at (h / f, w / f) (igemm_res_off; engine.cc op_conv) -- the upsampled tensor
    is never materialised.  Bit-identical to materialising it (the same f32 add), equal to the oracle; no `resize` launch for the sums."""
    det, _ = models.build_det("tiny", seed=0)
    x = np.random.default_rng(3).standard_normal((3, 3, 320, 480)).astype(np.float32)
    monkeypatch.setenv("OAR_FUSE_RES_UP", "0")
    e0 = api.OrtInfer(det, profile=True)
    api.prof_enable(True); api.prof_reset()
    plain = e0.infer(x)[0][1]
    before = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    monkeypatch.delenv("OAR_FUSE_RES_UP")
    e1 = api.OrtInfer(det, profile=True)
    api.prof_reset()
    got = e1.infer(x)[0][1]
    after = {e["name"]: e["launches"] for e in api.prof_snapshot()}
    api.prof_enable(False)
    assert np.array_equal(got, plain)
    assert after.get("resize", 0) == before.get("resize", 0) - 3, (before, after)     # the three top-down sums
    ref = onnx_ref.run(det, {e1.input_name(): x})[0]
    assert np.abs(got - ref).max() <= TOL


def test_engine_cfg_precision_and_caller_stream():
    """oar_engine_cfg.precision / .stream (SURVEY 8b "Device selection"; VERDICT r5 missing #5): the only arithmetic mode is OAR_PRECISION_F32 -- any
    other value is refused, not silently mapped -- and an engine created on the caller's HIP stream runs there and returns the same numbers."""
    import torch
    det, _ = models.build_det("tiny", seed=0)
    x, _ = R.det_preprocess(pages.make_page(7, (96, 160), lines=2))
    with pytest.raises(api.OCRError) as e:
        api.OrtInfer(det, precision=1)
    assert "precision" in str(e.value)
    own = api.OrtInfer(det)
    want = own.infer(x[None])[0][1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        marker = torch.ones(1 << 20, device="cuda").sum()       # the caller's own work, queued on the same stream in front of the engine's
    eng = api.OrtInfer(det, stream=s.cuda_stream)
    got = eng.infer(x[None])[0][1]
    assert np.array_equal(got, want) and float(marker) == float(1 << 20)
    eng.close()
    s.synchronize()                                              # the stream is the caller's: still usable after the engine is gone
    with torch.cuda.stream(s):
        assert float(torch.ones(8, device="cuda").sum()) == 8.0
    own.close()
