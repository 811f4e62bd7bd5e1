"""The bf16x6 convolution kernels against float64, held to the error of f32 arithmetic -- not to the suite's 2e-4, under which a kernel
that loses a whole slice product still passes 15 times over.

Every case of oar_ocr_amd/synth/x6_cases.py::GPU_CASES is a one-layer graph at the smallest shape its kernel's selection rule takes; the profile proves
the kernel ran.  Per input family: max |got - f64| / S <= tol_S with S = the operation on absolute values and tol_S = 4 max(noise_S, emu_S), measured
on the case's own sample (plain f32 product and fault-free bf16x6 emulator against f64); tests/test_x6_cases_cpu.py shows on the CPU that this bound
lies at least four times under every emulated fault on the `cancel` family only (the others check what it does not cover).  `pow2` must reproduce `normal` bit
for bit, `poison` must keep one NaN / inf inside its receptive field.  Two layers rerun on the f32 kernels in a child process (OAR_IGEMM_X6 is read once per
process).  The fused kernels whose output is not linear in one product (dsblock, dsblock_wa, dsblock_cs, attention_x6, ctc_head_x6) are held to 4 max |f32 numpy - f64|."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import x6_cases as C
from oar_ocr_amd.synth.child_run import infer_in_child
from oar_ocr_amd.synth.ctc_tail_cases import ctc_model as _ctc_model
from oar_ocr_amd.synth.onnx_writer import GraphBuilder

pytestmark = pytest.mark.gpu
IDS = [c.name for c in C.GPU_CASES]
_NORMAL = {}     # case name -> (reference bundle, GPU output) of the `normal` family: pow2 and poison compare with it; one case at a time is kept


def conv_model(case, w, b):
    g = GraphBuilder("x6")
    g.add_input("x", ["N", case.in_ch, "H", "W"])
    p = case.k // 2
    src = "x"
    if case.msrc:
        t = g.op("AveragePool", ["x"], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0])     # (the identity, NaN included; its output is channels-last, as the deferred Concat asks of its sources)
        src = g.op("Concat", [g.op("Relu", [t]), g.op("Neg", [t]), g.op("Abs", [t])], axis=1)
    if case.se:      # GlobalAveragePool -> Conv + Relu -> Conv + HardSigmoid -> Mul: the gate of x6_cases.se_gate, folded into the convolution's loads
        w1, b1, w2, b2, _ = C.se_gate(case)
        one = dict(kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
        h = g.op("Relu", [g.op("Conv", [g.op("GlobalAveragePool", ["x"]), g.init(w1), g.init(b1)], **one)])
        src = g.op("Mul", ["x", g.op("HardSigmoid", [g.op("Conv", [h, g.init(w2), g.init(b2)], **one)], alpha=C.SE_ALPHA, beta=C.SE_BETA)])
    y = g.op("Conv", [src, g.init(w), g.init(b)], kernel_shape=[case.k, case.k], strides=[1, 1], pads=[p, p, p, p], group=case.group, dilations=[1, 1])
    if case.relu:
        y = g.op("Relu", [y])
    g.add_output(y, ["N", case.cout, "H", "W"])
    return g.model()


def run_layer(case, x, w, b):
    """the layer on the GPU -> output; asserts that the case's kernel class ran"""
    eng = api.OrtInfer(conv_model(case, w, b), profile=True)
    try:
        api.prof_enable(True); api.prof_reset()
        got = eng.infer(x)[0][1]
        names = {e["name"] for e in api.prof_snapshot() if e["launches"]}
    finally:
        api.prof_enable(False)
        eng.close()
    assert case.kernel in names, (case.kernel, sorted(names))
    assert not (case.se and "binary" in names), sorted(names)     # the gate rode on the convolution: no Mul launch
    assert not (case.msrc and any("concat" in n or "copy" in n for n in names)), sorted(names)     # the convolution read the three sources itself: no concatenation
    return got


def _act(case, a):
    return np.where(a < 0, 0.0, a) if case.relu else a     # (NaN stays NaN)


def _report(case, family, ref, err):
    lg = lambda v: f"2^{np.log2(v):.1f}" if v > 0 else "0"
    print(f"\n[x6] {case.name} | {case.kernel} | {family} | noise_S {lg(ref['noise_S'])} | emu_S {lg(ref['emu_S'])} | tol_S {lg(ref['tol_S'])} | err_S {lg(err)}")


def _check_family(case, family):
    x, w, b = C.case_inputs(case, family)
    ref = C.reference_bundle(case, C.gated(case, x), w, b)
    got = run_layer(case, x, w, b)
    assert got.shape == ref["f64"].shape and np.isfinite(got).all()
    err = float((np.abs(got.astype(np.float64) - _act(case, ref["f64"])) / ref["S"]).max())
    _report(case, family, ref, err)
    assert err <= ref["tol_S"], (case.name, family, err, ref["tol_S"])
    return ref, got


def _normal(case):
    if case.name not in _NORMAL:
        _NORMAL.clear()
        _NORMAL[case.name] = _check_family(case, "normal")
    return _NORMAL[case.name]


CHECKS = ("normal", "positive", "dense", "cancel", "pow2", "poison nan", "poison inf")


PAIRS = [(c.name, k) for c in C.GPU_CASES for k in CHECKS if c.poison or not k.startswith("poison")]     # (the checks of one case run back to back:
                                                                                                            # they share its `normal` reference and output)

@pytest.mark.parametrize("name,check", PAIRS, ids=[f"{n}-{k}" for n, k in PAIRS])
def test_x6_kernel(name, check):
    """normal ... cancel: the family's error against float64 within its tol_S.
    pow2 (x 2^40, w 2^-25, bias 2^15): every product, partial sum and rounding of a correct kernel scales by 2^15 exactly -- the output is `normal`'s, bit for bit.
    poison: one NaN (or +inf, which the split turns into NaN) in the last partial pixel tile, in the channel group the K tail re-reads, or where the clamped
    addresses of padding taps point: the non-finite outputs are exactly those of the float64 reference, every other output is as accurate as without it."""
    case = C.case_by_name(name)
    if check == "normal":
        _NORMAL.pop(name, None)
        _normal(case)
    elif check == "pow2":
        _, plain = _normal(case)
        _, scaled = _check_family(case, "pow2")
        assert np.array_equal(scaled.view(np.uint32), np.ldexp(plain, C.POW2_B).view(np.uint32))
    elif check.startswith("poison"):
        _check_poison(case, check.split()[1])
    else:
        _check_family(case, check)


def _check_poison(case, kind):
    ref, _ = _normal(case)
    x, w, b = C.poison_inputs(case, kind)
    got = run_layer(case, x, w, b)
    with np.errstate(invalid="ignore"):
        lin = C.conv_ref(C.gated(case, x), w, b, case.group, "float64")
        f64 = _act(case, lin)
    # the set is taken in front of the activation: Relu makes 0 of a -inf, which the kernel -- whose split has made NaN of the inf already -- cannot follow
    bad = ~np.isfinite(lin)
    assert bad.sum() == (case.cout // case.group) * _field(case), bad.sum()     # (the reference itself: one group's channels at the pixels whose window holds the element)
    spread = ~np.isfinite(got) & ~bad
    lost = np.isfinite(got) & bad
    assert not spread.any() and not lost.any(), (case.name, kind, int(spread.sum()), int(lost.sum()), np.argwhere(spread)[:8].tolist(), np.argwhere(lost)[:8].tolist())
    err = float((np.abs(got.astype(np.float64) - f64)[~bad] / ref["S"][~bad]).max())
    _report(case, f"poison {kind}", ref, err)
    assert err <= ref["tol_S"], (case.name, kind, err, ref["tol_S"])


def _field(case):
    """output pixels that see the poisoned element"""
    _, _, py, px = C.poison_at(case)
    r = case.k // 2
    return (min(case.h - 1, py + r) - max(0, py - r) + 1) * (min(case.w - 1, px + r) - max(0, px - r) + 1)


@pytest.mark.parametrize("name,switch", [("ws_x6 K96 pf1", "OAR_IGEMM_X6"), ("os_x6 3x3 32->1024", "OAR_IGEMM_X6")])
def test_f32_kernel_in_a_child_process_agrees(name, switch, tmp_path):
    """the same layer and input with the bf16x6 kernel switched off (a fresh process: the switches are read once): an f32 kernel class runs, and both
    kernels lie within tol_S of float64"""
    case = C.case_by_name(name)
    ref, got = _normal(case)
    x, w, b = C.case_inputs(case, "normal")
    y32, names = infer_in_child(conv_model(case, w, b), x, {switch: "0"}, tmp_path)
    assert not any(n.endswith("_x6") for n in names) and names & {"conv_igemm", "conv_igemm_ws"}, sorted(names)
    f64 = _act(case, ref["f64"])
    e6 = float((np.abs(got.astype(np.float64) - f64) / ref["S"]).max())
    e32 = float((np.abs(y32.astype(np.float64) - f64) / ref["S"]).max())
    _report(case, f"f32 kernel ({switch}=0)", ref, e32)
    assert e6 <= ref["tol_S"] and e32 <= ref["tol_S"], (e6, e32, ref["tol_S"])


# ------------------------------------------------------------------------------------------------ fused kernels: not linear in one product
def _fused_report(name, kernel, family, b, err):
    lg = lambda v: f"2^{np.log2(v / b['scale']):.1f}" if v > 0 else "0"
    print(f"\n[x6] {name} | {kernel} | {family} | noise {lg(b['noise'])} | tol {lg(b['tol'])} | err {lg(err)}  (of the output scale {b['scale']:.3g})")


def _ds_model(case, wd, bd, wp, bp):
    g = GraphBuilder("ds")
    g.add_input("x", ["N", case.c, "H", "W"])
    p = case.k // 2
    act = lambda t: g.op("Relu", [t]) if case.act == "relu" else g.op("HardSwish", [t]) if case.act == "hswish" else t
    t = act(g.op("Conv", ["x", g.init(wd), g.init(bd)], kernel_shape=[case.k, case.k], strides=[1, 1], pads=[p, p, p, p], group=case.c, dilations=[1, 1]))
    y = act(g.op("Conv", [t, g.init(wp), g.init(bp)], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1]))
    g.add_output(y, ["N", case.cout, "H", "W"])
    return g.model()


def _ds_run(case, family, monkeypatch):
    inp = C.ds_inputs(case, family)
    for k, v in case.env:
        monkeypatch.setenv(k, v)      # (read per call by the planner and the launch)
    eng = api.OrtInfer(_ds_model(case, *inp[1:]), profile=True)
    try:
        api.prof_enable(True); api.prof_reset()
        got = eng.infer(inp[0])[0][1]
        names = {e["name"] for e in api.prof_snapshot() if e["launches"]}
    finally:
        api.prof_enable(False)
        eng.close()
    assert case.kernel in names and not any(n.startswith("conv") for n in names), (case.kernel, sorted(names))
    b = C.fused_bundle(lambda dt: C.ds_ref(case, *inp, dtype=dt))
    err = float(np.abs(got.astype(np.float64) - b["f64"]).max())
    _fused_report(case.name, case.kernel, family, b, err)
    assert err <= b["tol"], (case.name, family, err, b["tol"])
    return got


@pytest.mark.parametrize("case", C.DS_CASES, ids=[c.name for c in C.DS_CASES])
def test_fused_dsblock_kernels(case, monkeypatch):
    """depthwise + act -> pointwise (bf16x6) + act in one launch, each bf16x6 kernel forced by its per-call switch: within 4 max |f32 - f64| of float64 on
    normal and positive inputs, and the pow2 scaling (activation none / Relu) gives `normal`'s bits"""
    plain = _ds_run(case, "normal", monkeypatch)
    _ds_run(case, "positive", monkeypatch)
    scaled = _ds_run(case, "pow2", monkeypatch)
    assert np.array_equal(scaled.view(np.uint32), np.ldexp(plain, C.POW2_B).view(np.uint32))


@pytest.mark.parametrize("case", C.ATTN_CASES, ids=[c[0] for c in C.ATTN_CASES])
@pytest.mark.parametrize("family", ["normal", "positive"])
def test_attention_x6_kernel(case, family):
    """attention_x6.hip (head dim 32, more than 32 tokens: past the kernel that keeps a whole head in LDS registers) behind its projection, as the
    recognizer graphs emit the block: within 4 max |f32 - f64| of float64"""
    name, dim, heads, n, T = case
    x, w, bq = C.attn_inputs(dim, heads, n, T, family)
    g = GraphBuilder("attn")
    g.add_input("x", ["N", "T", dim])
    qkv = g.op("Add", [g.op("MatMul", ["x", g.init(w)]), g.init(bq)])
    qkv = g.op("Transpose", [g.op("Reshape", [qkv, g.init(np.array([0, -1, 3, heads, dim // heads], np.int64), "shape")])], perm=[2, 0, 3, 1, 4])
    q, k, v = g.op("Split", [qkv], n_out=3, axis=0)
    ax0 = g.init(np.array([0], np.int64), "axes")
    q, k, v = g.op("Squeeze", [q, ax0]), g.op("Squeeze", [k, ax0]), g.op("Squeeze", [v, ax0])
    q = g.op("Mul", [q, g.init(np.array((dim // heads) ** -0.5, np.float32), "scale")])
    att = g.op("Softmax", [g.op("MatMul", [q, g.op("Transpose", [k], perm=[0, 1, 3, 2])])], axis=-1)
    o = g.op("Reshape", [g.op("Transpose", [g.op("MatMul", [att, v])], perm=[0, 2, 1, 3]), g.init(np.array([0, -1, dim], np.int64), "shape")])
    g.add_output(o, ["N", "T", dim])
    eng = api.OrtInfer(g.model(), profile=True)
    try:
        api.prof_enable(True); api.prof_reset()
        got = eng.infer(x)[0][1]
        names = {e["name"] for e in api.prof_snapshot() if e["launches"]}
    finally:
        api.prof_enable(False)
        eng.close()
    assert "attention_x6" in names, sorted(names)
    b = C.fused_bundle(lambda dt: C.attn_ref(x, w, bq, heads, dt))
    err = float(np.abs(got.astype(np.float64) - b["f64"]).max())
    _fused_report(name, "attention_x6", family, b, err)
    assert err <= b["tol"], (name, family, err, b["tol"])


@pytest.mark.parametrize("family", ["normal", "positive"])
@pytest.mark.parametrize("case", C.CTC_CASES, ids=[c[0] for c in C.CTC_CASES])
def test_ctc_head_x6_kernel(case, family):
    """ctc_head_x6.hip behind a recognizer made of one feature layer: the features come from the engine on the graph cut in front of the Linear, the arg max
    and its probability are compared with the float64 soft-max of the float64 head on those features, within 4 max |f32 numpy - f64|.  The index must agree
    wherever the float64 runner-up lies further below than that bound."""
    from oar_ocr_amd.synth import models
    name, K, V = case
    crops, sel, fb, w, b = C.ctc_inputs(K, V, family)
    chars = api.read_dict(models.synth_dict(V - 2))
    pred = api.TextRecognitionPredictor(_ctc_model(K, V, sel, fb, w, b), chars)
    try:
        api.prof_enable(True); api.prof_reset()
        got = pred.predict(crops)
        names = {e["name"] for e in api.prof_snapshot() if e["launches"]}
    finally:
        api.prof_enable(False)
        pred.close()
    assert "ctc_head_x6" in names, sorted(names)
    x = api.k_rec_preprocess(crops)
    F = api.OrtInfer(_ctc_model(K, V, sel, fb, w, b, head=False)).infer(x)[0][1].reshape(-1, K)
    assert np.array_equal(F, C.ctc_select(x, sel, fb))                         # the feature layer selects: its output is known exactly from its input
    assert np.abs(x - C.ctc_pixels(crops)).max() <= 1e-6                      # (and the input is what the CPU test's stand-in says, to f32 rounding)
    i64, p64 = C.ctc_ref(F, w, b, "float64")
    _, p32 = C.ctc_ref(F, w, b, "float32")
    bundle = dict(noise=float(np.abs(p32 - p64).max()), scale=float(p64.max()))
    bundle["tol"] = 4.0 * bundle["noise"]
    gi, gp = got.indices.reshape(-1), got.probs.reshape(-1).astype(np.float64)
    err = float(np.abs(gp - p64).max())
    _fused_report(name, "ctc_head_x6", family, bundle, err)
    assert err <= bundle["tol"], (name, family, err, bundle["tol"])
    z = F.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    p = np.exp(z - z.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    second = np.sort(p, -1)[:, -2]
    clear = p64 - second > bundle["tol"]
    assert clear.mean() > 0.9 and np.array_equal(gi[clear], i64[clear])
