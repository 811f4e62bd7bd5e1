"""Decomposed LayerNorm as one launch and residual add + LayerNorm fused, through the engine (rewrite passes 2c and 10 of engine_rewrite.cc,
Planner::fuse_chains).  Launch classes come from api.prof_snapshot(); every knob is read when the model is loaded, so each test sets it in front of
OrtInfer.  Tolerance, as elsewhere: noise = max |f32 - f64| of the same graph through the oracles, tol = max(16 noise, 2^-19).

All small cases: N = 2, T = 5, C in {32, 132} (132: a float4 tail inside the second register of the half-wave kernels)."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models
from oracle import onnx_np, onnx_ref

pytestmark = pytest.mark.gpu

LN_KNOB, ADD_KNOB = "OAR_FUSE_LAYERNORM", "OAR_FUSE_ADD_LAYERNORM"
N, T = 2, 5
CS = (32, 132)
VARIANTS = [dict(), dict(axes="input"), dict(axis=2), dict(square="mul"), dict(eps_first=True), dict(eps_shape=(1,)), dict(inverse="reciprocal"),
            dict(inverse="div1", inverse_first=True), dict(inverse="reciprocal", inverse_first=True), dict(affine_first=True), dict(affine_rank=3),
            dict(affine="scale"), dict(affine="none"), dict(eps=1e-6), dict(axis2=2), dict(axis=2, axis2=-1)]
MISSES = [dict(miss=m) for m in ("two_axes", "axis_mid", "keepdims0", "power4", "numerator", "m_reader", "d_reader", "v_reader", "r_reader", "eps_dynamic",
                                 "eps_zero", "eps_negative") + models.LN_OUTPUT_MISSES] + [dict(axis=1), dict(shape=(32,)), dict(shape=(132,)),
                                                                            dict(affine_extent=1), dict(shape=(T, 32), affine_rank=3), dict(axis2=1)]   # known at plan time only: the kept nodes run
_ids = lambda kws: ["-".join(f"{k}={v}" for k, v in kw.items()) or "plain" for kw in kws]

_refs = {}


def _reference(key, model, feeds):
    """f64 outputs and tol of a graph: computed once, never modified.  onnx_np (numpy f64) where it knows every operator; else onnx_ref (torch) with f64 feeds,
    which promotes an element-wise graph to f64 throughout, or in f32 for a graph with f32 MatMul / Conv weights in it (then the noise is that of the graph's
    opset-17 twin, given as `key`'s reference by the caller)"""
    if key not in _refs:
        parsed = onnx_ref.parse_model(model)
        try:
            r64 = onnx_np.run(parsed, feeds)
        except NotImplementedError:
            r64 = onnx_ref.run(parsed, {k: np.asarray(v, np.float64) for k, v in feeds.items()})
        r64 = [np.asarray(v, np.float64) for v in r64]
        r32 = [np.asarray(v, np.float64) for v in onnx_ref.run(parsed, feeds)]
        noise = max(float(np.abs(a - b).max()) for a, b in zip(r32, r64))
        _refs[key] = (r64, max(16 * noise, 2.0 ** -19))
    return _refs[key]


def _run(model, feeds):
    """-> the outputs by name and the launch classes"""
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        out = dict(eng.infer(list(feeds.items())))
        snap = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["launches"]}
        return out, snap
    finally:
        api.prof_enable(False)
        eng.close()


def _count(snap, prefix):
    return sum(v for k, v in snap.items() if k.startswith(prefix))


def _x(shape, seed=1):
    return (np.random.default_rng(seed).standard_normal(shape) * 3 + 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ A: the decomposed spelling
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("kw", VARIANTS, ids=_ids(VARIANTS))
def test_each_accepted_spelling_is_one_layernorm_launch(kw, C, monkeypatch):
    kw = dict(kw)
    shape = (N, T, C)
    model, info = models.build_layernorm_case(shape, "decomposed", **kw)
    feeds = {"x": _x(shape)}
    (want,), tol = _reference(("ln", C, tuple(sorted(kw.items()))), model, feeds)
    monkeypatch.setenv(LN_KNOB, "1")
    out, snap = _run(model, feeds)
    err = float(np.abs(out["y"].astype(np.float64) - want).max())
    monkeypatch.setenv(LN_KNOB, "0")
    out0, snap0 = _run(model, feeds)
    err0 = float(np.abs(out0["y"].astype(np.float64) - want).max())
    print(f"{kw} C {C}: fused {sorted(snap.items())} err {err:.2e} | op by op {sum(snap0.values())} launches err {err0:.2e} | tol {tol:.2e}")
    assert snap.get("layernorm", 0) == 1 and _count(snap, "reduce") == 0 and _count(snap, "binary") == 0 and sum(snap.values()) == 1, sorted(snap.items())
    assert err <= tol, (err, tol)
    assert snap0.get("layernorm", 0) == 0 and _count(snap0, "reduce") == 2 and sum(snap0.values()) >= 7, sorted(snap0.items())      # the counter sees the difference
    assert err0 <= tol, (err0, tol)
    # the same weights under the opset-17 node: the same plan, the same bytes
    affine = kw.get("affine", "both")
    twin, _ = models.build_layernorm_case(shape, "op", affine=affine, eps=kw.get("eps", 1e-5))
    monkeypatch.setenv(LN_KNOB, "1")
    out_op, snap_op = _run(twin, feeds)
    assert snap_op == snap, (sorted(snap_op.items()), sorted(snap.items()))
    if affine == "both":                                          # (the op twin of a scale-less case multiplies by 1 and adds 0: -0.0 may become +0.0)
        assert out_op["y"].tobytes() == out["y"].tobytes()
    else:
        assert np.array_equal(out_op["y"], out["y"])


@pytest.mark.parametrize("kw", MISSES, ids=_ids(MISSES))
def test_each_near_miss_stays_op_by_op_and_right(kw, monkeypatch):
    kw = dict(kw)
    shapes = [kw.pop("shape")] if "shape" in kw else [(N, T, C) for C in CS]
    monkeypatch.setenv(LN_KNOB, "1")
    for shape in shapes:
        model, info = models.build_layernorm_case(shape, "decomposed", **kw)
        feeds = {"x": _x(shape)}
        wants, tol = _reference(("miss", shape, tuple(sorted(kw.items()))), model, feeds)
        want = wants[0]
        out, snap = _run(model, feeds)
        err = float(np.abs(out["y"].astype(np.float64) - want).max())
        print(f"{kw} {shape}: {sorted(snap.items())} err {err:.2e} tol {tol:.2e}")
        assert snap.get("layernorm", 0) == 0 and snap.get("add_layernorm", 0) == 0, sorted(snap.items())
        assert out["y"].shape == want.shape and err <= tol, (err, tol)
        if kw.get("miss") in models.LN_OUTPUT_MISSES:          # the intermediate the caller asked for comes back, and is the exporter's own value
            aux = out[models.LN_AUX_OUTPUT]
            err_aux = float(np.abs(aux.astype(np.float64) - wants[1]).max())
            print(f"   {models.LN_AUX_OUTPUT} {aux.shape}: err {err_aux:.2e}")
            assert len(wants) == 2 and aux.shape == wants[1].shape and err_aux <= tol, (err_aux, tol)
        else:
            assert len(wants) == 1


# ------------------------------------------------------------------------------------------------ B: Add + LayerNorm
@pytest.mark.parametrize("spelling", models.LN_SPELLINGS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("form", models.ADD_LAYERNORM_FORMS)
def test_add_layernorm_forms(form, C, spelling, monkeypatch):
    model, info = models.build_add_layernorm_case(N, T, C, form, layernorm=spelling)
    feeds = {"x": _x((N, T, C))}
    if info["r_shape"]:
        feeds["r"] = _x(info["r_shape"], seed=2)
    want, tol = _reference(("add", form, C, spelling), model, feeds)
    monkeypatch.setenv(ADD_KNOB, "1")
    out, snap = _run(model, feeds)
    monkeypatch.setenv(ADD_KNOB, "0")
    out0, snap0 = _run(model, feeds)
    err = float(np.abs(out["y"].astype(np.float64) - want[0]).max())
    print(f"{form} C {C} {spelling}: fused {sorted(snap.items())} | knob off {sorted(snap0.items())} | err {err:.2e} tol {tol:.2e}")
    assert err <= tol, (err, tol)
    assert snap0.get("add_layernorm", 0) == 0 and snap0.get("layernorm", 0) == 1, sorted(snap0.items())
    assert out["y"].tobytes() == out0["y"].tobytes()              # the same operations in the same order
    if form in ("per_sample", "relu", "offset_view"):
        if form == "offset_view":                                 # the operand is a view (no copy in front of the Add): it is the alignment that keeps the pair
            assert _count(snap0, "permute") == 0 and sum(snap0.values()) == 3, sorted(snap0.items())    # Relu, Add, LayerNorm
        assert snap == snap0, (sorted(snap.items()), sorted(snap0.items()))
        return
    assert snap.get("add_layernorm", 0) == 1 and snap.get("layernorm", 0) == 0, sorted(snap.items())
    assert _count(snap, "binary") == _count(snap0, "binary") - 1, (sorted(snap.items()), sorted(snap0.items()))
    if form in ("post", "table", "vector", "sum_output"):
        assert sum(snap.values()) == 1, sorted(snap.items())
    if form == "sum_output":
        b = feeds["r"]
        assert out["s"].tobytes() == (feeds["x"] + b).astype(np.float32).tobytes() and out0["s"].tobytes() == out["s"].tobytes()


# ------------------------------------------------------------------------------------------------ whole blocks in the decomposed spelling
def _aifi(spelling):
    from oar_ocr_amd.synth.mha_reference import aifi_layer_reference, reference_bundle
    H, W, D, nh, F = 3, 4, 32, 4, 64
    model, info = models.build_aifi_layer(H, W, D, nh, F, seed=2, layernorm=spelling)
    src = np.random.default_rng(5).standard_normal((2, H * W, D)).astype(np.float32)
    return model, src, reference_bundle(aifi_layer_reference, info, src)


def test_aifi_layer_decomposed_keeps_its_attention_launch_and_the_plan_of_the_op_spelling():
    model, src, ref = _aifi("decomposed")
    out, snap = _run(model, {"src": src})
    err = float(np.abs(out["y"].astype(np.float64) - ref["f64"]).max())
    print(f"aifi decomposed: {sorted(snap.items())} err {err:.2e} tol {ref['tol']:.2e}")
    assert err <= ref["tol"], (err, ref["tol"])
    assert snap.get("mha_attention", 0) == 1 and snap.get("softmax", 0) == 0 and _count(snap, "reduce") == 0, sorted(snap.items())
    assert snap.get("layernorm", 0) + snap.get("add_layernorm", 0) == 2, sorted(snap.items())
    out_op, snap_op = _run(_aifi("op")[0], {"src": src})
    assert snap_op == snap and out_op["y"].tobytes() == out["y"].tobytes()


def test_aifi_layer_decomposed_has_two_add_layernorm_launches():
    """Both residual adds of the layer follow a Linear (the attention's output projection, the FFN's second Linear), and rewrite pass 4 folds each into that
    Linear as its residual before pass 10 looks.  Neither sum has another reader, so the planner hands each residual to add_layernorm: the Linear writes its
    product alone, and the sum never reaches HBM."""
    model, src, ref = _aifi("decomposed")
    out, snap = _run(model, {"src": src})
    print(f"aifi decomposed: add_layernorm {snap.get('add_layernorm', 0)} layernorm {snap.get('layernorm', 0)} binary {_count(snap, 'binary')}")
    assert snap.get("add_layernorm", 0) == 2 and snap.get("layernorm", 0) == 0, sorted(snap.items())


@pytest.mark.parametrize("block", ["swin", "vit"])
def test_swin_and_vit_blocks_decomposed_keep_their_attention_launch(block, monkeypatch):
    rng = np.random.default_rng(5)
    if block == "swin":
        make = lambda s: models.build_swin_block(4, 8, 24, 3, 4, seed=3, whole=True, layernorm=s)
        x, cls = rng.standard_normal((2, 32, 24)).astype(np.float32), "window_attention"
    else:
        monkeypatch.setenv("OAR_FUSE_RELPOS_ATTENTION", "1")
        make = lambda s: models.build_vit_block(4, 6, 32, 2, ws=0, seed=3, whole=True, layernorm=s)
        x, cls = rng.standard_normal((2, 24, 32)).astype(np.float32), "relpos_attention"
    (want,), tol = _reference((block, "op"), make("op")[0], {"x": x})
    out, snap = _run(make("decomposed")[0], {"x": x})
    out_op, snap_op = _run(make("op")[0], {"x": x})
    err = float(np.abs(out["y"].astype(np.float64) - want).max())
    print(f"{block} decomposed: {sorted(snap.items())} err {err:.2e} tol {tol:.2e}")
    assert snap.get(cls, 0) == 1 and snap.get("softmax", 0) == 0 and _count(snap, "reduce") == 0, sorted(snap.items())
    assert snap == snap_op and out["y"].tobytes() == out_op["y"].tobytes()
    assert err <= tol, (err, tol)


def test_svtrv2_small_is_the_same_plan_in_both_spellings(monkeypatch):
    x = np.random.default_rng(3).random((2, 3, 48, 64)).astype(np.float32)
    op, _ = models.build_rec_svtrv2("svtrv2_small", vocab=97)
    dec, _ = models.build_rec_svtrv2("svtrv2_small", vocab=97, layernorm="decomposed")
    want = np.asarray(onnx_ref.run(op, {"x": x})[0])
    out, snap = _run(dec, {"x": x})
    out_op, snap_op = _run(op, {"x": x})
    monkeypatch.setenv(ADD_KNOB, "0")
    out0, snap0 = _run(op, {"x": x})
    print(f"svtrv2_small: {sorted(snap.items())} | add knob off {sorted(snap0.items())}")
    assert snap == snap_op and out["probs"].tobytes() == out_op["probs"].tobytes()
    assert np.abs(out["probs"] - want).max() <= 2e-4                                    # the suite's tolerance against the torch oracle (tests/test_gpu_engine.py)
    assert out0["probs"].tobytes() == out["probs"].tobytes()
    assert _count(snap, "reduce") == _count(snap_op, "reduce")
    # the three conv-mixer blocks' residual adds (the ones no Linear epilogue takes) are add_layernorm launches now
    assert snap.get("add_layernorm", 0) >= 3 and _count(snap, "binary") == _count(snap0, "binary") - 3, (sorted(snap.items()), sorted(snap0.items()))
