"""Decomposed LayerNorm and residual add + LayerNorm, host side: the input families of synth/layernorm_cases.py can tell a wrong row routine from
the right one, the decomposed and the opset-17 spelling of every builder compute the same values through the numpy oracle, the builders' default bytes are
those of the parent commit, the direct entry point checks its arguments in front of the device, and add_layernorm.hip compiles without scratch or spills.

Tolerance, as elsewhere in the project: noise = max |f32 numpy - f64|, tol = max(16 noise, 2^-19)."""
import hashlib
import re
import subprocess

import numpy as np
import pytest

from oar_ocr_amd import api, build
from oar_ocr_amd.synth import layernorm_cases as lc
from oar_ocr_amd.synth import models

EPS = 1e-5
_cache = {}


def _case(family, shape):
    """inputs and the reference bundle: computed once, never modified"""
    key = (family, shape)
    if key not in _cache:
        rows, C, b_rows = shape
        a, b, g, be = lc.inputs(family, rows, C, b_rows, seed=3)
        _cache[key] = (a, b, g, be, lc.reference_bundle(a, b, b_rows, g, be, EPS))
    return _cache[key]


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=["rows%d_C%d_b%d" % s for s in lc.SHAPES])
def test_the_right_routine_is_within_tol_on_every_family(shape, family):
    a, b, g, be, ref = _case(family, shape)
    y, s = lc.emulate(a, b, shape[2], g, be, EPS)
    err = lc.error(y, s, ref)
    print(f"{shape} {family}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    assert y.dtype == np.float32 and s.tobytes() == ref["sum"].tobytes()
    assert err <= ref["tol"], (err, ref["tol"])
    if lc.takes_v4(shape[1]):                                              # the one-wave form on the same row agrees too (it is what an odd offset selects)
        y1, _ = lc.emulate(a, b, shape[2], g, be, EPS, v4=False)
        assert lc.error(y1, s, ref) <= ref["tol"]


def test_each_fault_is_outside_tol_on_some_case():
    caught = {}
    for fault in lc.FAULTS:
        for family in lc.FAMILIES:
            for shape in lc.SHAPES:
                if fault in ("padded lanes counted", "rows reduced together") and not lc.takes_v4(shape[1]):
                    continue
                a, b, g, be, ref = _case(family, shape)
                y, s = lc.emulate(a, b, shape[2], g, be, EPS, fault=fault)
                err = lc.error(y, s, ref)
                if err > ref["tol"]:
                    caught.setdefault(fault, []).append((family, shape, err / ref["tol"]))
    for fault in lc.FAULTS:
        hits = caught.get(fault, [])
        print(f"{fault}: caught by {len(hits)} cases" + "".join(f"\n    {fam} {sh}: {r:.3g} tol" for fam, sh, r in hits[:6]))
    assert set(caught) == set(lc.FAULTS), sorted(set(lc.FAULTS) - set(caught))
    # the families do what they were built for
    fam = lambda fault: {f for f, _, _ in caught[fault]}
    assert "cancel" in fam("residual ignored") and "cancel" in fam("eps dropped") and "periodic" in fam("b row not modulo") and "offset" in fam("padded lanes counted")


def test_the_reference_is_layernorm_of_the_f32_sum():
    import torch
    a, b, g, be, ref = _case("offset", (15, 132, 5))
    s = torch.from_numpy(a) + torch.from_numpy(b).repeat(3, 1)
    assert s.numpy().tobytes() == ref["sum"].tobytes()
    want = torch.nn.functional.layer_norm(s.double(), (132,), torch.from_numpy(g).double(), torch.from_numpy(be).double(), EPS).numpy()
    assert np.abs(want - ref["f64"]).max() < 1e-12
    with pytest.raises(ValueError):
        lc.inputs("normal", 7, 8, 2)


# ------------------------------------------------------------------------------------------------ the spellings through the numpy oracle
def _oracle(model, feeds):
    """every output in f64.  oracle/onnx_np.py (numpy f64) has no Pow / Sqrt / Reciprocal, so a decomposed spelling goes through oracle/onnx_ref.py, the same
    interpreter over torch: with f64 feeds an element-wise graph is promoted to f64 throughout; a graph with a MatMul or Conv in it (f32 weights) runs in f32"""
    from oracle import onnx_np, onnx_ref
    parsed = onnx_ref.parse_model(model)
    try:
        outs = onnx_np.run(parsed, feeds)
    except NotImplementedError:
        try:
            outs = onnx_ref.run(parsed, {k: np.asarray(v, np.float64) for k, v in feeds.items()})
        except RuntimeError:
            outs = onnx_ref.run(parsed, feeds)
    return [np.asarray(v, np.float64) for v in outs]


def _tol(ref64, feeds, model):
    """the bundle rule on a whole graph: the same graph through the torch f32 interpreter gives the noise"""
    from oracle import onnx_ref
    r32 = np.asarray(onnx_ref.run(onnx_ref.parse_model(model), feeds)[0], np.float64)
    return max(16 * float(np.abs(r32 - ref64).max()), 2.0 ** -19)


VARIANTS = [dict(), dict(axes="input"), dict(axis=2), dict(square="mul"), dict(eps_first=True), dict(eps_shape=(1,)), dict(inverse="reciprocal"),
            dict(inverse="div1", inverse_first=True), dict(inverse="reciprocal", inverse_first=True), dict(affine_first=True), dict(affine_rank=3),
            dict(affine="scale"), dict(affine="none"), dict(axis2=2), dict(axis=2, axis2=-1)]
MISSES = ["two_axes", "axis_mid", "keepdims0", "power4", "numerator", "m_reader", "d_reader", "v_reader", "r_reader", "eps_dynamic", "eps_zero", "eps_negative"] + list(models.LN_OUTPUT_MISSES)


def test_every_accepted_variant_computes_the_op():
    x = np.random.default_rng(1).standard_normal((2, 5, 32)).astype(np.float32) * 3 + 1
    w = models.layernorm_case_weights(32, 0)
    for kw in VARIANTS:
        affine = kw.get("affine", "both")
        model, info = models.build_layernorm_case((2, 5, 32), "decomposed", **kw)
        got = _oracle(model, {"x": x})[0]
        d = x.astype(np.float64) - x.astype(np.float64).mean(-1, keepdims=True)
        want = d / np.sqrt((d * d).mean(-1, keepdims=True) + np.float64(np.float32(EPS)))
        if affine in ("both", "scale"):
            want = want * w["g"].astype(np.float64)
        if affine == "both":
            want = want + w["b"].astype(np.float64)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-12, kw
    op = _oracle(models.build_layernorm_case((2, 5, 32), "op")[0], {"x": x})[0]
    assert np.abs(op - _oracle(models.build_layernorm_case((2, 5, 32), "decomposed")[0], {"x": x})[0]).max() <= 2.0 ** -19      # (onnx_np keeps values in f32 between nodes)


def test_every_near_miss_builds_and_differs_from_the_op_or_is_marked():
    x = np.random.default_rng(1).standard_normal((2, 5, 32)).astype(np.float32) * 3 + 1
    plain = _oracle(models.build_layernorm_case((2, 5, 32), "decomposed")[0], {"x": x})[0]
    x64 = x.astype(np.float64)
    d64 = x64 - x64.mean(-1, keepdims=True)
    v64 = (d64 * d64).mean(-1, keepdims=True)
    inner = {"m_output": x64.mean(-1, keepdims=True), "d_output": d64, "v_output": v64, "r_output": np.sqrt(v64 + np.float64(np.float32(EPS)))}
    for miss in MISSES:
        outs = _oracle(models.build_layernorm_case((2, 5, 32), "decomposed", miss=miss)[0], {"x": x})
        got = outs[0]
        assert got.shape == plain.shape and np.isfinite(got).all(), miss
        same = float(np.abs(got - plain).max()) < 1e-4
        assert same == (miss in ("keepdims0", "eps_dynamic", "eps_zero", "eps_negative") + models.LN_OUTPUT_MISSES), (miss, float(np.abs(got - plain).max()))
        # an *_output miss is the accepted form but for the graph output: y is the plain one, and the second output is that intermediate
        assert len(outs) == (2 if miss in inner else 1), miss
        if miss in inner:
            assert outs[1].shape == inner[miss].shape and np.abs(outs[1] - inner[miss]).max() < 1e-12, miss
    assert np.isfinite(_oracle(models.build_layernorm_case((32,), "decomposed")[0], {"x": x[0, 0]})[0]).all()      # rank 1
    # scale and bias of one element broadcast over the channels; a [1, 1, C] scale over a rank-2 x lifts the result to rank 3
    w = models.layernorm_case_weights(32, 0)
    core = _oracle(models.build_layernorm_case((2, 5, 32), "decomposed", affine="none")[0], {"x": x})[0]
    one = _oracle(models.build_layernorm_case((2, 5, 32), "decomposed", affine_extent=1)[0], {"x": x})[0]
    assert np.abs(one - (core * np.float64(w["g"][0]) + np.float64(w["b"][0]))).max() < 1e-12
    lifted = _oracle(models.build_layernorm_case((5, 32), "decomposed", affine_rank=3)[0], {"x": x[0]})[0]
    assert lifted.shape == (1, 5, 32) and np.abs(lifted[0] - plain[0]).max() < 1e-12
    with pytest.raises(ValueError):
        models.build_layernorm_case((2, 5, 32), "op", affine_extent=1)
    with pytest.raises(ValueError):
        models.build_layernorm_case((2, 5, 32), "decomposed", miss="nothing")


@pytest.mark.parametrize("form", models.ADD_LAYERNORM_FORMS)
def test_add_layernorm_forms_agree_in_both_spellings(form):
    N, T, C = 2, 5, 32
    rng = np.random.default_rng(4)
    outs = {}
    for spelling in models.LN_SPELLINGS:
        model, info = models.build_add_layernorm_case(N, T, C, form, layernorm=spelling)
        feeds = {"x": rng.standard_normal((N, T, C)).astype(np.float32)} if not outs else dict(feeds)
        if info["r_shape"] and "r" not in feeds:
            feeds["r"] = rng.standard_normal(info["r_shape"]).astype(np.float32)
        outs[spelling] = (_oracle(model, feeds), _tol(_oracle(model, feeds)[0], feeds, model))
    (a, tol), (b, _) = outs["op"], outs["decomposed"]
    assert len(a) == len(b) == (2 if form == "sum_output" else 1)
    assert max(float(np.abs(p - q).max()) for p, q in zip(a, b)) <= tol


def test_blocks_agree_in_both_spellings():
    rng = np.random.default_rng(5)
    cases = [("aifi", lambda s: models.build_aifi_layer(3, 4, 32, 4, 64, seed=2, layernorm=s), {"src": rng.standard_normal((2, 12, 32)).astype(np.float32)}),
             ("swin", lambda s: models.build_swin_block(4, 8, 24, 3, 4, seed=3, whole=True, layernorm=s), {"x": rng.standard_normal((2, 32, 24)).astype(np.float32)}),
             ("vit", lambda s: models.build_vit_block(4, 6, 32, 2, ws=0, seed=3, whole=True, layernorm=s), {"x": rng.standard_normal((2, 24, 32)).astype(np.float32)}),
             ("svtrv2", lambda s: models.build_rec_svtrv2("svtrv2_small", vocab=40, layernorm=s), {"x": rng.random((1, 3, 48, 32)).astype(np.float32)})]
    for name, make, feeds in cases:
        op, dec = make("op"), make("decomposed")
        assert op[0] != dec[0], name
        a, b = _oracle(op[0], feeds)[0], _oracle(dec[0], feeds)[0]
        tol = _tol(a, feeds, op[0])
        err = float(np.abs(a - b).max())
        print(f"{name}: op vs decomposed {err:.2e} tol {tol:.2e}")
        assert a.shape == b.shape and err <= tol, (name, err, tol)
    with pytest.raises(ValueError):
        models.build_aifi_layer(3, 4, 32, 4, 64, layernorm="spelled")


def test_default_bytes_are_those_of_the_parent():
    """layernorm = "op" writes what the builders wrote before the keyword existed: SHA-256 of each default model, computed on the parent commit"""
    sha = lambda m: hashlib.sha256(m[0]).hexdigest()
    assert sha(models.build_rec_svtrv2("svtrv2_small")) == "3690d0faa77a95d25653cbfc8431791e302142c681063e7fb2fdd139b2ce2b22"
    assert sha(models.build_rec_svtrv2()) == "8ee6de1c37d4e420744f834a438b7ed23f5a9ab360b44c086c52756df4c3a812"
    assert sha(models.build_aifi_layer(5, 7, 32, 4, 64, seed=2)) == "cc8af56bb50cf5b2d4e6eb80071809dd050d9f6cb648327df9654d617311db2f"
    assert sha(models.build_swin_block(14, 21, 24, 3, 7, seed=3)) == "8846212ecc6f31f685bc0af9ed7e676f8955265dd9204d6e8ba97a39b9c79734"
    assert sha(models.build_swin_block(14, 21, 24, 3, 7, seed=3, whole=True)) == "15c2f4cbf550bda5a21516b70345b6b8f266fb97b943050583acba3e3fb1e4a1"
    assert sha(models.build_vit_block(5, 7, 32, 2, ws=4, seed=3)) == "f1b5499a3f5501fc4a3e121fffa8a7c50572123dc5891671ac0a906a6f277529"
    assert sha(models.build_vit_block(5, 7, 32, 2, ws=0, seed=3, whole=True)) == "d6233a2faa2014293d68e43f07cd5ba2c46f56ebf093df7b4ad2af44c3f8f78e"
    assert sha(models.build_p2o_fixture()) == "ac30548278c116faa600d2b2a997eb8dde434fd3d9eb1817df4a1cbb7d25c39b"
    assert sha(models.build_unimernet()) == "04f5d76c4d2e6253280b7d5104ef61ca594befa9df553d0b2271943c1e2379b7"
    assert models.build_aifi_layer(5, 7, 32, 4, 64, seed=2, layernorm="op")[0] == models.build_aifi_layer(5, 7, 32, 4, 64, seed=2)[0]


# ------------------------------------------------------------------------------------------------ the entry point's argument checks (no launch, no device)
@pytest.fixture(scope="module")
def L():
    build.build_lib()
    return api.lib()


def test_entry_point_is_exported_and_rejects_bad_arguments_in_front_of_the_device(L):
    assert "oar_k_add_layernorm" in api.EXPORTS and hasattr(L, "oar_k_add_layernorm") and callable(api.k_add_layernorm)
    ok = (api.OAR_OK,) if api.device_count() > 0 else (api.OAR_DEVICE,)

    def code(rows=6, C=8, b_rows=3, eps=1e-5, write_sum=1, o_floats=100, y_off=0, s_off=48, a=True, b=True, o=True, g=True, be=True):
        z = lambda n: np.zeros(max(int(n), 1), np.float32)
        A, B, G, E, O = z(rows * C), z(b_rows * C), z(C), z(C), z(o_floats)
        p = lambda v, on: api._p(v) if on else None
        return L.oar_k_add_layernorm(p(A, a), p(B, b), b_rows, p(G, g), p(E, be), rows, C, eps, write_sum, p(O, o), o_floats, y_off, s_off)
    assert code() in ok and code(g=False, be=False) in ok and code(b_rows=6) in ok and code(b_rows=1) in ok
    assert code(y_off=1, s_off=51) in ok and code(write_sum=0, s_off=10 ** 9) in ok            # odd offsets are legal; an unused s_off is not looked at
    bad = api.OAR_INVALID_INPUT
    assert code(a=False) == bad and code(b=False) == bad and code(o=False) == bad
    for kw in (dict(rows=0), dict(rows=-6), dict(C=0), dict(C=-8), dict(b_rows=0), dict(b_rows=-3)):
        assert code(**kw) == bad, kw
    assert code(b_rows=4) == bad and code(b_rows=12) == bad                                     # b_rows does not divide rows
    for eps in (0.0, -1e-5, float("nan")):
        assert code(eps=eps) == bad, eps
    assert code(o_floats=95) == bad and code(y_off=53) == bad and code(s_off=53) == bad          # an output that does not fit
    assert code(y_off=2 ** 64 - 4) == bad and code(s_off=2 ** 63) == bad                         # off + need would wrap
    assert code(s_off=47) == bad and code(y_off=4, s_off=0) == bad and code(s_off=0) == bad      # y and the sum overlap
    assert code(write_sum=0, o_floats=48) in ok and code(o_floats=96) in ok
    with pytest.raises(api.OCRError) as e:
        api.k_add_layernorm(np.zeros((6, 8), np.float32), np.zeros((4, 8), np.float32), None, None, 1e-5, False, np.zeros(48, np.float32), 0)
    assert e.value.code == bad and "divide" in str(e.value)
    with pytest.raises(ValueError):
        api.k_add_layernorm(np.zeros((6, 8), np.float32), np.zeros((3, 8), np.float32), np.zeros(7, np.float32), None, 1e-5, False, np.zeros(48, np.float32), 0)


# ------------------------------------------------------------------------------------------------ the kernel's resources
def test_add_layernorm_kernel_resources():
    """add_layernorm.hip with the build's own flags: 2 one-wave and 10 half-wave instantiations (NV in 1, 2, 3, 4, 8, with and without the stored sum), none
    with scratch or a spilled register, none with LDS"""
    src = build.CSRC / "add_layernorm.hip"
    assert "add_layernorm.hip" in build.SOURCES
    r = subprocess.run([build.HIPCC] + build.FLAGS + ["-c", str(src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    print({k: v for k, v in sorted(kernels.items())})
    assert len(kernels) == 12 and all("add_layernorm" in k for k in kernels), sorted(kernels)
    assert sum("v4" in k for k in kernels) == 10
    for k, v in kernels.items():
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0 and v["lds"] == 0, (k, v)
        assert v["vgprs"] <= 64, (k, v)                                      # 8 float4s of one row and their addresses: eight waves per SIMD stay possible
