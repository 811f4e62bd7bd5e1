"""The Qwen2-VL and Qwen2.5-VL vision towers on the GPU (vl.QwenVisionEncoder over oar_qvis_*) against the numpy reference in f64
(synth/qwen_vision_reference.py).  For each case the features (the last block's output, in the caller's order) and the merged embeddings are finite and within
their own tol = max(16 noise, 2^-19), noise = max |f32 - f64| of the reference on the same case.  Two calls give the same bytes, the launches the profiler
counts are the ones oar_qvis_cost states, images of one call do not see each other (bitwise), an image alone agrees with the same image inside a call, a bf16
checkpoint computes what its widened values compute, and a bad request is refused."""
import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import qwen_vision_reference as qr

pytestmark = pytest.mark.gpu

_cache = {}


def _cfg(case, **kw):
    d = dict(kind=case.kind, embed_dim=case.D, depth=case.L, num_heads=case.heads, intermediate_size=case.F, patch_size=case.patch, out_hidden_size=case.out_hidden,
             temporal_patch_size=case.temporal, in_channels=case.channels, spatial_merge_size=case.merge, hidden_act=case.act, window_size=case.window_size,
             fullatt_block_indexes=list(case.fullatt), max_tokens=case.tokens, max_images=len(case.grids))
    d.update(kw)
    return vl.QwenVisionConfig(**d)


def _case(name):
    """weights, pixels and the reference bundle: computed once, never modified"""
    if name not in _cache:
        case = qr.QVIS_CASES[name]
        w, px = qr.make_qvision(case), qr.make_qpixels(case)
        _cache[name] = (case, w, px, qr.qvision_bundle(case, w, px))
    return _cache[name]


def _launches(case):
    per_block = 8 if case.kind == "qwen2_5" or case.act == "quick_gelu" else 7
    return 1 + per_block * case.L + 3 + (2 if case.kind == "qwen2_5" else 0)


@pytest.mark.parametrize("name", list(qr.QVIS_CASES))
def test_features_and_embeddings_match_f64(name):
    case, w, px, ref = _case(name)
    with vl.QwenVisionEncoder.from_state_dict(_cfg(case), w) as enc:
        emb, feat = enc.encode(px, case.grids, return_features=True)
        emb2, feat2 = enc.encode(px, case.grids, return_features=True)
        only = enc.encode(px, case.grids)
        api.prof_reset()
        api.prof_enable(True)
        try:
            enc.encode(px, case.grids)
            snap = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["launches"]}
        finally:
            api.prof_enable(False)
        flops, nbytes, launches = enc.cost(case.grids)
    for key, got in (("feat", feat), ("emb", emb)):
        r = ref[key]
        err = float(np.abs(got.astype(np.float64) - r["f64"]).max())
        print(f"case {name} {key}: noise {r['noise']:.2e} tol {r['tol']:.2e} err {err:.2e}")
        assert got.shape == r["f64"].shape and np.isfinite(got).all() and err <= r["tol"], (name, key, err, r["tol"])
    assert emb2.tobytes() == emb.tobytes() and feat2.tobytes() == feat.tobytes() and only.tobytes() == emb.tobytes()   # call to call
    print(snap)
    assert set(snap) <= {"qvis_linear", "qvis_norm", "vis_attention", "qvis_act", "qvis_gather"}, snap
    assert sum(snap.values()) == launches == _launches(case) and flops > 0 and nbytes > 0
    assert snap["vis_attention"] == case.L and snap.get("qvis_gather", 0) == (2 if case.kind == "qwen2_5" else 0)


def test_images_of_one_call_do_not_see_each_other():
    """case W5 with the pixels of its middle image replaced (other values, then NaN): the other two images' features and embeddings are bitwise unchanged"""
    case, w, px, _ = _case("W5")
    a, b = 196, 196 + 256                                                      # the middle image's rows
    with vl.QwenVisionEncoder.from_state_dict(_cfg(case), w) as enc:
        emb, feat = enc.encode(px, case.grids, return_features=True)
        for fill in ("other", "nan"):
            q = px.copy()
            q[a:b] = np.nan if fill == "nan" else np.random.default_rng(9).uniform(-1, 1, q[a:b].shape).astype(np.float32)
            e2, f2 = enc.encode(q, case.grids, return_features=True)
            assert f2[:a].tobytes() == feat[:a].tobytes() and f2[b:].tobytes() == feat[b:].tobytes(), fill
            assert e2[:a // 4].tobytes() == emb[:a // 4].tobytes() and e2[b // 4:].tobytes() == emb[b // 4:].tobytes(), fill
            if fill == "nan":
                assert np.isnan(f2[a:b]).all() and np.isnan(e2[a // 4:b // 4]).all()
            else:
                assert not np.array_equal(f2[a:b], feat[a:b])


@pytest.mark.parametrize("name, image", [("A2", 1), ("W5", 0)])
def test_an_image_alone_agrees_with_the_same_image_inside_a_call(name, image):
    """other tiles, other window offsets, and (at max_tokens far above the case's) other weight formats: the same result within tol"""
    case, w, px, ref = _case(name)
    lens = [h * wd for h, wd in case.grids]
    a = sum(lens[:image])
    b = a + lens[image]
    with vl.QwenVisionEncoder.from_state_dict(_cfg(case, max_tokens=40000, max_images=16), w) as enc:
        emb, feat = enc.encode(px, case.grids, return_features=True)
        alone_e, alone_f = enc.encode(px[a:b], [case.grids[image]], return_features=True)
    assert np.abs(feat - ref["feat"]["f64"]).max() <= ref["feat"]["tol"] and np.abs(emb - ref["emb"]["f64"]).max() <= ref["emb"]["tol"]
    assert np.abs(alone_f - ref["feat"]["f64"][a:b]).max() <= ref["feat"]["tol"] and np.abs(alone_e - ref["emb"]["f64"][a // 4:b // 4]).max() <= ref["emb"]["tol"]


@pytest.mark.parametrize("name", ["W5", "X5"])
def test_rows_near_eps_match_f64(name):
    """the pixels scaled by 1e-3: the first RMSNorm of every row sees mean(x^2) near its eps, so where eps stands in the formula decides the result (put inside the mean's
    divisor it moves W5 and X5 by far more than tol: tests/test_qwen_vision_reference_cpu.py); the same rule, tol from this input's own f32 / f64 references"""
    case, w, px, _ = _case(name)
    small = (px * np.float32(1e-3)).astype(np.float32)
    ref = qr.qvision_bundle(case, w, small)
    with vl.QwenVisionEncoder.from_state_dict(_cfg(case), w) as enc:
        emb, feat = enc.encode(small, case.grids, return_features=True)
    for key, got in (("feat", feat), ("emb", emb)):
        r = ref[key]
        err = float(np.abs(got.astype(np.float64) - r["f64"]).max())
        print(f"case {name} x 1e-3 {key}: noise {r['noise']:.2e} tol {r['tol']:.2e} err {err:.2e}")
        assert np.isfinite(got).all() and err <= r["tol"], (name, key, err, r["tol"])


@pytest.mark.parametrize("name", ["B2", "X5"])
def test_a_bf16_checkpoint_computes_what_its_widened_values_compute(name):
    case, w, px, _ = _case(name)
    from oar_ocr_amd.synth.lm_reference import bf16_bits_to_f32, to_bf16_bits
    bits = {k: to_bf16_bits(v) for k, v in w.items()}
    wide = {k: bf16_bits_to_f32(v).reshape(w[k].shape) for k, v in bits.items()}
    with vl.QwenVisionEncoder.from_state_dict(_cfg(case), bits) as e16, vl.QwenVisionEncoder.from_state_dict(_cfg(case), wide) as e32:
        assert e16.encode(px, case.grids).tobytes() == e32.encode(px, case.grids).tobytes()


def test_bad_requests_are_refused_and_the_model_still_works():
    case, w, px, ref = _case("X5")                                             # grids (4, 36), (6, 6): 180 patches, 2 images
    with vl.QwenVisionEncoder.from_state_dict(_cfg(case), w) as enc:
        for grids, n in (([(4, 36), (6, 6), (2, 2)], 184), ([(3, 8)], 24), ([(4, 36), (6, 8)], 192), ([], 0)):   # too many images, merge, max_tokens, none
            with pytest.raises(api.OCRError) as e:
                enc.encode(np.zeros((n, case.K), np.float32), grids)
            assert e.value.code == api.OAR_INVALID_INPUT, (grids, e.value.code)
        with pytest.raises(api.OCRError):
            enc.encode(np.zeros((180, case.K + 4), np.float32), case.grids)
        emb = enc.encode(px, case.grids)
    assert np.abs(emb - ref["emb"]["f64"]).max() <= ref["emb"]["tol"]
    missing = {k: v for k, v in w.items() if not k.endswith("blocks.1.mlp.up_proj.bias")}
    with pytest.raises(api.OCRError) as e:
        vl.QwenVisionEncoder.from_state_dict(_cfg(case), missing)
    assert e.value.code == api.OAR_INVALID_INPUT and "up_proj.bias" in str(e.value)
    key = "visual.blocks.0.mlp.gate_proj.weight"
    wrong = {"transposed": {**w, key: np.ascontiguousarray(w[key].T)}, "unfused qkv": {**w, "visual.blocks.1.attn.qkv.weight": w["visual.blocks.1.attn.qkv.weight"][:case.D]},
             "a vector as a matrix": {**w, "visual.merger.ln_q.weight": w["visual.merger.ln_q.weight"][None, :]}, "f16": {**w, key: w[key].astype(np.float16).view(np.int16)}}
    for what, tensors in wrong.items():                                        # a wrong shape, and a dtype that is neither float nor bf16 bits
        with pytest.raises(api.OCRError) as e:
            vl.QwenVisionEncoder.from_state_dict(_cfg(case), tensors)
        assert e.value.code == api.OAR_INVALID_INPUT, (what, e.value.code)
    with pytest.raises(api.OCRError) as e:                                     # a rank the tower has no tensor of
        vl.QwenVisionEncoder.from_state_dict(_cfg(case), {**w, key: w[key].reshape(2, 2, 2, 5, 24)})
    assert e.value.code == api.OAR_INVALID_INPUT and "gate_proj" in str(e.value)
