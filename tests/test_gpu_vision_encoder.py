"""The vision encoder and projector on the GPU (vl.VisionEncoder over oar_vis_*) against the torch reference in f64 (synth/vision_reference.py).
For each case the features (post_layernorm) and the projected embeddings are finite and within their own tol = max(16 noise, 2^-19), noise = max |f32 - f64|
of the reference on the same case.  Images of one call do not see each other (bitwise), two calls give the same bytes, a larger max_tokens gives the same
result within tol, a bf16 checkpoint computes what its widened values compute, and a bad request is refused."""
import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import vision_reference as vr

pytestmark = pytest.mark.gpu

_cache = {}


def _cfg(case, **kw):
    d = dict(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, intermediate_size=case.F, patch_size=case.patch, text_hidden=case.text_hidden,
             pos_grid=case.G, spatial_merge_size=case.merge, layer_norm_eps=case.eps, hidden_act=case.act, max_tokens=case.tokens, max_images=len(case.grids))
    d.update(kw)
    return vl.VisionConfig(**d)


def _case(name):
    """weights, pixels and the reference bundle: computed once, never modified"""
    if name not in _cache:
        case = vr.ENCODER_CASES[name]
        w, px = vr.make_vision(case), vr.make_pixels(case)
        _cache[name] = (case, w, px, vr.vision_bundle(case, w, px))
    return _cache[name]


@pytest.mark.parametrize("name", list(vr.ENCODER_CASES))
def test_features_and_embeddings_match_f64(name):
    case, w, px, ref = _case(name)
    with vl.VisionEncoder.from_state_dict(_cfg(case), w) as enc:
        emb, feat = enc.encode(px, case.grids, return_features=True)
        emb2, feat2 = enc.encode(px, case.grids, return_features=True)
        only = enc.encode(px, case.grids)
        flops, nbytes, launches = enc.cost(case.grids)
    for key, got in (("feat", feat), ("emb", emb)):
        r = ref[key]
        err = float(np.abs(got.astype(np.float64) - r["f64"]).max())
        print(f"case {name} {key}: noise {r['noise']:.2e} tol {r['tol']:.2e} err {err:.2e}")
        assert got.shape == r["f64"].shape and np.isfinite(got).all() and err <= r["tol"], (name, key, err, r["tol"])
    assert emb2.tobytes() == emb.tobytes() and feat2.tobytes() == feat.tobytes() and only.tobytes() == emb.tobytes()   # call to call
    assert launches == 8 * case.L + 7 and flops > 0 and nbytes > 0                      # (every case uses the tanh GELU: 8 launches per layer)


def test_images_of_one_call_do_not_see_each_other():
    """case P with the pixels of its middle image replaced (other values, then NaN): the other two images' features and embeddings are bitwise unchanged"""
    case, w, px, _ = _case("P")
    a, b = 4, 64                                                               # the middle image's rows
    with vl.VisionEncoder.from_state_dict(_cfg(case), w) as enc:
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


def test_a_larger_max_tokens_and_another_composition_agree_within_tol():
    """max_tokens far above what the case needs picks other weight formats (at 40000 rows the layer Linears take the bf16x6 format, which then serves a call of 204 rows), and
    an image encoded alone runs in other tiles: the same result within tol"""
    case, w, px, ref = _case("P")
    with vl.VisionEncoder.from_state_dict(_cfg(case, max_tokens=40000, max_images=16), w) as enc:
        emb, feat = enc.encode(px, case.grids, return_features=True)
        alone_e, alone_f = enc.encode(px[4:64], [case.grids[1]], return_features=True)
    assert np.abs(feat - ref["feat"]["f64"]).max() <= ref["feat"]["tol"] and np.abs(emb - ref["emb"]["f64"]).max() <= ref["emb"]["tol"]
    assert np.abs(alone_f - ref["feat"]["f64"][4:64]).max() <= ref["feat"]["tol"] and np.abs(alone_e - ref["emb"]["f64"][1:16]).max() <= ref["emb"]["tol"]


def test_a_bf16_checkpoint_computes_what_its_widened_values_compute():
    case, w, px, _ = _case("R")
    from oar_ocr_amd.synth.lm_reference import bf16_bits_to_f32, to_bf16_bits
    bits = {k: to_bf16_bits(v) for k, v in w.items()}
    wide = {k: bf16_bits_to_f32(v).reshape(w[k].shape) for k, v in bits.items()}
    with vl.VisionEncoder.from_state_dict(_cfg(case), bits) as e16, vl.VisionEncoder.from_state_dict(_cfg(case), wide) as e32:
        assert e16.encode(px, case.grids).tobytes() == e32.encode(px, case.grids).tobytes()


def test_bad_requests_are_refused_and_the_model_still_works():
    case, w, px, ref = _case("R")
    with vl.VisionEncoder.from_state_dict(_cfg(case), w) as enc:
        for grids, n in (([(4, 8), (6, 6), (4, 4), (2, 2)], 88), ([(3, 8)], 24), ([(4, 8), (6, 6), (4, 6)], 92), ([], 0)):   # too many images, merge, max_tokens, none
            with pytest.raises(api.OCRError) as e:
                enc.encode(np.zeros((n, 12), np.float32), grids)
            assert e.value.code == api.OAR_INVALID_INPUT, (grids, e.value.code)
        emb = enc.encode(px, case.grids)
    assert np.abs(emb - ref["emb"]["f64"]).max() <= ref["emb"]["tol"]


def test_the_erf_gelu_stays_in_the_linears_epilogue():
    """hidden_act = "gelu": the erf form runs in fc1's epilogue, 7 launches per layer, and the result is within tol of the reference with that activation"""
    import dataclasses
    case = dataclasses.replace(vr.ENCODER_CASES["R"], act="gelu")
    w, px = vr.make_vision(case), vr.make_pixels(case)
    ref = vr.vision_bundle(case, w, px)
    with vl.VisionEncoder.from_state_dict(_cfg(case), w) as enc:
        emb, feat = enc.encode(px, case.grids, return_features=True)
        assert enc.cost(case.grids)[2] == 7 * case.L + 7
    for key, got in (("feat", feat), ("emb", emb)):
        err = float(np.abs(got - ref[key]["f64"]).max())
        print(f"case R erf {key}: noise {ref[key]['noise']:.2e} tol {ref[key]['tol']:.2e} err {err:.2e}")
        assert err <= ref[key]["tol"], (key, err, ref[key]["tol"])
    assert np.abs(ref["feat"]["f64"] - _case("R")[3]["feat"]["f64"]).max() > 0          # (not the tanh case again)


def test_images_to_tokens_matches_the_composite_reference():
    """composite case PA: two u8 images through preprocess_images, the encoder, the projector and the decoder (vl.PaddleOCRVL.generate_tokens); the tokens of 24
    free-running steps are the f64 reference's and every step's logits are within the end-to-end tol"""
    r = vr.composite_reference()
    vc, lc = r["vis_case"], r["lm_case"]
    cfg_json = dict(hidden_size=lc.D, num_hidden_layers=lc.L, num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, head_dim=lc.head_dim, intermediate_size=lc.F,
                    vocab_size=lc.vocab, rms_norm_eps=lc.eps, rope_theta=lc.theta, rope_scaling=dict(mrope_section=list(lc.mrope_section)), tie_word_embeddings=lc.tie,
                    image_token_id=vr.PA_IDS["image"], vision_start_token_id=vr.PA_IDS["start"],
                    vision_config=dict(hidden_size=vc.D, num_hidden_layers=vc.L, num_attention_heads=vc.heads, intermediate_size=vc.F, patch_size=vc.patch, image_size=vc.G * vc.patch,
                                       spatial_merge_size=vc.merge, layer_norm_eps=vc.eps, hidden_act=vc.act))
    preproc = dict(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096, rescale_factor=1.0 / 255.0, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    with vl.PaddleOCRVL.from_state_dict(cfg_json, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=2), vision_overrides=dict(max_tokens=64, max_images=2)) as m:
        out = m.generate_tokens(r["images"], vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=vr.PA_STEPS, return_logits=True)
        again = m.generate_tokens(r["images"], vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=vr.PA_STEPS, return_logits=True)
    assert out.tokens.shape == (2, vr.PA_STEPS) and out.logits.tobytes() == again.logits.tobytes()
    for i, (t64, l64, _, _) in enumerate(r["runs"]):
        err = float(np.abs(out.logits[i].astype(np.float64) - l64).max())
        print(f"PA sequence {i}: noise {r['noise']:.2e} tol {r['tol']:.2e} logit err {err:.2e}, least margin {r['margins'][i].min() / r['tol']:.1f} tol")
        assert np.array_equal(out.tokens[i], t64) and err <= r["tol"], (i, err, r["tol"])


def test_preprocess_images_resizes_to_the_expected_grids():
    """12 x 19 rounds to 12 x 20 and 13 x 22 to 12 x 24 (factor 4): the resize is the library's exact resize kernel; a constant image stays constant through CatmullRom"""
    cfg = vl.ImageProcessorConfig(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096)
    img = np.random.default_rng(1).integers(0, 256, (12, 19, 3), dtype=np.uint8)
    px, grids = vl.preprocess_images([img, np.full((13, 22, 3), 200, np.uint8)], cfg)
    assert grids.tolist() == [[6, 10], [6, 12]] and px.shape == (60 + 72, 12) and np.isfinite(px).all()
    assert np.array_equal(px[60:], np.full((72, 12), (np.float32(200) * np.float32(1 / 255) - np.float32(0.5)) / np.float32(0.5), np.float32))
    assert px[:60].min() >= -1.0 and px[:60].max() <= 1.0 and px[:60].std() > 0.3


def test_pos_embed_returns_the_table_bit_for_bit_at_its_own_size():
    """vis_pos_embed alone (api.k_vis_pos_embed): three images in one launch, the middle one at h = w = G, whose rows must be the table's bytes; the others within tol of
    the f64 resampling (noise = max |f32 - f64| of the reference's own resampling); the guard words around the output come back untouched"""
    import torch
    G, D, grids, guard = 4, 24, [(4, 8), (4, 4), (6, 6)], 64
    table = np.random.default_rng(8).standard_normal((G * G, D)).astype(np.float32)
    T = sum(h * w for h, w in grids)
    sentinel = np.uint32(0x7FA5C3E1)
    o_io = np.full(guard + T * D + guard, sentinel, np.uint32).view(np.float32)
    out = api.k_vis_pos_embed(table, G, grids, o_io, guard)
    bits = out.view(np.uint32)
    assert (bits[:guard] == sentinel).all() and (bits[guard + T * D:] == sentinel).all() and not (bits[guard:guard + T * D] == sentinel).any()
    o = out[guard:guard + T * D].reshape(T, D)
    assert o[32:48].tobytes() == table.tobytes()
    r64 = torch.cat([vr.resample_table(torch.from_numpy(table).double(), G, h, w) for h, w in grids]).numpy()
    r32 = torch.cat([vr.resample_table(torch.from_numpy(table), G, h, w) for h, w in grids]).numpy()
    noise = float(np.abs(r32 - r64).max())
    tol, err = max(16 * noise, 2.0 ** -19), float(np.abs(o - r64).max())
    print(f"vis_pos_embed: noise {noise:.2e} tol {tol:.2e} err {err:.2e}")
    assert err <= tol
    assert api.k_vis_pos_embed(table, G, grids, o_io, guard).tobytes() == out.tobytes()


def test_the_profiler_tells_the_vision_stage_apart():
    """one encode of case P under the profiler: the launches are in the classes vis_embed, vis_linear, vis_layernorm, vis_attention and vis_project and in no other, and
    they add up to what oar_vis_cost reports"""
    case, w, px, _ = _case("P")
    with vl.VisionEncoder.from_state_dict(_cfg(case), w) as enc:
        enc.encode(px, case.grids)
        api.prof_reset()
        api.prof_enable(True)
        try:
            enc.encode(px, case.grids)
            snap = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["launches"]}   # (classes other tests of the process registered stay listed, with 0)
        finally:
            api.prof_enable(False)
        launches = enc.cost(case.grids)[2]
    print(snap)
    L = case.L
    assert snap == {"vis_embed": 1, "vis_linear": 1 + 5 * L + 2, "vis_layernorm": 2 * L + 2, "vis_attention": L, "vis_project": 1}, snap   # (the tanh GELU counts with fc1)
    assert sum(snap.values()) == launches
