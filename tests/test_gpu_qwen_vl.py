"""Images to tokens through the Qwen towers (vl.QwenVL.generate_tokens): composite MA (the qwen2 tower) and NA (the windowed qwen2_5 tower), each
in front of a small Qwen2-style decoder with q / k / v biases and an M-RoPE section; three u8 images, a prefix and a suffix of a few ids.  The tokens of 24
free-running steps are the f64 reference's (whose margins tests/test_qwen_vision_reference_cpu.py holds above 2 tol), the logits under the reference's tokens are
within tol, the GEMM prefill with split-key decode attention gives the same tokens, and MA with no_repeat_ngram_size = 3 follows the f64 run with the ban."""
import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import qwen_vision_reference as qr

pytestmark = pytest.mark.gpu


def _json(r):
    vc, lc = r["vis_case"], r["lm_case"]
    vision = dict(depth=vc.L, num_heads=vc.heads, in_chans=vc.channels, patch_size=vc.patch, spatial_merge_size=vc.merge, temporal_patch_size=vc.temporal, hidden_act=vc.act)
    if vc.kind == "qwen2_5":
        vision.update(hidden_size=vc.D, out_hidden_size=vc.out_hidden, intermediate_size=vc.F, window_size=vc.window_size, fullatt_block_indexes=list(vc.fullatt))
    else:
        vision.update(embed_dim=vc.D, hidden_size=vc.out_hidden, mlp_ratio=vc.F / vc.D)
    # (no attention_bias key: a Qwen2 config.json does not say that q / k / v have biases, QwenVL must know)
    cfg = dict(hidden_size=lc.D, num_hidden_layers=lc.L, num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, head_dim=lc.head_dim, intermediate_size=lc.F,
               vocab_size=lc.vocab, rms_norm_eps=lc.eps, rope_theta=lc.theta, rope_scaling=dict(mrope_section=list(lc.mrope_section)), tie_word_embeddings=lc.tie,
               image_token_id=qr.COMPOSITE_IDS["image"], vision_start_token_id=qr.COMPOSITE_IDS["start"], vision_config=vision)
    preproc = dict(patch_size=vc.patch, merge_size=vc.merge, temporal_patch_size=vc.temporal, min_pixels=16, max_pixels=4096, rescale_factor=1.0 / 255.0,
                   image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    return cfg, preproc


@pytest.fixture(scope="module", params=list(qr.COMPOSITES))
def composite(request):
    r = qr.composite_reference(request.param)
    cfg, preproc = _json(r)
    with vl.QwenVL.from_state_dict(cfg, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=3), vision_overrides=dict(max_tokens=160, max_images=3)) as m:
        yield request.param, r, m


def test_the_configuration_is_read_as_the_reference_reads_it(composite):
    name, r, m = composite
    vc = r["vis_case"]
    assert m.lm.cfg.qkv_bias and m.vision.cfg.kind == vc.kind and m.vision.cfg.intermediate_size == vc.F and m.vision.cfg.out_hidden_size == vc.out_hidden
    assert m.generation_defaults == {}


def test_images_to_tokens_match_the_f64_reference(composite):
    name, r, m = composite
    ids = qr.COMPOSITE_IDS
    out = m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=qr.COMPOSITE_STEPS, return_logits=True)
    again = m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=qr.COMPOSITE_STEPS, return_logits=True)
    forced = m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=qr.COMPOSITE_STEPS, return_logits=True, forced_tokens=[t for t, _, _, _ in r["runs"]])
    fast = m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=qr.COMPOSITE_STEPS, prefill="gemm", decode_attention="split")
    assert out.tokens.shape == (3, qr.COMPOSITE_STEPS) and out.logits.tobytes() == again.logits.tobytes()
    for i, (t64, l64, _, _) in enumerate(r["runs"]):
        err = float(np.abs(forced.logits[i].astype(np.float64) - l64).max())
        print(f"{name} sequence {i}: noise {r['noise']:.2e} tol {r['tol']:.2e} logit err {err:.2e}, least margin {r['margins'][i].min() / r['tol']:.1f} tol")
        assert np.array_equal(out.tokens[i], t64), (name, i)
        assert np.isfinite(forced.logits[i]).all() and err <= r["tol"], (name, i, err, r["tol"])
        assert np.array_equal(fast.tokens[i], t64), (name, i, "gemm prefill, split decode attention")


def test_no_repeat_ngram_follows_the_f64_run_with_the_ban():
    """MA with no_repeat_ngram_size = 3 (the reference's margins there exceed 4 r tol, and the ban changes every sequence)"""
    r = qr.composite_reference("MA")
    cfg, preproc = _json(r)
    ids = qr.COMPOSITE_IDS
    with vl.QwenVL.from_state_dict(cfg, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=3), vision_overrides=dict(max_tokens=160, max_images=3)) as m:
        out = m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=qr.COMPOSITE_STEPS, no_repeat_ngram_size=qr.COMPOSITE_NGRAM)
    plain = [t for t, _, _, _ in r["runs"]]
    for i, g in enumerate(r["ngram_runs"]):
        assert np.array_equal(out.tokens[i], g["tokens"]), (i, out.tokens[i], g["tokens"])
        assert not np.array_equal(g["tokens"], plain[i])                       # the ban changed the sequence


def test_the_refill_schedule_refuses_the_processors(composite):
    name, r, m = composite
    ids = qr.COMPOSITE_IDS
    with pytest.raises(api.OCRError) as e:
        m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=4, schedule="refill", no_repeat_ngram_size=3)
    assert e.value.code == api.OAR_UNSUPPORTED_OP
    out = m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=qr.COMPOSITE_STEPS, schedule="refill", slots=2)
    for i, (t64, _, _, _) in enumerate(r["runs"]):
        assert np.array_equal(out.tokens[i], t64), (name, i)
