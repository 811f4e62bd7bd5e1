"""vl.CausalLM with prefill="gemm" (lm_prefill_gemm.hip, lm_prefill_attn.hip, then the decode chain) against the f64 torch reference of
synth/lm_reference.py: teacher-forced logits within tol = max(16 noise, 2^-19) and exact tokens on every case of tests/test_gpu_lm_decode.py and
tests/test_gpu_lm_paths.py, prompts at the edges of the attention kernel's 64-query tiles (synth/lm_prefill_cases.py), and the properties the path promises: logits do
not depend on the other sequences of the call or on chunk_rows, two runs give the same bytes, bf16 tables equal their widened values, one-position prompts equal the
rows prefill bit for bit, and a rows call after a GEMM call equals a fresh model's."""
import ctypes as C

import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_prefill_cases as P
from oar_ocr_amd.synth import lm_reference as R
from oar_ocr_amd.synth import vision_reference as vr

pytestmark = pytest.mark.gpu

MAX_POS = 64


def _cfg(case, **kw):
    d = dict(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, num_key_value_heads=case.kv_heads, head_dim=case.head_dim, intermediate_size=case.F,
             vocab_size=case.vocab, rms_norm_eps=case.eps, rope_theta=case.theta, mrope_section=list(case.mrope_section), qkv_bias=case.qkv_bias, tie_word_embeddings=case.tie,
             max_positions=MAX_POS, max_sequences=16)
    d.update(kw)
    return vl.CausalLMConfig(**d)


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        ref = R.reference_for(name)
        _MODELS[name] = vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"])
    return _MODELS[name]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()


def _gemm_launches():
    return sum(e["launches"] for e in api.prof_snapshot() if e["name"].startswith("lm_gemm_"))


@pytest.mark.parametrize("name", list(R.CASES))
def test_teacher_forced_logits_are_within_the_f32_noise_of_f64(name):
    """Prompts of 1, 17 and 37 positions in one call: 0 + 16 + 36 GEMM rows, then the handover step with the three last positions and 19 decode steps."""
    ref = R.reference_for(name)
    lm = _model(name)
    n = R.TEACHER_STEPS
    out = lm.generate(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=n, return_logits=True,
                      forced_tokens=[t[:n] for t, _ in ref["runs"]], prefill="gemm")
    err = max(float(np.abs(out.logits[i].astype(np.float64) - l64[:n].numpy()).max()) for i, (_, l64) in enumerate(ref["runs"]))
    print(f"gemm prefill case {name}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} error {err:.3e} ({err / ref['tol']:.3f} tol)")
    assert np.isfinite(out.logits).all() and err <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64[:n])


@pytest.mark.parametrize("name", list(R.LONG_CASES))
def test_long_prompt_logits_are_within_the_f32_noise_of_f64(name):
    """T - 1 = 121, 505 or 249 GEMM rows (57 past a multiple of 64) and a one-position mate with none, in a cache of exactly T + LONG_STEPS positions."""
    ref = R.long_reference_for(name)
    case, T, n = ref["case"], ref["T"], R.LONG_STEPS
    emb, pos, forced = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]], [t for t, _ in ref["runs"]]
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=T + n, max_sequences=2), ref["weights"]) as lm:
        out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, forced_tokens=forced, prefill="gemm")
    errs = [float(np.abs(out.logits[i].astype(np.float64) - l64.numpy()).max()) for i, (_, l64) in enumerate(ref["runs"])]
    print(f"gemm prefill case {name} T={T}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} error {errs[0]:.3e} ({errs[0] / ref['tol']:.3f} tol), mate {errs[1]:.3e} ({errs[1] / ref['tol']:.3f} tol)")
    assert np.isfinite(out.logits).all() and max(errs) <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64), (name, i, out.tokens[i], t64)


@pytest.mark.parametrize("name", list(P.EDGE_CASES))
def test_prompts_at_the_edges_of_the_query_tiles(name):
    """Prompts of 64, 65, 66 and 129 positions in one call: 63, 64, 65 and 128 GEMM rows, 4 forced steps."""
    ref = P.edge_reference_for(name)
    case, n = ref["case"], P.EDGE_STEPS
    emb, pos, forced = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]], [t for t, _ in ref["runs"]]
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=max(P.EDGE_LENGTHS) + n, max_sequences=4), ref["weights"]) as lm:
        out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, forced_tokens=forced, prefill="gemm")
    errs = [float(np.abs(out.logits[i].astype(np.float64) - l64.numpy()).max()) for i, (_, l64) in enumerate(ref["runs"])]
    print(f"gemm prefill edge case {name}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} errors " + " ".join(f"{e:.3e} ({e / ref['tol']:.3f} tol)" for e in errs))
    assert np.isfinite(out.logits).all() and max(errs) <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64), (name, i, out.tokens[i], t64)


def test_a_sequence_does_not_depend_on_the_other_sequences_of_the_call():
    """Case A's 37-position prompt alone, as the first of 16 different sequences and as the last of them: tokens and logits bitwise equal."""
    ref = R.reference_for("A")
    case, weights = ref["case"], ref["weights"]
    lm = _model("A")
    emb, pos, _ = ref["prompts"][2]
    others = [R.make_prompt(case, weights, T, 50 + i) for i, T in enumerate([1, 3, 37, 16, 17, 2, 15, 33, 5, 18, 31, 4, 20, 9, 12])]
    n = 12
    alone = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, prefill="gemm")
    first = lm.generate(inputs_embeds=[emb] + [o[0] for o in others], position_ids=[pos] + [o[1] for o in others], max_new_tokens=n, return_logits=True, prefill="gemm")
    last = lm.generate(inputs_embeds=[o[0] for o in others] + [emb], position_ids=[o[1] for o in others] + [pos], max_new_tokens=n, return_logits=True, prefill="gemm")
    assert np.array_equal(alone.tokens, ref["runs"][2][0][:n])
    for got, slot in ((first, 0), (last, 15)):
        assert np.array_equal(got.tokens[slot], alone.tokens)
        assert got.logits[slot].tobytes() == alone.logits.tobytes(), slot
    assert not np.array_equal(first.tokens[1], first.tokens[0])


CHUNKS = (1, 16, 40, 64, 100, None)


def _chunk_runs(lm, emb, pos, n, L):
    outs = []
    api.prof_enable(True)
    try:
        for chunk in CHUNKS:
            api.prof_reset()
            outs.append(lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, prefill="gemm", prefill_chunk=chunk))
            launches = _gemm_launches()
            flops, nbytes, want = lm.prefill_cost([e.shape[0] for e in emb])
            rows = sum(e.shape[0] - 1 for e in emb)
            chunks = -(-rows // (chunk or 2048))
            assert launches == want == chunks * (5 * (L - 1) + 1), (chunk, launches, want)
            assert flops > 0 and nbytes > 0
    finally:
        api.prof_enable(False)
    return outs


def test_logits_do_not_depend_on_chunk_rows_case_a():
    """Case A's three prompts (52 GEMM rows) in chunks of 1, 16, 40, 64, 100 and the default: logits bitwise equal; the lm_gemm_* launches are prefill_cost's."""
    ref = R.reference_for("A")
    outs = _chunk_runs(_model("A"), [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]], 8, ref["case"].L)
    for o in outs[1:]:
        assert o.logits.tobytes() == outs[0].logits.tobytes() and np.array_equal(o.tokens, outs[0].tokens)
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(outs[0].tokens[i], t64[:8])


def test_logits_do_not_depend_on_chunk_rows_case_lc():
    """LC's 506-position prompt (505 GEMM rows: eight tiles, chunks that cut them at every offset) with its one-position mate."""
    ref = R.long_reference_for("LC")
    case, T, n = ref["case"], ref["T"], 4
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=T + n, max_sequences=2), ref["weights"]) as lm:
        outs = _chunk_runs(lm, [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]], n, case.L)
    for o in outs[1:]:
        assert o.logits.tobytes() == outs[0].logits.tobytes() and np.array_equal(o.tokens, outs[0].tokens)
    assert np.array_equal(outs[0].tokens[0], ref["runs"][0][0][:n])


@pytest.mark.parametrize("name", ["E", "V"])
def test_bf16_tables_equal_the_same_values_widened_to_f32(name):
    ref = R.reference_for(name)
    case, weights = ref["case"], ref["weights"]
    bits = {k: R.to_bf16_bits(v) for k, v in weights.items()}
    wide = {k: R.bf16_bits_to_f32(v) for k, v in bits.items()}
    emb, pos = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]]
    with vl.CausalLM.from_state_dict(_cfg(case), bits) as m16, vl.CausalLM.from_state_dict(_cfg(case), wide) as m32:
        a = m16.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True, prefill="gemm")
        b = m32.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True, prefill="gemm")
        c = m16.generate(input_ids=[3, 1, 4, 1, 5], max_new_tokens=6, return_logits=True, prefill="gemm")
        d = m32.generate(input_ids=[3, 1, 4, 1, 5], max_new_tokens=6, return_logits=True, prefill="gemm")
        assert m32.prefill_cost([17, 37])[1] > m16.prefill_cost([17, 37])[1]          # the weight stream is counted at two bytes an element
    assert a.logits.tobytes() == b.logits.tobytes() and np.array_equal(a.tokens, b.tokens)
    assert c.logits.tobytes() == d.logits.tobytes() and np.array_equal(c.tokens, d.tokens)
    assert float(np.abs(a.logits - _model(name).generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True, prefill="gemm").logits).max()) > 1e-3


def test_two_runs_give_identical_bytes():
    ref = R.reference_for("B")
    lm = _model("B")
    kw = dict(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=12, return_logits=True, prefill="gemm")
    a, b = lm.generate(**kw), lm.generate(**kw)
    assert a.logits.tobytes() == b.logits.tobytes() and a.tokens.tobytes() == b.tokens.tobytes()


def test_one_position_prompts_equal_the_rows_prefill_bit_for_bit():
    """With every prompt of length 1 the GEMM phase launches nothing and the call is the rows call."""
    lm = _model("A")
    ids = [[5], [11], [96], [0]]
    api.prof_reset()
    api.prof_enable(True)
    try:
        g = lm.generate(input_ids=ids, max_new_tokens=9, return_logits=True, prefill="gemm")
        assert _gemm_launches() == 0 and lm.prefill_cost([1, 1, 1, 1]) == (0.0, 0.0, 0)
    finally:
        api.prof_enable(False)
    r = lm.generate(input_ids=ids, max_new_tokens=9, return_logits=True, prefill="rows")
    assert g.logits.tobytes() == r.logits.tobytes() and g.tokens.tobytes() == r.tokens.tobytes()


def test_eos_ends_one_sequence_and_the_other_keeps_going():
    ref = R.reference_for("A")
    lm = _model("A")
    t17, t37 = ref["runs"][1][0], ref["runs"][2][0]
    eos = int(t17[5])
    assert eos not in t17[:5]
    out = lm.generate(inputs_embeds=[ref["prompts"][1][0], ref["prompts"][2][0]], position_ids=[ref["prompts"][1][1], ref["prompts"][2][1]], max_new_tokens=R.FREE_STEPS,
                      eos_token_id=eos, prefill="gemm")
    assert out.counts[0] == 6 and np.array_equal(out.tokens[0, :6], t17[:6]) and (out.tokens[0, 6:] == eos).all()
    stop = np.flatnonzero(t37 == eos)
    n37 = int(stop[0]) + 1 if len(stop) else R.FREE_STEPS
    assert n37 > 6 and out.counts[1] == n37 and np.array_equal(out.tokens[1, :n37], t37[:n37])


def test_a_rows_call_after_a_gemm_call_equals_a_fresh_models():
    ref = R.reference_for("A")
    emb, pos = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]]
    with vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"]) as used, vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"]) as fresh:
        g = used.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True, prefill="gemm", prefill_chunk=16)
        a = used.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)               # (the default is the rows prefill)
        b = fresh.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)
        api.prof_reset()
        api.prof_enable(True)
        try:
            used.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=2)
            assert _gemm_launches() == 0
        finally:
            api.prof_enable(False)
    assert a.logits.tobytes() == b.logits.tobytes() and a.tokens.tobytes() == b.tokens.tobytes()
    assert np.array_equal(g.tokens, a.tokens) and g.logits.tobytes() != a.logits.tobytes()                                # (another sum order: the same tokens, other last bits)


def test_set_prefill_rejects_what_it_does_not_know():
    lm = _model("A")
    L = vl._lib()
    assert L.oar_lm_set_prefill(lm._h, 2, 0) == api.OAR_INVALID_INPUT
    assert L.oar_lm_set_prefill(lm._h, -1, 0) == api.OAR_INVALID_INPUT
    assert L.oar_lm_set_prefill(lm._h, 1, -1) == api.OAR_INVALID_INPUT
    assert L.oar_lm_set_prefill(lm._h, 1, 65537) == api.OAR_INVALID_INPUT
    assert L.oar_lm_set_prefill(None, 1, 0) == api.OAR_INVALID_INPUT
    assert L.oar_lm_set_prefill(lm._h, 1, 65536) == api.OAR_OK and L.oar_lm_set_prefill(lm._h, 0, 0) == api.OAR_OK
    with pytest.raises(api.OCRError) as e:
        lm.generate(input_ids=[1, 2, 3], max_new_tokens=2, prefill="matmul")
    assert e.value.code == api.OAR_INVALID_INPUT
    with pytest.raises(api.OCRError) as e:
        lm.generate(input_ids=[1, 2, 3], max_new_tokens=2, prefill="gemm", prefill_chunk=-1)
    assert e.value.code == api.OAR_INVALID_INPUT
    f, b, n = C.c_double(), C.c_double(), C.c_int32()
    assert L.oar_lm_prefill_cost(lm._h, 0, None, C.byref(f), C.byref(b), C.byref(n)) == api.OAR_INVALID_INPUT


def test_images_to_tokens_with_gemm_prefill_matches_the_composite_reference():
    """composite case PA through vl.PaddleOCRVL.generate_tokens(..., prefill="gemm"): the tokens of all 24 free-running steps are the f64 reference's"""
    r = vr.composite_reference()
    vc, lc = r["vis_case"], r["lm_case"]
    cfg_json = dict(hidden_size=lc.D, num_hidden_layers=lc.L, num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, head_dim=lc.head_dim, intermediate_size=lc.F,
                    vocab_size=lc.vocab, rms_norm_eps=lc.eps, rope_theta=lc.theta, rope_scaling=dict(mrope_section=list(lc.mrope_section)), tie_word_embeddings=lc.tie,
                    image_token_id=vr.PA_IDS["image"], vision_start_token_id=vr.PA_IDS["start"],
                    vision_config=dict(hidden_size=vc.D, num_hidden_layers=vc.L, num_attention_heads=vc.heads, intermediate_size=vc.F, patch_size=vc.patch, image_size=vc.G * vc.patch,
                                       spatial_merge_size=vc.merge, layer_norm_eps=vc.eps, hidden_act=vc.act))
    preproc = dict(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096, rescale_factor=1.0 / 255.0, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    with vl.PaddleOCRVL.from_state_dict(cfg_json, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=2), vision_overrides=dict(max_tokens=64, max_images=2)) as m:
        api.prof_reset()
        api.prof_enable(True)
        try:
            out = m.generate_tokens(r["images"], vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=vr.PA_STEPS, return_logits=True, prefill="gemm")
            assert _gemm_launches() > 0
        finally:
            api.prof_enable(False)
    assert out.tokens.shape == (2, vr.PA_STEPS)
    for i, (t64, l64, _, _) in enumerate(r["runs"]):
        err = float(np.abs(out.logits[i].astype(np.float64) - l64).max())
        print(f"PA sequence {i} with gemm prefill: noise {r['noise']:.2e} tol {r['tol']:.2e} logit err {err:.2e}")
        assert np.array_equal(out.tokens[i], t64) and err <= r["tol"], (i, err, r["tol"])
