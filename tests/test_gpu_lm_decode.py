"""vl.CausalLM (lm_decode.hip) against the f64 torch reference (synth/lm_reference.py): teacher-forced logits within the reference's own f32 noise, exact greedy tokens
on greedy-safe seeds, and the two properties the kernels promise -- a row's result does not depend on the rows it shares a step with, and two runs give the same bytes.

Cases A-D, E-H (3, 7, 8 and 12 query heads per kv head, idle lanes), V and W (several row groups per workgroup) and why they are what they are: synth/lm_reference.py
CASES; long caches, equal maxima and the end of generation: tests/test_gpu_lm_paths.py.  Case D runs as specified: the rows kernels stage 1024 columns at a time (not 768), and D = 1544 /
F = 1540 are still above one staging chunk and no multiples of it."""
import ctypes as C

import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_reference as R

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


@pytest.mark.parametrize("name", list(R.CASES))
def test_teacher_forced_logits_are_within_the_f32_noise_of_f64(name):
    """Three sequences (prompts of 1, 17 and 37 positions, the image block in the middle of the longer two) in one call, 20 steps forced to the f64 tokens: every
    logit within tol = max(16 noise, 2^-19), noise = max |f32 - f64| of the reference itself."""
    ref = R.reference_for(name)
    lm = _model(name)
    n = R.TEACHER_STEPS
    out = lm.generate(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=n, return_logits=True,
                      forced_tokens=[t[:n] for t, _ in ref["runs"]])
    err = max(float(np.abs(out.logits[i].astype(np.float64) - l64[:n].numpy()).max()) for i, (_, l64) in enumerate(ref["runs"]))
    print(f"case {name}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} error {err:.3e} ({err / ref['tol']:.3f} tol)")
    assert np.isfinite(out.logits).all() and err <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64[:n])


@pytest.mark.parametrize("name", list(R.CASES))
def test_free_running_tokens_equal_the_f64_reference(name):
    ref = R.reference_for(name)
    lm = _model(name)
    out = lm.generate(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=R.FREE_STEPS)
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64), (name, i, out.tokens[i], t64)
    assert out.counts.tolist() == [R.FREE_STEPS] * 3


def test_eos_ends_one_sequence_and_the_other_keeps_going():
    ref = R.reference_for("A")
    lm = _model("A")
    t17, t37 = ref["runs"][1][0], ref["runs"][2][0]
    eos = int(t17[5])
    assert eos not in t17[:5]
    out = lm.generate(inputs_embeds=[ref["prompts"][1][0], ref["prompts"][2][0]], position_ids=[ref["prompts"][1][1], ref["prompts"][2][1]], max_new_tokens=R.FREE_STEPS,
                      eos_token_id=eos)
    assert out.counts[0] == 6 and np.array_equal(out.tokens[0, :6], t17[:6]) and (out.tokens[0, 6:] == eos).all()
    stop = np.flatnonzero(t37 == eos)
    n37 = int(stop[0]) + 1 if len(stop) else R.FREE_STEPS
    assert n37 > 6 and out.counts[1] == n37 and np.array_equal(out.tokens[1, :n37], t37[:n37])


def test_a_row_does_not_depend_on_its_step_mates_or_its_slot():
    """Sequence 0 alone, as the first of 16 different sequences, and as the last of them (slot 15): tokens and logits bitwise equal."""
    ref = R.reference_for("A")
    case, weights = ref["case"], ref["weights"]
    lm = _model("A")
    emb, pos, _ = ref["prompts"][1]
    others = [R.make_prompt(case, weights, T, 50 + i) for i, T in enumerate([1, 3, 37, 16, 17, 2, 15, 33, 5, 18, 31, 4, 20, 9, 12])]
    n = 12
    alone = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True)
    first = lm.generate(inputs_embeds=[emb] + [o[0] for o in others], position_ids=[pos] + [o[1] for o in others], max_new_tokens=n, return_logits=True)
    last = lm.generate(inputs_embeds=[o[0] for o in others] + [emb], position_ids=[o[1] for o in others] + [pos], max_new_tokens=n, return_logits=True)
    assert np.array_equal(alone.tokens, ref["runs"][1][0][:n])
    for got, slot in ((first, 0), (last, 15)):
        assert np.array_equal(got.tokens[slot], alone.tokens)
        assert got.logits[slot].tobytes() == alone.logits.tobytes(), slot
    assert not np.array_equal(first.tokens[1], first.tokens[0])


def test_prefill_in_chunks_equals_one_position_at_a_time():
    """A 37-token prompt prefilled in chunks of 16 against the same tokens fed one by one (a 1-token prompt, the other 36 forced): logits bitwise equal."""
    ref = R.reference_for("A")
    lm = _model("A")
    ids = np.random.default_rng(7).integers(0, ref["case"].vocab, 37).astype(np.int32)
    n = 8
    a = lm.generate(input_ids=ids, max_new_tokens=n, return_logits=True)
    forced = np.concatenate([ids[1:], a.tokens[:n - 1]])
    b = lm.generate(input_ids=ids[:1], max_new_tokens=36 + n, return_logits=True, forced_tokens=forced)
    assert b.logits[36:].tobytes() == a.logits.tobytes()
    assert np.array_equal(b.tokens[36:], a.tokens)


def test_bf16_tables_equal_the_same_values_widened_to_f32():
    ref = R.reference_for("A")
    case, weights = ref["case"], ref["weights"]
    bits = {k: R.to_bf16_bits(v) for k, v in weights.items()}
    wide = {k: R.bf16_bits_to_f32(v) for k, v in bits.items()}
    emb, pos = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]]
    with vl.CausalLM.from_state_dict(_cfg(case), bits) as m16, vl.CausalLM.from_state_dict(_cfg(case), wide) as m32:
        a = m16.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)
        b = m32.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)
        c = m16.generate(input_ids=[3, 1, 4, 1, 5], max_new_tokens=6, return_logits=True)      # (the embedding gather reads the bf16 table)
        d = m32.generate(input_ids=[3, 1, 4, 1, 5], max_new_tokens=6, return_logits=True)
        c_ = case
        matrices = c_.L * (c_.D * (c_.heads + 2 * c_.kv_heads) * c_.head_dim + c_.heads * c_.head_dim * c_.D + 3 * c_.F * c_.D) + c_.vocab * c_.D
        assert m32.cost(16, 32)[1] - m16.cost(16, 32)[1] >= 2.0 * matrices          # the weight stream is counted at two bytes an element
    assert a.logits.tobytes() == b.logits.tobytes() and np.array_equal(a.tokens, b.tokens)
    assert c.logits.tobytes() == d.logits.tobytes() and np.array_equal(c.tokens, d.tokens)
    assert float(np.abs(a.logits - _model("A").generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True).logits).max()) > 1e-3   # (rounding did change the model)


def test_cache_bounds_and_the_logits_buffer():
    ref = R.reference_for("A")
    case = ref["case"]
    emb, pos, _ = ref["prompts"][1]
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=40), ref["weights"]) as lm:
        need = 23 * case.vocab
        buf = np.full(need + 256, np.float32(-777.25), np.float32)
        out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=23, logits_out=buf)       # 17 + 23 = 40: the cache is exactly full
        assert (buf[need:] == np.float32(-777.25)).all() and np.isfinite(buf[:need]).all()
        assert np.array_equal(out.tokens, ref["runs"][1][0][:23])
        api.prof_reset()
        api.prof_enable(True)
        try:
            with pytest.raises(api.OCRError) as e:
                lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=24)
            assert e.value.code == api.OAR_INVALID_INPUT and "max_positions" in str(e.value)
            assert not [s for s in api.prof_snapshot() if s["name"].startswith("lm_") and s["launches"]]
        finally:
            api.prof_enable(False)


def test_two_runs_give_identical_bytes():
    ref = R.reference_for("B")
    lm = _model("B")
    kw = dict(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=12, return_logits=True)
    a, b = lm.generate(**kw), lm.generate(**kw)
    assert a.logits.tobytes() == b.logits.tobytes() and a.tokens.tobytes() == b.tokens.tobytes()


def test_launch_count_and_classes():
    """A decode step is 5 L + 2 launches: 4 L lm_rows, L lm_attn, one lm_head, one lm_combine.  A 1-token prompt given as an id costs one lm_embed launch and its
    prefill step is a step like any other, so max_new tokens take max_new steps."""
    ref = R.reference_for("A")
    lm = _model("A")
    L, n = ref["case"].L, 5
    api.prof_reset()
    api.prof_enable(True)
    try:
        lm.generate(input_ids=[11], max_new_tokens=n)
        snap = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["name"].startswith("lm_")}
    finally:
        api.prof_enable(False)
    assert snap == {"lm_rows": 4 * L * n, "lm_attn": L * n, "lm_head": n, "lm_combine": n, "lm_embed": 1}, snap
    assert sum(v for k, v in snap.items() if k != "lm_embed") == n * (5 * L + 2)
    flops, nbytes, launches = lm.cost(1, 8)
    c = ref["case"]
    weights = c.L * (c.D * (c.heads + 2 * c.kv_heads) * c.head_dim + c.heads * c.head_dim * c.D + 3 * c.F * c.D) + c.vocab * c.D
    assert launches == 5 * L + 2 and nbytes >= 4.0 * weights and flops >= 2.0 * weights


def test_rejected_arguments_launch_nothing():
    ref = R.reference_for("A")
    case, weights = ref["case"], ref["weights"]
    api.prof_reset()
    api.prof_enable(True)
    try:
        for kw, code in ((dict(head_dim=132, mrope_section=[22, 22, 22]), api.OAR_UNSUPPORTED_OP), (dict(head_dim=6, mrope_section=[1, 1, 1]), api.OAR_UNSUPPORTED_OP),
                         (dict(mrope_section=[2, 3, 2]), api.OAR_INVALID_INPUT), (dict(num_key_value_heads=3), api.OAR_INVALID_INPUT)):
            with pytest.raises(api.OCRError) as e:
                vl.CausalLM.from_state_dict(_cfg(case, **kw), weights)
            assert e.value.code == code, (kw, str(e.value))
        with pytest.raises(api.OCRError) as e:
            vl.CausalLM.from_state_dict(_cfg(case), {k: v for k, v in weights.items() if k != "model.norm.weight"})
        assert e.value.code == api.OAR_INVALID_INPUT and "model.norm.weight" in str(e.value)
        # 17 sequences at the C level (the Python class would split them into groups of 16)
        lm = _model("A")
        ids = np.zeros(1, np.int32)
        lengths = np.ones(17, np.int32)
        ptrs = (C.c_void_p * 17)(*[ids.ctypes.data] * 17)
        tokens, counts = np.zeros((17, 2), np.int32), np.zeros(17, np.int32)
        req = vl.LmRequest()
        req.n_seq, req.lengths, req.input_ids = 17, lengths.ctypes.data_as(C.POINTER(C.c_int32)), C.cast(ptrs, C.POINTER(C.c_void_p))
        req.max_new_tokens, req.eos_token_id, req.tokens, req.counts = 2, -1, tokens.ctypes.data, counts.ctypes.data
        assert vl._lib().oar_lm_generate(lm._h, C.byref(req)) == api.OAR_INVALID_INPUT
        with pytest.raises(api.OCRError) as e:
            lm.generate(input_ids=[case.vocab], max_new_tokens=2)
        assert e.value.code == api.OAR_INVALID_INPUT
        assert not [s for s in api.prof_snapshot() if s["name"].startswith("lm_") and s["launches"]]
    finally:
        api.prof_enable(False)
    out = lm.generate(input_ids=[[1, 2, 3]] * 18, max_new_tokens=3)      # the class runs 18 sequences as 16 + 2
    assert out.tokens.shape == (18, 3) and (out.tokens == out.tokens[0]).all()
