"""vl.CausalLM with decode_attention="split", split_keys=64 (lm_decode_split.hip in place of the chain's lm_attn launch) and stop_at_eos, against the f64 torch
reference of synth/lm_reference.py with its own noise / tol = max(16 noise, 2^-19): teacher-forced logits and exact tokens on short and long caches, and the properties
the mode promises: a sequence does not depend on its step mates, a prompt prefilled 16 rows a step equals one row a step bit for bit, the GEMM prefill's handover goes
through it, nothing depends on what the workspace held, cost() follows the mode, and a call that stops at eos returns the bytes of the call that does not."""
import ctypes as C

import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_reference as R
from oar_ocr_amd.synth import lm_split_cases as S

pytestmark = pytest.mark.gpu

MAX_POS = 64
SPLIT = dict(decode_attention="split", split_keys=64)


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


@pytest.mark.parametrize("name", ["A", "E", "F", "H"])
def test_teacher_forced_logits_are_within_the_f32_noise_of_f64(name):
    """A: G = 2; E: G = 8, head size 128; F: G = 7 (chunks of 4 and 3 heads); H: G = 12 (8 and 4), head size 8.  Prompts of 1, 17 and 37 positions, 20 forced steps."""
    ref = R.reference_for(name)
    lm = _model(name)
    n = R.TEACHER_STEPS
    out = lm.generate(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=n, return_logits=True,
                      forced_tokens=[t[:n] for t, _ in ref["runs"]], **SPLIT)
    err = max(float(np.abs(out.logits[i].astype(np.float64) - l64[:n].numpy()).max()) for i, (_, l64) in enumerate(ref["runs"]))
    print(f"split decode case {name}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} error {err:.3e} ({err / ref['tol']:.3f} tol)")
    assert np.isfinite(out.logits).all() and err <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64[:n])


@pytest.mark.parametrize("name", ["LA", "LC", "LD"])
def test_long_cache_logits_are_within_the_f32_noise_of_f64(name):
    """Prompts of 122, 506 and 250 positions with a one-position mate; the 12 forced steps cross 128, 512 and 256 keys: a new span opens under way."""
    ref = R.long_reference_for(name)
    case, T, n = ref["case"], ref["T"], R.LONG_STEPS
    emb, pos, forced = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]], [t for t, _ in ref["runs"]]
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=T + n, max_sequences=2), ref["weights"]) as lm:
        out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, forced_tokens=forced, **SPLIT)
        alone = lm.generate(inputs_embeds=emb[1], position_ids=pos[1], max_new_tokens=n, return_logits=True, forced_tokens=forced[1], **SPLIT)
    errs = [float(np.abs(out.logits[i].astype(np.float64) - l64.numpy()).max()) for i, (_, l64) in enumerate(ref["runs"])]
    print(f"split decode case {name} T={T}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} error {errs[0]:.3e} ({errs[0] / ref['tol']:.3f} tol), mate {errs[1]:.3e} ({errs[1] / ref['tol']:.3f} tol)")
    assert np.isfinite(out.logits).all() and max(errs) <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64), (name, i, out.tokens[i], t64)
    assert out.logits[1].tobytes() == alone.logits.tobytes() and np.array_equal(out.tokens[1], alone.tokens)


def test_free_running_tokens_equal_the_f64_reference():
    ref = R.reference_for("A")
    out = _model("A").generate(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=R.FREE_STEPS, **SPLIT)
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64), (i, out.tokens[i], t64)
    assert (out.counts == R.FREE_STEPS).all()


def test_a_sequence_does_not_depend_on_the_other_sequences_of_the_call():
    """Case A's 17-position prompt alone, as the first of 16 different sequences and as the last of them: tokens and logits bitwise equal."""
    ref = R.reference_for("A")
    case, weights = ref["case"], ref["weights"]
    lm = _model("A")
    emb, pos, _ = ref["prompts"][1]
    others = [R.make_prompt(case, weights, T, 50 + i) for i, T in enumerate([1, 3, 37, 16, 17, 2, 15, 33, 5, 18, 31, 4, 20, 9, 12])]
    n = 12
    alone = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, **SPLIT)
    first = lm.generate(inputs_embeds=[emb] + [o[0] for o in others], position_ids=[pos] + [o[1] for o in others], max_new_tokens=n, return_logits=True, **SPLIT)
    last = lm.generate(inputs_embeds=[o[0] for o in others] + [emb], position_ids=[o[1] for o in others] + [pos], max_new_tokens=n, return_logits=True, **SPLIT)
    assert np.array_equal(alone.tokens, ref["runs"][1][0][:n])
    for got, slot in ((first, 0), (last, 15)):
        assert np.array_equal(got.tokens[slot], alone.tokens)
        assert got.logits[slot].tobytes() == alone.logits.tobytes(), slot
    again = lm.generate(inputs_embeds=[o[0] for o in others] + [emb], position_ids=[o[1] for o in others] + [pos], max_new_tokens=n, return_logits=True, **SPLIT)
    assert again.logits.tobytes() == last.logits.tobytes() and again.tokens.tobytes() == last.tokens.tobytes()


def test_prefill_in_chunks_equals_one_position_at_a_time():
    """LD's geometry (case A's, a cache of 250 + 12): a 100-token prompt prefilled 16 rows a step against the same tokens fed one by one; position 64 opens the second span."""
    ref = R.long_reference_for("LD")
    case = ref["case"]
    ids = np.random.default_rng(7).integers(0, case.vocab, 100).astype(np.int32)
    n = 6
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=128, max_sequences=2), ref["weights"]) as lm:
        a = lm.generate(input_ids=ids, max_new_tokens=n, return_logits=True, **SPLIT)
        forced = np.concatenate([ids[1:], a.tokens[:n - 1]])
        b = lm.generate(input_ids=ids[:1], max_new_tokens=99 + n, return_logits=True, forced_tokens=forced, **SPLIT)
        serial = lm.generate(input_ids=ids, max_new_tokens=n, return_logits=True)
    assert b.logits[99:].tobytes() == a.logits.tobytes() and np.array_equal(b.tokens[99:], a.tokens)
    assert np.array_equal(serial.tokens, a.tokens) and serial.logits.tobytes() != a.logits.tobytes()          # (another sum order: the mode was really on)


def test_gemm_prefill_with_split_decode_stays_within_tol():
    """LA's 122-position prompt and its one-position mate: 121 GEMM rows, then the handover step and 12 decode steps through lm_attn_split / lm_attn_merge."""
    ref = R.long_reference_for("LA")
    case, T, n = ref["case"], ref["T"], R.LONG_STEPS
    emb, pos, forced = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]], [t for t, _ in ref["runs"]]
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=T + n, max_sequences=2), ref["weights"]) as lm:
        api.prof_reset()
        api.prof_enable(True)
        try:
            out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, forced_tokens=forced, prefill="gemm", **SPLIT)
            names = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["name"].startswith("lm_") and e["launches"]}
        finally:
            api.prof_enable(False)
    errs = [float(np.abs(out.logits[i].astype(np.float64) - l64.numpy()).max()) for i, (_, l64) in enumerate(ref["runs"])]
    print(f"gemm prefill + split decode case LA: noise {ref['noise']:.3e} tol {ref['tol']:.3e} errors {errs[0]:.3e} {errs[1]:.3e} ({max(errs) / ref['tol']:.3f} tol)")
    assert np.isfinite(out.logits).all() and max(errs) <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64)
    # every step's rows give a token (the handover step holds the last positions alone): n steps of L split and L merge launches, no serial attention
    assert names.get("lm_attn_split") == n * case.L and names.get("lm_attn_merge") == n * case.L and "lm_attn" not in names and "lm_prefill_attn" not in names, names


def test_a_short_call_after_a_long_call_equals_a_fresh_models():
    """A 250-position call fills four spans of the workspace; the one-position call after it reads the first alone."""
    ref = R.long_reference_for("LD")
    case, T = ref["case"], ref["T"]
    cfg = _cfg(case, max_positions=T + 8, max_sequences=2)
    with vl.CausalLM.from_state_dict(cfg, ref["weights"]) as used, vl.CausalLM.from_state_dict(cfg, ref["weights"]) as fresh:
        used.generate(inputs_embeds=ref["prompts"][0][0], position_ids=ref["prompts"][0][1], max_new_tokens=4, **SPLIT)
        a = used.generate(input_ids=[5], max_new_tokens=8, return_logits=True, **SPLIT)
        b = fresh.generate(input_ids=[5], max_new_tokens=8, return_logits=True, **SPLIT)
    assert a.logits.tobytes() == b.logits.tobytes() and a.tokens.tobytes() == b.tokens.tobytes()


def test_cost_follows_the_mode_and_a_serial_call_after_a_split_call_equals_a_fresh_models():
    ref = R.reference_for("A")
    L = ref["case"].L
    emb, pos = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]]
    with vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"]) as used, vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"]) as fresh:
        f0, b0, n0 = used.cost(3, 40)
        assert n0 == 5 * L + 2
        api.prof_reset()
        api.prof_enable(True)
        try:
            s = used.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True, **SPLIT)
            names = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["name"].startswith("lm_") and e["launches"]}
        finally:
            api.prof_enable(False)
        f1, b1, n1 = used.cost(3, 40)
        heads, dh = ref["case"].heads, ref["case"].head_dim
        assert n1 == 6 * L + 2 and f1 == f0 and b1 == b0 + 2 * 4 * 3 * L * heads * 1 * (dh + 2)             # one span of 64 keys: each partial written and read
        # 55 prompt rows in 4 steps (the fourth ends all three prompts... or not: whichever, its classes are the prefill ones unless every row gives a token), 9 decode steps
        steps = -(-sum(e.shape[0] for e in emb) // 16) + 9
        assert names["lm_attn_split"] + names["lm_prefill_attn_split"] == steps * L == names["lm_attn_merge"] + names["lm_prefill_attn_merge"], names
        assert "lm_attn" not in names and "lm_prefill_attn" not in names
        a = used.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)          # (the default: serial)
        assert used.cost(3, 40) == (f0, b0, n0)
        b = fresh.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)
    assert a.logits.tobytes() == b.logits.tobytes() and a.tokens.tobytes() == b.tokens.tobytes()
    assert np.array_equal(s.tokens, a.tokens) and s.logits.tobytes() != a.logits.tobytes()


def test_stop_at_eos_returns_the_bytes_of_the_call_that_does_not_stop():
    """Case A's two sequences whose eos is the first token of one and a later token of the other, 64 tokens asked for: 4 prefill steps and 63 decode steps scheduled."""
    ref = R.reference_for("A")
    i, j, eos, nj = R.all_end_choice(ref)
    n = 64
    emb, pos = [ref["prompts"][i][0], ref["prompts"][j][0]], [ref["prompts"][i][1], ref["prompts"][j][1]]
    cfg = _cfg(ref["case"], max_positions=128, max_sequences=2)
    g = S.split_arithmetic()
    stride, look = g["stop_stride"], g["stop_lookahead"]
    again = dict(inputs_embeds=list(reversed(emb)), position_ids=list(reversed(pos)), max_new_tokens=12, return_logits=True)
    with vl.CausalLM.from_state_dict(cfg, ref["weights"]) as lm, vl.CausalLM.from_state_dict(cfg, ref["weights"]) as fresh:
        assert lm.decode_stats() == (0, 0)
        for mode in (dict(), SPLIT):
            off = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, eos_token_id=eos, return_logits=True, **mode)
            limit, enq = lm.decode_stats()
            prefill_steps = -(-(emb[0].shape[0] + emb[1].shape[0]) // 16)
            assert limit == enq == prefill_steps + n - 1
            on = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, eos_token_id=eos, return_logits=True, stop_at_eos=True, **mode)
            limit, enq = lm.decode_stats()
            t_stop = prefill_steps - 1 + nj - 1                                                  # the step that gives token nj - 1 of the longer-lived sequence
            print(f"stop at eos: t_stop {t_stop}, steps_enqueued {enq} of {limit}, bound {t_stop + 1 + look + stride}")
            assert limit == prefill_steps + n - 1 and enq <= t_stop + 1 + look + stride and enq < limit
            assert on.tokens.tobytes() == off.tokens.tobytes() and on.counts.tobytes() == off.counts.tobytes() and on.counts.tolist() == [1, nj]
            assert on.logits[1, :nj].tobytes() == off.logits[1, :nj].tobytes() and on.logits[0, 0].tobytes() == off.logits[0, 0].tobytes()
            assert (on.tokens[0] == eos).all() and (on.tokens[1, nj:] == eos).all()
            none_on = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, eos_token_id=None, return_logits=True, stop_at_eos=True, **mode)
            assert lm.decode_stats() == (limit, limit)
            none_off = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, eos_token_id=None, return_logits=True, **mode)
            assert none_on.tokens.tobytes() == none_off.tokens.tobytes() and none_on.logits.tobytes() == none_off.logits.tobytes() and none_on.counts.tolist() == [n, n]
            lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, eos_token_id=eos, stop_at_eos=True, **mode)
            after = lm.generate(**again)
            clean = fresh.generate(**again)
            assert after.logits.tobytes() == clean.logits.tobytes() and after.tokens.tobytes() == clean.tokens.tobytes()


def test_set_decode_rejects_what_it_does_not_know():
    lm = _model("A")
    L = vl._lib()
    assert L.oar_lm_set_decode(None, 1, 64, 0) == api.OAR_INVALID_INPUT
    for mode in (2, -1):
        assert L.oar_lm_set_decode(lm._h, mode, 64, 0) == api.OAR_INVALID_INPUT
    for sk in (-64, 1, 32, 63, 65, 96, 4160, 8192):
        assert L.oar_lm_set_decode(lm._h, 1, sk, 0) == api.OAR_INVALID_INPUT, sk
        assert L.oar_lm_set_decode(lm._h, 0, sk, 0) == api.OAR_INVALID_INPUT, sk
    for stop in (2, -1):
        assert L.oar_lm_set_decode(lm._h, 1, 64, stop) == api.OAR_INVALID_INPUT
    for ok in ((1, 0, 0), (1, 64, 1), (1, 4096, 0), (0, 0, 1), (0, 0, 0)):
        assert L.oar_lm_set_decode(lm._h, *ok) == api.OAR_OK, ok
    for kw in (dict(decode_attention="flash"), dict(decode_attention="split", split_keys=100), dict(decode_attention="split", split_keys=-64)):
        with pytest.raises(api.OCRError) as e:
            lm.generate(input_ids=[1, 2, 3], max_new_tokens=2, **kw)
        assert e.value.code == api.OAR_INVALID_INPUT
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert L.oar_lm_decode_stats(None, C.byref(a), C.byref(b)) == api.OAR_INVALID_INPUT
    assert L.oar_lm_decode_stats(lm._h, None, None) == api.OAR_OK
    out = lm.generate(input_ids=[1, 2, 3], max_new_tokens=2)                                                  # the refusals have left the model as it was
    assert out.tokens.shape == (2,)
