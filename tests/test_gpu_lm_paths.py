"""vl.CausalLM (lm_decode.hip) on the kernel paths that the short cases of tests/test_gpu_lm_decode.py cannot reach: caches of hundreds of positions (the attention
kernel's unrolled turns, its second outer iteration, eight waves with keys), equal maxima at every level of the argmax, every sequence at its eos, a cache that an earlier
call left full, and bf16 tables on the G = 8 and the three-row-group cases.  Same frame: the f64 torch reference of synth/lm_reference.py, tol = max(16 noise, 2^-19) from
the reference's own f32 run, inputs whose conditions (greedy margins, the weight of every boundary key) tests/test_lm_reference_cpu.py checks."""
import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_reference as R

pytestmark = pytest.mark.gpu


def _cfg(case, **kw):
    d = dict(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, num_key_value_heads=case.kv_heads, head_dim=case.head_dim, intermediate_size=case.F,
             vocab_size=case.vocab, rms_norm_eps=case.eps, rope_theta=case.theta, mrope_section=list(case.mrope_section), qkv_bias=case.qkv_bias, tie_word_embeddings=case.tie,
             max_positions=64, max_sequences=16)
    d.update(kw)
    return vl.CausalLMConfig(**d)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(R.LONG_CASES))
def test_long_cache_logits_are_within_the_f32_noise_of_f64(name):
    """A prompt of T positions (the image block in its middle) and a one-position prompt in one call, LONG_STEPS steps forced to the f64 tokens, in a cache of exactly
    T + LONG_STEPS positions: rows that attend one key and rows that attend hundreds share every step.  Both sequences' logits within tol, exact tokens, and the mate's
    logits and tokens bitwise equal to the mate run alone."""
    ref = R.long_reference_for(name)
    case, T, n = ref["case"], ref["T"], R.LONG_STEPS
    emb, pos, forced = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]], [t for t, _ in ref["runs"]]
    with vl.CausalLM.from_state_dict(_cfg(case, max_positions=T + n, max_sequences=2), ref["weights"]) as lm:
        out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True, forced_tokens=forced)
        alone = lm.generate(inputs_embeds=emb[1], position_ids=pos[1], max_new_tokens=n, return_logits=True, forced_tokens=forced[1])
    errs = [float(np.abs(out.logits[i].astype(np.float64) - l64.numpy()).max()) for i, (_, l64) in enumerate(ref["runs"])]
    print(f"case {name} T={T}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} error {errs[0]:.3e} ({errs[0] / ref['tol']:.3f} tol), mate {errs[1]:.3e} ({errs[1] / ref['tol']:.3f} tol)")
    assert np.isfinite(out.logits).all() and max(errs) <= ref["tol"]
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64), (name, i, out.tokens[i], t64)
    assert out.logits[1].tobytes() == alone.logits.tobytes() and np.array_equal(out.tokens[1], alone.tokens)


@pytest.mark.parametrize("place", R.TIE_PLACES)
def test_lowest_index_among_equal_maxima(place):
    """Case V's geometry (three row groups per lm-head workgroup, 417 workgroups) with lm-head row v a copy of row v - d wherever (v // d) is odd: the pair sits in one
    wave, in neighbouring waves, row groups, workgroups, or in workgroups half the grid apart (and at the plain distances 16, 48 and 9984).  The two rows of every pair
    have the same logit bits, and every token is the lowest index among the rows identical to the f64 winner's."""
    d = R.tie_distances()[place]
    ref = R.tie_reference_for(d)
    canon, n = ref["canon"], R.TEACHER_STEPS
    with vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"]) as lm:
        out = lm.generate(inputs_embeds=[p[0] for p in ref["prompts"]], position_ids=[p[1] for p in ref["prompts"]], max_new_tokens=n, return_logits=True,
                          forced_tokens=[t for t, _ in ref["runs"]])
    err = max(float(np.abs(out.logits[i].astype(np.float64) - l64.numpy()).max()) for i, (_, l64) in enumerate(ref["runs"]))
    paired = int(sum((t64 + d < len(canon)).sum() for t64, _ in ref["runs"]))
    print(f"equal maxima {place} d={d}: tol {ref['tol']:.3e} error {err:.3e} ({err / ref['tol']:.3f} tol); {paired} of {3 * n} winners have a copy")
    assert np.isfinite(out.logits).all() and err <= ref["tol"]
    assert np.array_equal(_bits(out.logits), _bits(out.logits[..., canon]))
    for i, (t64, _) in enumerate(ref["runs"]):
        assert np.array_equal(out.tokens[i], t64), (place, i, out.tokens[i], t64)


@pytest.mark.parametrize("name", ["E", "V"])
def test_bf16_tables_equal_the_same_values_widened_to_f32_on_the_new_paths(name):
    """E: eight query heads per kv head; V: three row groups per lm-head workgroup."""
    ref = R.reference_for(name)
    case, weights = ref["case"], ref["weights"]
    bits = {k: R.to_bf16_bits(v) for k, v in weights.items()}
    wide = {k: R.bf16_bits_to_f32(v) for k, v in bits.items()}
    emb, pos = [p[0] for p in ref["prompts"]], [p[1] for p in ref["prompts"]]
    with vl.CausalLM.from_state_dict(_cfg(case), bits) as m16, vl.CausalLM.from_state_dict(_cfg(case), wide) as m32, vl.CausalLM.from_state_dict(_cfg(case), weights) as m:
        a = m16.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)
        b = m32.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)
        c = m16.generate(input_ids=[3, 1, 4, 1, 5], max_new_tokens=6, return_logits=True)
        d = m32.generate(input_ids=[3, 1, 4, 1, 5], max_new_tokens=6, return_logits=True)
        e = m.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=10, return_logits=True)
    assert a.logits.tobytes() == b.logits.tobytes() and np.array_equal(a.tokens, b.tokens)
    assert c.logits.tobytes() == d.logits.tobytes() and np.array_equal(c.tokens, d.tokens)
    assert float(np.abs(a.logits - e.logits).max()) > 1e-3      # (rounding did change the model)


def _lm_launches():
    return sum(e["launches"] for e in api.prof_snapshot() if e["name"].startswith("lm_"))


def test_every_sequence_ends_early():
    """Two sequences of case A and an eos that is the first token of one and a later token of the other: from then on `alive` is 0, every kernel of every scheduled step
    is still launched and returns at once, lm_combine writes eos.  The next call on the model starts from a clean state."""
    ref = R.reference_for("A")
    i, j, eos, nj = R.all_end_choice(ref)
    L, n = ref["case"].L, R.FREE_STEPS
    emb, pos = [ref["prompts"][i][0], ref["prompts"][j][0]], [ref["prompts"][i][1], ref["prompts"][j][1]]
    ti, tj = ref["runs"][i][0], ref["runs"][j][0]
    again = dict(inputs_embeds=list(reversed(emb)), position_ids=list(reversed(pos)), max_new_tokens=n, return_logits=True)
    with vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"]) as lm, vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"]) as fresh:
        api.prof_reset()
        api.prof_enable(True)
        try:
            out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, eos_token_id=eos)
            launches = _lm_launches()
        finally:
            api.prof_enable(False)
        after = lm.generate(**again)
        clean = fresh.generate(**again)
    assert out.counts.tolist() == [1, nj] and 1 < nj < n
    assert out.tokens[0, 0] == ti[0] == eos and (out.tokens[0] == eos).all()
    assert np.array_equal(out.tokens[1, :nj], tj[:nj]) and (out.tokens[1, nj:] == eos).all()
    # the schedule: the prompts' rows packed 16 to a step (5 L launches, and 2 more where a prompt ends in the step), then one step per further token
    Ti, Tj = emb[0].shape[0], emb[1].shape[0]
    prefill = -(-(Ti + Tj) // 16)
    ending = len({(Ti - 1) // 16, (Ti + Tj - 1) // 16})
    assert launches == prefill * 5 * L + ending * 2 + (n - 1) * (5 * L + 2), (launches, prefill, ending)
    assert after.logits.tobytes() == clean.logits.tobytes() and after.tokens.tobytes() == clean.tokens.tobytes() and after.counts.tolist() == [n, n]
    assert np.array_equal(after.tokens[0], tj) and np.array_equal(after.tokens[1], ti)


def test_a_short_call_over_a_cache_that_a_longer_call_filled():
    """Slots 0 to 2 filled by three 37-position prompts and 24 tokens each (61 of 64 positions), then a one-position prompt in slot 0: it attends its own keys only, so
    it equals the same call on a fresh model bit for bit."""
    ref = R.reference_for("A")
    case, weights = ref["case"], ref["weights"]
    long = [R.make_prompt(case, weights, 37, 60 + s) for s in range(3)]
    emb, pos, _ = ref["prompts"][0]
    n = R.FREE_STEPS
    with vl.CausalLM.from_state_dict(_cfg(case), weights) as lm, vl.CausalLM.from_state_dict(_cfg(case), weights) as fresh:
        filled = lm.generate(inputs_embeds=[p[0] for p in long], position_ids=[p[1] for p in long], max_new_tokens=n)
        a = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True)
        b = fresh.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=n, return_logits=True)
    assert filled.counts.tolist() == [n] * 3
    assert a.logits.tobytes() == b.logits.tobytes() and a.tokens.tobytes() == b.tokens.tobytes()
    assert np.array_equal(a.tokens, ref["runs"][0][0])
