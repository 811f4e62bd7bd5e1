"""vl.CausalLM.generate with repetition_penalty / no_repeat_ngram_size (oar_lm_generate_ex; lm_logits.hip).

Exact replay: the device's token at every step equals the numpy-f32 processors applied on the host to the device's OWN raw logits row of that step with the history so
far -- bit-exact by construction, no tolerance.  Against f64: the tokens equal the f64 reference's at all 48 steps; legitimate because the pinned seeds keep the best
processed f64 logit more than 4 r tol ahead of the second (tests/test_lm_logits_cases_cpu.py).  Cases A, E, C, V and the three settings: synth/lm_logits_cases.py."""
import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_logits_cases as LC
from oar_ocr_amd.synth import lm_reference as R

pytestmark = pytest.mark.gpu

MAX_POS = 96      # 37 + 48 positions
RUNS = [(name, s) for name in LC.MODEL_CASES for s in LC.SETTINGS]
RUN_IDS = [f"{name}-r{r}-n{n}" for name, (r, n) in RUNS]


def _cfg(case, **kw):
    d = dict(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, num_key_value_heads=case.kv_heads, head_dim=case.head_dim, intermediate_size=case.F,
             vocab_size=case.vocab, rms_norm_eps=case.eps, rope_theta=case.theta, mrope_section=list(case.mrope_section), qkv_bias=case.qkv_bias, tie_word_embeddings=case.tie,
             max_positions=MAX_POS, max_sequences=16)
    d.update(kw)
    return vl.CausalLMConfig(**d)


_MODELS, _OUTS = {}, {}


def _model(name):
    if name not in _MODELS:
        ref = LC.reference_for(name)
        _MODELS[name] = vl.CausalLM.from_state_dict(_cfg(ref["case"]), ref["weights"])
    return _MODELS[name]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()
    _OUTS.clear()


def _prompt_kw(ref, which=(0, 1)):
    return dict(inputs_embeds=[ref["prompts"][i][0] for i in which], position_ids=[ref["prompts"][i][1] for i in which], history_ids=[ref["prompts"][i][2] for i in which])


def _free_run(name, setting):
    """one free run with logits per (case, setting), shared by the tests that look at it"""
    if (name, setting) not in _OUTS:
        ref = LC.reference_for(name)
        _OUTS[(name, setting)] = _model(name).generate(max_new_tokens=LC.STEPS, return_logits=True, repetition_penalty=setting[0], no_repeat_ngram_size=setting[1], **_prompt_kw(ref))
    return _OUTS[(name, setting)]


def _replay(out, histories, r, n, steps, eos=None):
    """the numpy-f32 processors on the device's own logits: the first (sequence, step) whose token differs, or None"""
    for i, ids in enumerate(histories):
        hist = [int(v) for v in ids]
        for g in range(steps):
            tok = LC.choose(LC.process(out.logits[i, g], hist, r, n))
            if tok != int(out.tokens[i, g]):
                return (i, g, tok, int(out.tokens[i, g]))
            if eos is not None and tok == eos:
                break
            hist.append(tok)
    return None


@pytest.mark.parametrize("name,setting", RUNS, ids=RUN_IDS)
def test_every_token_is_the_processed_argmax_of_the_devices_own_logits(name, setting):
    ref = LC.reference_for(name)
    out = _free_run(name, setting)
    assert out.tokens.shape == (2, LC.STEPS) and np.isfinite(out.logits).all() and out.counts.tolist() == [LC.STEPS] * 2
    assert _replay(out, [p[2] for p in ref["prompts"]], setting[0], setting[1], LC.STEPS) is None


@pytest.mark.parametrize("name,setting", RUNS, ids=RUN_IDS)
def test_tokens_equal_the_f64_reference(name, setting):
    ref = LC.reference_for(name)
    out = _free_run(name, setting)
    for i, g in enumerate(ref["runs"][setting]):
        assert np.array_equal(out.tokens[i], g["tokens"]), (name, setting, i, out.tokens[i], g["tokens"])
        err = float(np.abs(out.logits[i].astype(np.float64) - g["raw"].numpy()).max())
        print(f"case {name} r {setting[0]} n {setting[1]} sequence {i}: raw logit error {err:.3e} = {err / ref['tol']:.3f} tol")
        assert err <= ref["tol"]


@pytest.mark.parametrize("name,setting", RUNS, ids=RUN_IDS)
def test_returned_logits_stay_the_raw_logits(name, setting):
    """Forced to the f64 run's tokens, the logits with processors on are the bytes of the same call with processors off; the tokens are the f64 run's, and differ from
    the plain arg-max wherever the f64 run's token differs from its raw arg-max (steps whose raw f64 margin is below 4 tol aside)."""
    ref = LC.reference_for(name)
    lm = _model(name)
    runs = ref["runs"][setting]
    kw = dict(max_new_tokens=LC.STEPS, return_logits=True, forced_tokens=[g["tokens"] for g in runs], **_prompt_kw(ref))
    on = lm.generate(repetition_penalty=setting[0], no_repeat_ngram_size=setting[1], **kw)
    off = lm.generate(**kw)
    assert on.logits.tobytes() == off.logits.tobytes()
    for i, g in enumerate(runs):
        assert np.array_equal(on.tokens[i], g["tokens"])
        top = np.sort(g["raw"].numpy(), axis=1)
        safe = top[:, -1] - top[:, -2] > 4.0 * ref["tol"]
        named = (g["tokens"] != g["raw_argmax"]) & safe
        assert np.array_equal(off.tokens[i][safe], g["raw_argmax"][safe])
        assert (on.tokens[i][named] != off.tokens[i][named]).all()
        if name in LC.BITE_CASES:
            assert int((on.tokens[i] != off.tokens[i]).sum()) >= 3


def test_composes_with_gemm_prefill_and_split_attention():
    ref = LC.reference_for("A")
    lm = _model("A")
    s = (1.3, 3)
    kw = dict(max_new_tokens=LC.STEPS, return_logits=True, repetition_penalty=s[0], no_repeat_ngram_size=s[1], **_prompt_kw(ref))
    for extra in (dict(prefill="gemm"), dict(decode_attention="split"), dict(prefill="gemm", prefill_chunk=16, decode_attention="split", split_keys=64)):
        out = lm.generate(**kw, **extra)
        assert _replay(out, [p[2] for p in ref["prompts"]], s[0], s[1], LC.STEPS) is None, extra
        for i, g in enumerate(ref["runs"][s]):
            assert np.array_equal(out.tokens[i], g["tokens"]), (extra, i)


def test_eos_rule_with_and_without_stop_at_eos():
    """eos = a token the processed run emits mid-way: tokens up to it, eos behind it, counts, identical with stop_at_eos (which then enqueues fewer steps)"""
    ref = LC.reference_for("A")
    lm = _model("A")
    s = (1.3, 3)
    runs = ref["runs"][s]
    eos = int(runs[0]["tokens"][9])
    firsts = [int(np.flatnonzero(g["tokens"] == eos)[0]) if (g["tokens"] == eos).any() else None for g in runs]
    assert firsts[0] is not None and firsts[0] <= 9
    kw = dict(max_new_tokens=LC.STEPS, return_logits=True, eos_token_id=eos, repetition_penalty=s[0], no_repeat_ngram_size=s[1], **_prompt_kw(ref))
    a = lm.generate(**kw)
    b = lm.generate(stop_at_eos=True, **kw)
    limit, enq = lm.decode_stats()
    for i, (g, f) in enumerate(zip(runs, firsts)):
        n = LC.STEPS if f is None else f + 1
        assert a.counts[i] == n and np.array_equal(a.tokens[i, :n], g["tokens"][:n]) and (a.tokens[i, n:] == eos).all()
    assert a.tokens.tobytes() == b.tokens.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    assert _replay(a, [p[2] for p in ref["prompts"]], s[0], s[1], LC.STEPS, eos=eos) is None
    if all(f is not None for f in firsts):
        assert enq <= limit and enq <= (limit - (LC.STEPS - 1)) + max(firsts) + 16 + 8 + 1


def test_a_row_does_not_depend_on_its_step_mates_or_its_slot():
    """Sequence 0 alone, as the first of 16 different sequences and in the last slot: tokens and logits bitwise equal, processors on"""
    ref = LC.reference_for("A")
    case, weights = ref["case"], ref["weights"]
    lm = _model("A")
    emb, pos, ids = ref["prompts"][0]
    others = [R.make_prompt(case, weights, T, 50 + i) for i, T in enumerate([1, 3, 37, 16, 17, 2, 15, 33, 5, 18, 31, 4, 20, 9, 12])]
    kw = dict(max_new_tokens=16, return_logits=True, repetition_penalty=1.3, no_repeat_ngram_size=3)
    alone = lm.generate(inputs_embeds=emb, position_ids=pos, history_ids=ids, **kw)
    first = lm.generate(inputs_embeds=[emb] + [o[0] for o in others], position_ids=[pos] + [o[1] for o in others], history_ids=[ids] + [o[2] for o in others], **kw)
    last = lm.generate(inputs_embeds=[o[0] for o in others] + [emb], position_ids=[o[1] for o in others] + [pos], history_ids=[o[2] for o in others] + [ids], **kw)
    assert np.array_equal(alone.tokens, ref["runs"][(1.3, 3)][0]["tokens"][:16])
    for got, slot in ((first, 0), (last, 15)):
        assert np.array_equal(got.tokens[slot], alone.tokens) and got.logits[slot].tobytes() == alone.logits.tobytes(), slot
    assert _replay(last, [o[2] for o in others] + [ids], 1.3, 3, 16) is None
    again = lm.generate(inputs_embeds=[o[0] for o in others] + [emb], position_ids=[o[1] for o in others] + [pos], history_ids=[o[2] for o in others] + [ids], **kw)
    assert again.tokens.tobytes() == last.tokens.tobytes() and again.logits.tobytes() == last.logits.tobytes()


def _snapshot(fn):
    api.prof_reset()
    api.prof_enable(True)
    try:
        out = fn()
        snap = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["name"].startswith("lm_") and e["launches"]}
    finally:
        api.prof_enable(False)
    return out, snap


def test_off_is_off_and_on_adds_one_lm_select_launch_per_step():
    ref = LC.reference_for("A")
    lm = _model("A")
    L, n = ref["case"].L, 5
    plain_classes = {"lm_rows": 4 * L * n, "lm_attn": L * n, "lm_head": n, "lm_combine": n, "lm_embed": 1}
    base, snap = _snapshot(lambda: lm.generate(input_ids=[11], max_new_tokens=n, return_logits=True))
    assert snap == plain_classes and sum(v for k, v in snap.items() if k != "lm_embed") == n * (5 * L + 2)
    for kw in (dict(repetition_penalty=1.0, no_repeat_ngram_size=0), dict(repetition_penalty=1.0, no_repeat_ngram_size=1), dict(history_ids=[5, 6, 7])):
        out, snap = _snapshot(lambda: lm.generate(input_ids=[11], max_new_tokens=n, return_logits=True, **kw))
        assert snap == plain_classes, (kw, snap)
        assert out.tokens.tobytes() == base.tokens.tobytes() and out.logits.tobytes() == base.logits.tobytes()
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(repetition_penalty=2.0, no_repeat_ngram_size=3)):
        out, snap = _snapshot(lambda: lm.generate(input_ids=[11], max_new_tokens=n, return_logits=True, **kw))
        assert snap == dict(plain_classes, lm_select=n), (kw, snap)
        assert sum(v for k, v in snap.items() if k != "lm_embed") == n * (5 * L + 3)
        assert _replay(vl.LMOutput(out.tokens[None], out.counts, out.logits[None]), [[11]], kw.get("repetition_penalty", 1.0), kw.get("no_repeat_ngram_size", 0), n) is None
    _, snap = _snapshot(lambda: lm.generate(input_ids=[11], max_new_tokens=n, repetition_penalty=1.3, decode_attention="split"))
    assert snap.get("lm_select") == n and sum(v for k, v in snap.items() if k != "lm_embed") == n * (6 * L + 3), snap


def test_rejected_arguments_launch_nothing():
    ref = LC.reference_for("A")
    lm = _model("A")
    emb, pos, ids = ref["prompts"][0]

    def attempts():
        for kw, code in ((dict(input_ids=[1, 2, 3], repetition_penalty=1.3, schedule="refill"), api.OAR_UNSUPPORTED_OP),
                         (dict(input_ids=[1, 2, 3], no_repeat_ngram_size=2, schedule="refill"), api.OAR_UNSUPPORTED_OP),
                         (dict(input_ids=[1, 2, 3], repetition_penalty=0.5), api.OAR_INVALID_INPUT), (dict(input_ids=[1, 2, 3], repetition_penalty=float("nan")), api.OAR_INVALID_INPUT),
                         (dict(input_ids=[1, 2, 3], no_repeat_ngram_size=-1), api.OAR_INVALID_INPUT),
                         (dict(inputs_embeds=emb, position_ids=pos, repetition_penalty=1.3), api.OAR_INVALID_INPUT),
                         (dict(inputs_embeds=emb, position_ids=pos, no_repeat_ngram_size=2, history_ids=[1, -2, 3]), api.OAR_INVALID_INPUT),
                         (dict(input_ids=[1, 2, 3], repetition_penalty=1.3, history_ids=[0] * 65537), api.OAR_INVALID_INPUT)):
            with pytest.raises(api.OCRError) as e:
                lm.generate(max_new_tokens=4, **kw)
            assert e.value.code == code, (kw, str(e.value))

    _, snap = _snapshot(attempts)
    assert snap == {}, snap
    out = lm.generate(input_ids=[[1, 2, 3]] * 18, max_new_tokens=6, no_repeat_ngram_size=2, repetition_penalty=1.3)      # 18 sequences run as 16 + 2, histories sliced with them
    assert out.tokens.shape == (18, 6) and (out.tokens == out.tokens[0]).all()


def test_images_to_tokens_with_processors_matches_the_composite_reference():
    """composite case PA through vl.PaddleOCRVL.generate_tokens with PA_SETTING: the history is the expanded ids (prefix, one image id per image token, suffix)"""
    from oar_ocr_amd.synth import vision_reference as vr
    p = LC.composite_reference()
    r = p["base"]
    vc, lc = r["vis_case"], r["lm_case"]
    cfg_json = dict(hidden_size=lc.D, num_hidden_layers=lc.L, num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, head_dim=lc.head_dim, intermediate_size=lc.F,
                    vocab_size=lc.vocab, rms_norm_eps=lc.eps, rope_theta=lc.theta, rope_scaling=dict(mrope_section=list(lc.mrope_section)), tie_word_embeddings=lc.tie,
                    image_token_id=vr.PA_IDS["image"], vision_start_token_id=vr.PA_IDS["start"],
                    vision_config=dict(hidden_size=vc.D, num_hidden_layers=vc.L, num_attention_heads=vc.heads, intermediate_size=vc.F, patch_size=vc.patch, image_size=vc.G * vc.patch,
                                       spatial_merge_size=vc.merge, layer_norm_eps=vc.eps, hidden_act=vc.act))
    preproc = dict(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096, rescale_factor=1.0 / 255.0, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    rp, ng = LC.PA_SETTING
    with vl.PaddleOCRVL.from_state_dict(cfg_json, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=2), vision_overrides=dict(max_tokens=64, max_images=2)) as m:
        out = m.generate_tokens(r["images"], vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=vr.PA_STEPS, return_logits=True, repetition_penalty=rp, no_repeat_ngram_size=ng)
        with pytest.raises(api.OCRError) as e:
            m.generate_tokens(r["images"], vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=4, repetition_penalty=rp, schedule="refill")
        assert e.value.code == api.OAR_UNSUPPORTED_OP
    for i, g in enumerate(p["runs"]):
        assert g["margin"].min() > 4.0 * rp * p["tol"]
        assert np.array_equal(out.tokens[i], g["tokens"]), (i, out.tokens[i], g["tokens"])
    assert _replay(out, [run[2] for run in r["runs"]], rp, ng, vr.PA_STEPS) is None
