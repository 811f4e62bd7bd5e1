"""vl.CausalLM.generate(schedule="refill") (oar_lm_generate_queue, lm_queue.hip): any number of sequences share <= 16 cache slots and a finished
sequence's slot goes to the next waiting one.  The workload of synth/lm_queue_cases.py against its f64 reference (tokens, counts, teacher-forced logits within the
case's own tol) and, byte for byte, against every sequence run alone, in rows / gemm prefill x serial / split attention; the orders of use of one slot, queues
without eos, a sequence of NaN embeddings in the queue, reproducibility, and PaddleOCRVL.generate_tokens on more than 16 images."""
import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_queue_cases as Q
from oar_ocr_amd.synth import vision_reference as vr

pytestmark = pytest.mark.gpu

MAX_POS = 64
MODES = {"rows-serial": dict(prefill="rows", decode_attention="serial"), "rows-split": dict(prefill="rows", decode_attention="split", split_keys=64),
         "gemm-serial": dict(prefill="gemm", decode_attention="serial"), "gemm-split": dict(prefill="gemm", decode_attention="split", split_keys=64)}

_LM = {}
_ALONE = {}


def _cfg(case, **kw):
    d = dict(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, num_key_value_heads=case.kv_heads, head_dim=case.head_dim, intermediate_size=case.F,
             vocab_size=case.vocab, rms_norm_eps=case.eps, rope_theta=case.theta, mrope_section=list(case.mrope_section), qkv_bias=case.qkv_bias, tie_word_embeddings=case.tie,
             max_positions=MAX_POS, max_sequences=16)
    d.update(kw)
    return vl.CausalLMConfig(**d)


def _model():
    if "lm" not in _LM:
        w = Q.workload()
        _LM["lm"] = vl.CausalLM.from_state_dict(_cfg(w["case"]), w["weights"])
    return _LM["lm"]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _LM.values():
        m.close()
    _LM.clear()
    _ALONE.clear()


def _alone(mode, eos, max_new=Q.MAX_NEW):
    """Every sequence of the workload through generate on its own (teacher-forced with the expected tokens when eos is the workload's), once per mode."""
    key = (mode, eos, max_new)
    if key not in _ALONE:
        w, lm = Q.workload(), _model()
        outs = []
        for i, (emb, pos, _) in enumerate(w["prompts"]):
            forced = w["tokens"][i] if eos is not None else None
            outs.append(lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=max_new, eos_token_id=eos, return_logits=True, forced_tokens=forced, **MODES[mode]))
        _ALONE[key] = outs
    return _ALONE[key]


def _equal_to_alone(out, idx, alone, eos):
    """tokens, counts and the logits rows up to each count equal the alone runs' bytes; the logits rows behind a count are zero."""
    for n, i in enumerate(idx):
        a = alone[i]
        c = int(a.counts[0])
        assert int(out.counts[n]) == c, (n, i, out.counts[n], c)
        assert out.tokens[n].tobytes() == a.tokens.tobytes(), (n, i, out.tokens[n], a.tokens)
        if out.logits is not None:
            assert out.logits[n, :c].tobytes() == a.logits[:c].tobytes(), (n, i)
            assert not out.logits[n, c:].any(), (n, i)


@pytest.mark.parametrize("slots", [16, 4])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_workload_equals_f64_and_every_sequence_alone(mode, slots):
    w, lm = Q.workload(), _model()
    c = Q.queue_constants()
    emb, pos = [p[0] for p in w["prompts"]], [p[1] for p in w["prompts"]]
    n = len(emb)
    out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=Q.MAX_NEW, eos_token_id=Q.EOS, return_logits=True, forced_tokens=list(w["tokens"]), schedule="refill",
                      slots=slots, **MODES[mode])
    stats = lm.queue_stats()
    assert np.array_equal(out.tokens, w["tokens"]), np.argwhere(out.tokens != w["tokens"])[:5]
    assert np.array_equal(out.counts, w["counts"])
    err = max(float(np.abs(out.logits[i, :k].astype(np.float64) - w["logits64"][i, :k]).max()) for i, k in enumerate(w["counts"]))
    print(f"queue workload {mode} slots {slots}: noise {w['noise']:.3e} tol {w['tol']:.3e} error {err:.3e} ({err / w['tol']:.3f} tol), least margin {w['margin'] / w['tol']:.1f} tol; {stats}")
    assert np.isfinite(out.logits).all() and err <= w["tol"]
    _equal_to_alone(out, range(n), _alone(mode, Q.EOS), Q.EOS)
    free = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=Q.MAX_NEW, eos_token_id=Q.EOS, schedule="refill", slots=slots, **MODES[mode])
    assert free.tokens.tobytes() == out.tokens.tobytes() and free.counts.tobytes() == out.counts.tobytes() and free.logits is None
    # every slot was turned over at least twice, and no sequence idled longer than the lag allows.  A turnover is one entry of lm_queue_turnover for the slot; a slot
    # that held a single sequence has two (to it, away from it), so the stronger figure is asserted wherever the schedule can reach it: every slot held two sequences
    # or more.  With the rows prefill on 16 slots it cannot: the first 16 prompts' 230 rows take 15 steps, slot 15 gets its first row at step 14, and the 24 waiting
    # sequences have gone to the slots that started earlier before it retires (1 in the simulation of tests/test_lm_queue_cpu.py for every seed that was tried).
    assert stats["admissions"] == n and stats["min_slot_turnovers"] >= 2
    assert stats["min_slot_admissions"] >= (1 if (slots == 16 and mode.startswith("rows")) else 2)
    assert stats["max_dead_rows"] <= c["lookahead"] + c["stride"] and stats["dead_rows"] <= int((w["counts"] < Q.MAX_NEW).sum()) * (c["lookahead"] + c["stride"])
    produced_least = int(w["counts"].sum()) + sum(int(p[0].shape[0]) - 1 for p in w["prompts"])
    gemm_rows = sum(int(p[0].shape[0]) - 1 for p in w["prompts"]) if mode.startswith("gemm") else 0
    assert stats["rows"] == produced_least + stats["dead_rows"] - gemm_rows and stats["steps"] * 16 >= stats["rows"]
    assert (stats["gemm_phases"] > 0) == mode.startswith("gemm") and stats["gemm_phases"] <= n - slots + 1


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("mode", ["rows-serial", "gemm-split"])
def test_a_slot_used_by_long_after_short_and_short_after_long(mode, slots):
    """Seven sequences with prompts of 37, 9, 1, 33, 2, 16 and 3 positions that end after 12, 1, 12, 3, 12, 2 and 8 tokens: with one slot every sequence inherits the
    `done` flag, token row and cache of the one before it."""
    w, lm = Q.workload(), _model()
    idx = [2, 13, 0, 7, 5, 3, 1]
    assert [int(w["counts"][i]) for i in idx] == [12, 1, 12, 3, 12, 2, 8] and [w["prompts"][i][0].shape[0] for i in idx] == [37, 9, 1, 33, 2, 16, 3]
    out = lm.generate(inputs_embeds=[w["prompts"][i][0] for i in idx], position_ids=[w["prompts"][i][1] for i in idx], max_new_tokens=Q.MAX_NEW, eos_token_id=Q.EOS,
                      return_logits=True, schedule="refill", slots=slots, **MODES[mode])
    assert np.array_equal(out.tokens, w["tokens"][idx])
    _equal_to_alone(out, idx, _alone(mode, Q.EOS), Q.EOS)
    assert lm.queue_stats()["admissions"] == 7


@pytest.mark.parametrize("mode", ["rows-serial", "gemm-split"])
def test_queues_without_eos_and_of_one_token(mode):
    w, lm = Q.workload(), _model()
    idx = list(range(20))
    emb, pos = [w["prompts"][i][0] for i in idx], [w["prompts"][i][1] for i in idx]
    out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=Q.MAX_NEW, return_logits=True, schedule="refill", **MODES[mode])
    stats = lm.queue_stats()
    _equal_to_alone(out, idx, _alone(mode, None), None)
    assert (out.counts == Q.MAX_NEW).all() and stats["dead_rows"] == 0 and stats["admissions"] == 20
    assert stats["rows"] == 20 * Q.MAX_NEW + (0 if mode.startswith("gemm") else sum(e.shape[0] - 1 for e in emb))
    one = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=1, eos_token_id=Q.EOS, return_logits=True, schedule="refill", **MODES[mode])
    alone = _alone(mode, None)
    for n, i in enumerate(idx):
        assert one.tokens[n, 0] == alone[i].tokens[0] and one.logits[n, 0].tobytes() == alone[i].logits[0].tobytes() and one.counts[n] == 1
    stats = lm.queue_stats()
    assert stats["dead_rows"] == 0 and stats["admissions"] == 20 and stats["rows"] == (20 if mode.startswith("gemm") else sum(e.shape[0] for e in emb))
    assert not mode.startswith("gemm") or (stats["steps"], stats["gemm_phases"]) == (2, 2)          # 16 sequences, then 4: a phase and a step each


@pytest.mark.parametrize("mode", list(MODES))
def test_a_sequence_of_nan_embeddings_harms_no_other(mode):
    """Two slots; the second sequence is 20 positions of NaN and runs to the limit; the sequences behind it are shorter than it, and one of them inherits its slot with
    NaN keys and values at every position from its own length on."""
    w, lm = Q.workload(), _model()
    idx = [2, None, 8, 11, 15, 1, 0]
    nan = np.full((20, w["case"].D), np.nan, np.float32)
    assert all(w["prompts"][i][0].shape[0] < 20 for i in idx[2:])
    emb = [nan if i is None else w["prompts"][i][0] for i in idx]
    pos = [None if i is None else w["prompts"][i][1] for i in idx]
    out = lm.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=Q.MAX_NEW, eos_token_id=Q.EOS, return_logits=True, schedule="refill", slots=2, **MODES[mode])
    keep = [n for n, i in enumerate(idx) if i is not None]
    sub = vl.LMOutput(out.tokens[keep], out.counts[keep], out.logits[keep])
    _equal_to_alone(sub, [i for i in idx if i is not None], _alone(mode, Q.EOS), Q.EOS)
    assert np.isnan(out.logits[1]).all() and out.counts[1] == Q.MAX_NEW


def test_two_runs_a_used_model_and_the_groups_schedule_give_the_same_bytes():
    w = Q.workload()
    emb, pos = [p[0] for p in w["prompts"]], [p[1] for p in w["prompts"]]
    mode = MODES["gemm-split"]
    kw = dict(inputs_embeds=emb, position_ids=pos, max_new_tokens=Q.MAX_NEW, eos_token_id=Q.EOS, return_logits=True)
    with vl.CausalLM.from_state_dict(_cfg(w["case"]), w["weights"]) as used, vl.CausalLM.from_state_dict(_cfg(w["case"]), w["weights"]) as fresh:
        assert used.queue_stats()["steps"] == 0
        groups = used.generate(stop_at_eos=True, **kw, **mode)                       # a long ordinary call first: 3 groups, stopping at eos
        before = used.decode_stats()
        a = used.generate(schedule="refill", **kw, **mode)
        assert used.decode_stats() == before and used.queue_stats()["steps"] > 0     # generate's own statistics are untouched by the queued call
        b = used.generate(schedule="refill", **kw, **mode)
        c = fresh.generate(schedule="refill", **kw, **mode)
        for other in (b, c):
            assert other.tokens.tobytes() == a.tokens.tobytes() and other.counts.tobytes() == a.counts.tobytes() and other.logits.tobytes() == a.logits.tobytes()
        assert groups.tokens.tobytes() == a.tokens.tobytes() and groups.counts.tobytes() == a.counts.tobytes()
        for i, k in enumerate(a.counts):
            assert groups.logits[i, :k].tobytes() == a.logits[i, :k].tobytes(), i
        # logits_out serves any number of sequences, and the default schedule is the groups one
        buf = np.full(len(emb) * Q.MAX_NEW * w["case"].vocab + 7, 5.0, np.float32)
        d = used.generate(schedule="refill", logits_out=buf, **{k: v for k, v in kw.items() if k != "return_logits"}, **mode)
        assert d.logits.tobytes() == a.logits.tobytes() and (buf[-7:] == 5.0).all()
        with pytest.raises(api.OCRError):
            used.generate(logits_out=buf, **{k: v for k, v in kw.items() if k != "return_logits"}, **mode)
        for bad in ("queue", "", None):
            with pytest.raises(api.OCRError) as e:
                used.generate(input_ids=[1, 2, 3], max_new_tokens=2, schedule=bad)
            assert e.value.code == api.OAR_INVALID_INPUT
        with pytest.raises(api.OCRError) as e:
            used.generate(input_ids=[1, 2, 3], max_new_tokens=2, schedule="refill", slots=17)
        assert e.value.code == api.OAR_INVALID_INPUT
        ids = used.generate(input_ids=[[1, 2, 3], [4], [5, 6]], max_new_tokens=3, schedule="refill", slots=2)
        ids_groups = used.generate(input_ids=[[1, 2, 3], [4], [5, 6]], max_new_tokens=3)
        assert ids.tokens.tobytes() == ids_groups.tokens.tobytes()


def test_generate_tokens_refills_on_more_than_16_images():
    """The composite case's two images, nine times over: 18 sequences on 16 slots equal the groups schedule's bytes."""
    r = vr.composite_reference()
    vc, lc = r["vis_case"], r["lm_case"]
    cfg_json = dict(hidden_size=lc.D, num_hidden_layers=lc.L, num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, head_dim=lc.head_dim, intermediate_size=lc.F,
                    vocab_size=lc.vocab, rms_norm_eps=lc.eps, rope_theta=lc.theta, rope_scaling=dict(mrope_section=list(lc.mrope_section)), tie_word_embeddings=lc.tie,
                    image_token_id=vr.PA_IDS["image"], vision_start_token_id=vr.PA_IDS["start"],
                    vision_config=dict(hidden_size=vc.D, num_hidden_layers=vc.L, num_attention_heads=vc.heads, intermediate_size=vc.F, patch_size=vc.patch, image_size=vc.G * vc.patch,
                                       spatial_merge_size=vc.merge, layer_norm_eps=vc.eps, hidden_act=vc.act))
    preproc = dict(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096, rescale_factor=1.0 / 255.0, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    images = list(r["images"]) * 9
    n = 6
    eos = int(r["runs"][0][0][2])                                                    # the third token of the first image's run: its copies end there
    with vl.PaddleOCRVL.from_state_dict(cfg_json, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=16), vision_overrides=dict(max_tokens=64, max_images=2)) as m:
        groups = m.generate_tokens(images, vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=n, eos_token_id=eos, return_logits=True)
        refill = m.generate_tokens(images, vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=n, eos_token_id=eos, return_logits=True, schedule="refill")
        stats = m.lm.queue_stats()
    assert refill.tokens.shape == (18, n) and stats["admissions"] == 18
    assert refill.tokens.tobytes() == groups.tokens.tobytes() and refill.counts.tobytes() == groups.counts.tobytes()
    for i, k in enumerate(refill.counts):
        assert refill.logits[i, :k].tobytes() == groups.logits[i, :k].tobytes(), i
    for i, (t64, _, _, _) in enumerate(r["runs"]):
        k = int(refill.counts[i])
        assert np.array_equal(refill.tokens[i, :k], t64[:k])
