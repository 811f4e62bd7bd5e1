"""The logits processors of DESIGN 4.47 on the CPU: the rules' known answers, the numpy-f32 spelling against a brute-force one, the conditions that make the GPU
tests legitimate (synth/lm_logits_cases.py: every pinned seed meets the margin condition, A / E / C the bite condition), and oar_lm_logits_check, which needs no
device, on every refused argument."""
import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_logits_cases as LC
from oar_ocr_amd.synth import lm_reference as R

ROOT = Path(__file__).resolve().parents[1]


def test_known_answers_worked_by_hand():
    assert LC.banned_tokens([7, 8, 9, 7, 8, 5, 7, 8], 3) == {5, 9}
    assert LC.banned_tokens([7, 8], 3) == set()
    assert LC.banned_tokens([7, 8, 9], 0) == set() and LC.banned_tokens([7, 8, 9], 1) == set()
    # the duplicate counts once (6 / 1.5 = 4 < 5, not 6 / 2.25), the id beyond the vocabulary is ignored
    x = LC.process(np.asarray([6, 5, 4, -2], np.float32), [0, 0, 57], 1.5, 0)
    assert x.tolist() == [4.0, 5.0, 4.0, -2.0] and LC.choose(x) == 1
    # a negative seen logit is multiplied: -.5 -> -.75, below -.6
    x = LC.process(np.asarray([-.5, -.6, -.7, -.8], np.float32), [0], 1.5, 0)
    assert x[0] == np.float32(-.5) * np.float32(1.5) and LC.choose(x) == 1
    assert LC.choose(np.asarray([np.nan, 1.0, np.nan, 1.0], np.float32)) == 1 and LC.choose(np.full(5, np.nan, np.float32)) == 0
    assert LC.choose(np.full(4, -np.inf, np.float32)) == 0 and LC.choose(np.asarray([-0.0, 0.0], np.float32)) == 0


def _brute(logits, history, r, n):
    """the rules spelled element by element"""
    x = [np.float32(v) for v in logits]
    V, H = len(x), len(history)
    for t in range(V):
        if any(h == t for h in history):
            x[t] = np.float32(x[t] * np.float32(r)) if x[t] < 0 else np.float32(x[t] / np.float32(r))
    if n > 1 and H >= n:
        for i in range(0, H - n + 1):
            if all(history[i + j] == history[H - n + 1 + j] for j in range(n - 1)):
                t = history[i + n - 1]
                if 0 <= t < V:
                    x[t] = np.float32(-np.inf)
    return np.asarray(x, np.float32)


def test_numpy_process_equals_the_brute_force_spelling():
    rng = np.random.default_rng(11)
    for trial in range(200):
        V = int(rng.integers(2, 40))
        H = int(rng.integers(0, 30))
        n = int(rng.integers(0, 6))
        r = float(rng.choice([1.0, 1.08, 1.3, 2.0]))
        hist = [int(v) for v in rng.integers(0, min(V, 5) + 2, H)]      # few ids: many repeats; some beyond a small vocabulary
        x = (rng.standard_normal(V) * 2).astype(np.float32)
        x[rng.integers(0, V)] = 0.0
        x[rng.integers(0, V)] = -0.0
        if trial % 5 == 0:
            x[rng.integers(0, V)] = np.nan
        with np.errstate(all="ignore"):
            want = _brute(x, hist, r, n)
        got = LC.process(x, hist, r, n)
        assert got.tobytes() == want.tobytes(), (trial, V, hist, r, n)
        got64 = LC.process64(torch.from_numpy(x).double(), hist, r, n).numpy()
        ok = ~np.isnan(want)
        assert np.array_equal(np.isinf(got64), np.isinf(want)) and np.allclose(got64[ok & ~np.isinf(want)], want[ok & ~np.isinf(want)], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", LC.MODEL_CASES)
def test_pinned_seeds_meet_the_margin_and_bite_conditions(name):
    """Margin: at every step the best processed f64 logit leads the second best by more than 4 r tol, tol = max(16 noise, 2^-19): the penalty scales
    a logit's error by up to r, and a seen logit near zero may take either branch.  Bite (A, E, C): the processed token differs from the raw arg-max at 3 or more
    steps of every sequence, and over the case the raw arg-max is banned (n > 1) or loses to the penalty alone (r > 1) at least once."""
    ref = LC.reference_for(name)
    assert ref["tol"] == max(16.0 * ref["noise"], 2.0 ** -19) and ref["noise"] > 0
    cond = LC.conditions(ref)
    assert set(cond) == set(LC.SETTINGS)
    for (r, n), c in cond.items():
        print(f"case {name} seed {LC.SEEDS[name]} r {r} n {n}: tol {ref['tol']:.3e}, least margin {c['margin_ratio']:.2f} x 4 r tol, differing steps >= {c['least_differing']}, "
              f"ban hits {c['ban_hits']}, demoted {c['demoted']}")
        assert c["margin_ratio"] > 1.0, (name, r, n, c)
        if name in LC.BITE_CASES:
            assert c["least_differing"] >= 3, (name, r, n, c)
            assert (n > 1 and c["ban_hits"] >= 1) or (r > 1 and c["demoted"] >= 1), (name, r, n, c)
    for runs in ref["runs"].values():
        for g, (_, _, ids) in zip(runs, ref["prompts"]):
            assert len(g["tokens"]) == LC.STEPS and g["histories"][0] == [int(v) for v in ids]
            assert g["histories"][-1] == [int(v) for v in ids] + [int(t) for t in g["tokens"][:-1]]


def test_forcing_and_eos_in_the_reference_generate():
    ref = LC.reference_for("A")
    emb, pos, ids = ref["prompts"][0]
    r64 = R.RefLM(ref["case"], ref["weights"], torch.float64)
    free = ref["runs"][(1.3, 3)][0]
    forced = np.full(12, -1, np.int64)
    forced[3] = (int(free["tokens"][3]) + 1) % ref["case"].vocab
    g = LC.generate(r64, emb, pos, ids, 12, 1.3, 3, forced_tokens=forced)
    assert np.array_equal(g["tokens"][:4], free["tokens"][:4]) and g["histories"][4][-1] == forced[3]
    eos = int(free["tokens"][5])
    first = int(np.flatnonzero(free["tokens"] == eos)[0])
    g = LC.generate(r64, emb, pos, ids, 12, 1.3, 3, eos_token_id=eos)
    assert np.array_equal(g["tokens"][:first + 1], free["tokens"][:first + 1]) and (g["tokens"][first:] == eos).all()
    off = LC.generate(r64, emb, pos, ids, 12, 1.0, 0)
    plain, _ = r64.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=12)
    assert np.array_equal(off["tokens"], plain)


def test_kernel_cases_cover_what_they_claim():
    cases = LC.kernel_cases()
    assert {c["logits"].shape[1] for c in cases} == set(LC.KERNEL_VOCABS) and {c["logits"].shape[0] for c in cases} >= {1, 3, 16}
    lens = {len(h) for c in cases for h in c["histories"]}
    assert {0, 1, 2, 3, 4, 5, 255, 256, 257, 1030} <= lens
    assert {c["n"] for c in cases} >= {0, 2, 3, 5, 2000} and any(c["n"] > max(len(h) for h in c["histories"]) for c in cases)
    assert any(t >= c["logits"].shape[1] for c in cases for h in c["histories"] for t in h)
    hits_first = hits_last = many = 0
    for c in cases:
        n = c["n"]
        for h in c["histories"]:
            H = len(h)
            if n > 1 and H >= n:
                tail = h[H - n + 1:]
                hits_first += h[:n - 1] == tail
                hits_last += h[H - n:H - 1] == tail
                many += len(LC.banned_tokens(h, n)) >= 4
    assert hits_first >= 5 and hits_last >= 5 and many >= 5
    flat = np.concatenate([c["logits"].reshape(-1) for c in cases if c["logits"].shape[1] <= 1030])
    assert np.isnan(flat).any() and (flat == 0).any() and np.signbit(flat[flat == 0]).any()
    for c in cases:
        want = LC.kernel_expected(c)
        if "equal_maxima" in c:
            for j, (lo, d) in enumerate(c["equal_maxima"]):
                assert want[2 * j] == lo + d and want[2 * j + 1] == lo, (c["name"], j)
        if "banned_but_one" in c["name"]:
            V = c["logits"].shape[1]
            assert want.tolist() == [0, 0, V // 2] and len(LC.banned_tokens(c["histories"][2], 2)) == V - 1
        if "nan_inf" in c["name"]:
            assert np.isnan(c["logits"][0]).all() and np.isinf(c["logits"][1]).all()


# ------------------------------------------------------------------------------------------------ the checks that need no device
def _request(n_seq, lengths, max_new, keep, embeds=False, hidden=64):
    ids = [np.arange(max(int(t), 1), dtype=np.int32) % 7 for t in lengths]
    arrs = [np.zeros((a.size, hidden), np.float32) for a in ids] if embeds else ids
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    ln = np.asarray(lengths, np.int32)
    tokens, counts = np.zeros((max(len(ids), 1), max(max_new, 1)), np.int32), np.zeros(max(len(ids), 1), np.int32)
    keep += [arrs, ptrs, ln, tokens, counts]
    req = vl.LmRequest()
    req.n_seq = n_seq
    req.lengths = ln.ctypes.data_as(C.POINTER(C.c_int32))
    if embeds:
        req.inputs_embeds = C.cast(ptrs, C.POINTER(C.c_void_p))
    else:
        req.input_ids = C.cast(ptrs, C.POINTER(C.c_void_p))
    req.max_new_tokens = max_new
    req.eos_token_id = -1
    req.tokens, req.counts = tokens.ctypes.data, counts.ctypes.data
    return req


def _cfg(**kw):
    c = R.CASES["A"]
    d = dict(hidden_size=c.D, num_hidden_layers=c.L, num_attention_heads=c.heads, num_key_value_heads=c.kv_heads, head_dim=c.head_dim, intermediate_size=c.F,
             vocab_size=c.vocab, mrope_section=list(c.mrope_section), max_positions=64, max_sequences=16)
    d.update(kw)
    return vl.CausalLMConfig(**d).to_c()


def test_argument_checks_need_no_device():
    L = vl._lib()
    keep = []
    cfg = _cfg()
    check = lambda req, lp: L.oar_lm_logits_check(C.byref(cfg), C.byref(req), None if lp is None else C.byref(lp))   # noqa: E731
    ids_req, emb_req = _request(3, [3, 9, 4], 8, keep), _request(3, [3, 9, 4], 8, keep, embeds=True)
    hist = [[1, 2, 500, 1 << 30], [], [3] * 65536]
    # accepted: no processors at all, both off, on with the input ids as history, on with histories of their own (ids beyond the vocabulary, lengths 0 and 65536)
    assert check(ids_req, None) == api.OAR_OK and check(emb_req, None) == api.OAR_OK
    assert check(emb_req, vl._logits_cfg(3, 1.0, 0, None, keep)) == api.OAR_OK and check(emb_req, vl._logits_cfg(3, 1.0, 1, None, keep)) == api.OAR_OK
    assert check(ids_req, vl._logits_cfg(3, 1.3, 3, None, keep)) == api.OAR_OK
    assert check(emb_req, vl._logits_cfg(3, 1.3, 3, hist, keep)) == api.OAR_OK and check(ids_req, vl._logits_cfg(3, 1.0, 2, hist, keep)) == api.OAR_OK
    # refused
    for r in (0.99, 0.0, -1.5, math.inf, math.nan):
        assert check(ids_req, vl._logits_cfg(3, r, 0, None, keep)) == api.OAR_INVALID_INPUT, r
    assert check(ids_req, vl._logits_cfg(3, 1.0, -1, None, keep)) == api.OAR_INVALID_INPUT
    assert check(emb_req, vl._logits_cfg(3, 1.3, 0, None, keep)) == api.OAR_INVALID_INPUT         # embeddings carry no ids
    assert check(emb_req, vl._logits_cfg(3, 1.0, 2, None, keep)) == api.OAR_INVALID_INPUT
    assert check(ids_req, vl._logits_cfg(3, 1.3, 3, [[1], [-1], [2]], keep)) == api.OAR_INVALID_INPUT      # a negative id
    assert check(ids_req, vl._logits_cfg(3, 1.3, 3, [[1], [2], [3] * 65537], keep)) == api.OAR_INVALID_INPUT
    lp = vl._logits_cfg(3, 1.3, 3, hist, keep)
    lp.history_lengths = None                                                                         # ids without lengths
    assert check(ids_req, lp) == api.OAR_INVALID_INPUT
    lp = vl._logits_cfg(3, 1.3, 3, hist, keep)
    lp.history_ids = None
    assert check(ids_req, lp) == api.OAR_INVALID_INPUT
    lp = vl._logits_cfg(3, 1.3, 3, hist, keep)
    C.cast(lp.history_ids, C.POINTER(C.c_void_p))[0] = None                                           # a null entry of non-zero length
    assert check(ids_req, lp) == api.OAR_INVALID_INPUT
    on = vl._logits_cfg(3, 1.3, 3, None, keep)
    assert L.oar_lm_logits_check(None, C.byref(ids_req), C.byref(on)) == api.OAR_INVALID_INPUT and L.oar_lm_logits_check(C.byref(cfg), None, C.byref(on)) == api.OAR_INVALID_INPUT
    assert check(_request(3, [3, 57, 3], 8, keep), on) == api.OAR_INVALID_INPUT                    # what oar_lm_generate refuses: 57 + 8 > 64 positions
    bad = _request(3, [3, 9, 4], 8, keep)
    bad.n_seq = 17
    assert check(bad, on) == api.OAR_INVALID_INPUT
    # the bans of a row are an LDS bitmap: a vocabulary above 2^19 runs the penalty alone
    big = _cfg(vocab_size=(1 << 19) + 1)
    assert L.oar_lm_logits_check(C.byref(big), C.byref(ids_req), C.byref(vl._logits_cfg(3, 1.3, 2, None, keep))) == api.OAR_UNSUPPORTED_OP
    assert L.oar_lm_logits_check(C.byref(big), C.byref(ids_req), C.byref(vl._logits_cfg(3, 1.3, 0, None, keep))) == api.OAR_OK
    # entries that need a model or buffers refuse nulls before they look for a device
    assert L.oar_lm_generate_ex(None, C.byref(ids_req), C.byref(on)) == api.OAR_INVALID_INPUT
    assert L.oar_k_lm_select(None, 1, 33, None, None, 1.0, 0, None, 0, 0) == api.OAR_INVALID_INPUT
    x, ln, tok = np.zeros((1, 33), np.float32), np.zeros(1, np.int32), np.zeros(4, np.int32)
    p = (C.c_void_p * 1)(None)
    sel = lambda rows, V, r, n, nt, off: L.oar_k_lm_select(api._p(x), rows, V, api._p(ln), p, r, n, api._p(tok), nt, off)   # noqa: E731
    for args in ((0, 33, 1.0, 0, 4, 0), (17, 33, 1.0, 0, 4, 0), (1, 1, 1.0, 0, 4, 0), (1, 1 << 24, 1.0, 0, 4, 0), (1, 33, 0.5, 0, 4, 0), (1, 33, 1.0, -2, 4, 0),
                 (1, 33, 1.0, 0, 4, 4), (1, 33, 1.0, 0, 4, 5)):
        assert sel(*args) == api.OAR_INVALID_INPUT, args


def test_python_refuses_the_refill_schedule_with_a_processor_before_anything_runs():
    lm = vl.CausalLM(vl.CausalLMConfig(64, 2, 4, 2, 16, 96, 97), None)     # no handle: anything that reached the library would fail differently
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2)):
        with pytest.raises(api.OCRError) as e:
            lm.generate(input_ids=[1, 2, 3], max_new_tokens=4, schedule="refill", **kw)
        assert e.value.code == api.OAR_UNSUPPORTED_OP


def test_generation_defaults_come_from_generation_config_json(tmp_path):
    assert vl.read_generation_defaults(tmp_path) == {}
    (tmp_path / "generation_config.json").write_text(json.dumps({"repetition_penalty": 1.05, "no_repeat_ngram_size": 35, "eos_token_id": [2, 7], "do_sample": False, "top_p": None}))
    assert vl.read_generation_defaults(tmp_path) == {"repetition_penalty": 1.05, "no_repeat_ngram_size": 35, "eos_token_id": [2, 7]}
    assert vl.CausalLM(vl.CausalLMConfig(64, 2, 4, 2, 16, 96, 97), None).generation_defaults == {}


def test_composite_case_with_processors_is_greedy_safe():
    """composite case PA with PA_SETTING (tests/test_gpu_lm_logits.py): every step's processed f64 margin exceeds 4 r tol, and the processors change the tokens"""
    p = LC.composite_reference()
    r, n = LC.PA_SETTING
    for g in p["runs"]:
        assert g["margin"].min() > 4.0 * r * p["tol"] and int((g["tokens"] != g["raw_argmax"]).sum()) >= 3
