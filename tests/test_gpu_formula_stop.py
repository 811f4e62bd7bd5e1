"""The stop token of the FormulaDecode operator (`OrtInfer.set_decode_stop`): a chunk of <= 16 images ends after the last step at which one of its
images was still decoding, every row reads the stop token after its first one, and with the setting off nothing differs from the plain decode.

Reference: `formula_reference_bundle` (torch on the CPU, f64 and f32), run free for all M steps; weights `formula_weights(seed=0)`, memory
`default_rng(1000).standard_normal((B, S, D))` -- the helpers of test_gpu_formula_decode.py, restated.  Each case first asserts on the reference alone that
gap >= 8 tol (tol = max(16 noise, 2^-19), as there) and that the stop token first occurs where the table says; then, with f_b the first occurrence in image b
(M - 1 where there is none) and t_stop the largest f_b of a chunk:
  token_ids[b, :f_b + 1] are the reference's, token_ids[b, f_b + 1:] are the stop token, the logits rows t <= f_b are within tol of the f64 logits;
  steps_executed == sum over chunks of (t_stop + 1), exactly; steps_enqueued <= sum over chunks of min(M, t_stop + 1 + lookahead);
  the profiler counts steps_enqueued * (8 Ld + 2) launches of class formula_decode, on a first and on a second infer;
  with the stop off -- before it was ever set, and again after set_decode_stop(-1) -- every position equals the reference and steps_executed == M * chunks."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_reference_bundle

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SEED = 0
#         D  nh   F   V Ld   S    M   B
SMALL = (24, 3, 40, 37, 1, 9, 96, 5)
DEEP = (40, 5, 72, 61, 2, 37, 160, 3)
WIDE = (24, 3, 40, 37, 1, 9, 64, 17)              # two chunks: 16 rows and 1 row
#        shape, stop token, first occurrence per image (None: absent)
CASES = [(SMALL, 15, [55, 8, 13, 7, 15]),                                                               # all distinct: the chunk ends after step 55 of 96
         (SMALL, 11, [18, 7, 7, 6, 14]),                                                                # two images finish in one step
         (SMALL, 9, [None] * 5),                                                                        # never stops
         (DEEP, 51, [7, 24, 7]),                                                                        # two layers
         (WIDE, 34, [16, 22, 8, 12, 12, 12, 8, 12, 11, 5, 19, 22, 8, 23, 14, 8, 8]),                    # chunks end at steps 23 (image 13) and 8
         (WIDE, 16, [0] * 17)]                                                                          # everything ends at step 0
IDS = ["distinct", "two_in_one_step", "never", "two_layers", "two_chunks", "step_0"]


def _memory(shape):
    D, nh, F, V, Ld, S, M, B = shape
    return np.random.default_rng(1000 + SEED).standard_normal((B, S, D)).astype(np.float32)


_cache = {}


def _case(shape):
    """model, memory and reference bundle of one shape: computed once, never modified"""
    if shape not in _cache:
        D, nh, F, V, Ld, S, M, B = shape
        model, info = models.build_formulanet(D=D, nh=nh, F=F, V=V, Ld=Ld, M=M, seed=SEED, head_only=True, with_logits=True)
        mem = _memory(shape)
        _cache[shape] = (model, mem, formula_reference_bundle(info["weights"], mem, M))
    return _cache[shape]


def _first(tokens, e):
    return [int(np.nonzero(r == e)[0][0]) if np.any(r == e) else None for r in tokens]


def _check_plain(outs, ref, st, shape, label):
    D, nh, F, V, Ld, S, M, B = shape
    chunks = (B + 15) // 16
    assert np.array_equal(outs["token_ids"], ref["tokens"]), (label, np.argwhere(outs["token_ids"] != ref["tokens"])[:4])
    err = float(np.abs(outs["logits"].astype(np.float64) - ref["logits"]).max())
    assert err <= ref["tol"], (label, err, ref["tol"])
    assert (st.steps_limit, st.steps_enqueued, st.steps_executed) == (M * chunks,) * 3, (label, st)


@pytest.mark.parametrize("shape,e,first", CASES, ids=IDS)
def test_stop_token(shape, e, first):
    D, nh, F, V, Ld, S, M, B = shape
    model, mem, ref = _case(shape)
    tol = ref["tol"]
    assert ref["gap"] >= 8 * tol, ("the reference itself is ill conditioned for this seed", ref["gap"], tol)
    assert _first(ref["tokens"], e) == first
    f = [M - 1 if v is None else v for v in first]
    chunks = [range(c0, min(c0 + 16, B)) for c0 in range(0, B, 16)]
    t_stop = [max(f[b] for b in ch) for ch in chunks]
    want_executed = sum(t + 1 for t in t_stop)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_enable(False)
        _check_plain(dict(eng.infer(mem)), ref, eng.decode_stats(), shape, "before the stop token was set")
        eng.set_decode_stop(e)
        for run in ("first", "second"):
            api.prof_reset()
            api.prof_enable(True)
            outs = dict(eng.infer(mem))
            snap = {x["name"]: x for x in api.prof_snapshot()}
            api.prof_enable(False)
            st = eng.decode_stats()
            ids = outs["token_ids"]
            err = max(float(np.abs(outs["logits"][b, :f[b] + 1].astype(np.float64) - ref["logits"][b, :f[b] + 1]).max()) for b in range(B))
            bound = sum(min(M, t + 1 + st.lookahead) for t in t_stop)
            print(f"{shape} e = {e} ({run}): {st} | want executed {want_executed}, enqueued <= {bound} | logits err {err:.2e} tol {tol:.2e} | "
                  f"formula_decode launches {snap.get('formula_decode', {}).get('launches')} formula_stop {snap.get('formula_stop', {}).get('launches')}")
            assert ids.shape == (B, M) and ids.dtype == np.int64
            for b in range(B):
                assert np.array_equal(ids[b, :f[b] + 1], ref["tokens"][b, :f[b] + 1]), (run, b, ids[b], ref["tokens"][b])
                assert np.all(ids[b, f[b] + 1:] == e), (run, b, ids[b])
            assert err <= tol, (run, err, tol)
            assert st.steps_limit == M * len(chunks) and st.lookahead >= 1
            assert st.steps_executed == want_executed, (run, st, want_executed)
            assert want_executed <= st.steps_enqueued <= bound, (run, st, bound)
            assert snap["formula_decode"]["launches"] == st.steps_enqueued * (8 * Ld + 2), (run, snap["formula_decode"], st)
        eng.set_decode_stop(-1)
        _check_plain(dict(eng.infer(mem)), ref, eng.decode_stats(), shape, "after set_decode_stop(-1)")
    finally:
        api.prof_enable(False)
        eng.close()


def test_never_stopping_equals_the_plain_decode_everywhere():
    """the stop token occurs nowhere: tokens AND every logits row equal the run with the stop off bit for bit, and all 96 steps are executed"""
    shape, e, first = CASES[2]
    model, mem, ref = _case(shape)
    assert _first(ref["tokens"], e) == first
    eng = api.OrtInfer(model)
    try:
        plain = dict(eng.infer(mem))
        eng.set_decode_stop(e)
        stopped = dict(eng.infer(mem))
        st = eng.decode_stats()
        assert np.array_equal(plain["token_ids"], stopped["token_ids"]) and np.array_equal(plain["logits"], stopped["logits"])
        assert (st.steps_limit, st.steps_enqueued, st.steps_executed) == (96, 96, 96), st
    finally:
        eng.close()


def test_invalid_stop_tokens_are_refused():
    shape = SMALL
    model, mem, ref = _case(shape)
    eng = api.OrtInfer(model)
    try:
        with pytest.raises(api.OCRError) as ex:
            eng.set_decode_stop(shape[3])                     # V itself: the first id outside the vocabulary
        assert ex.value.code == api.OAR_INVALID_INPUT, str(ex.value)
        eng.set_decode_stop(shape[3] - 1)                     # the last id inside it
    finally:
        eng.close()
    det, _ = models.build_det("tiny", seed=0)                 # a graph without a decode Loop
    eng = api.OrtInfer(det)
    try:
        with pytest.raises(api.OCRError) as ex:
            eng.set_decode_stop(0)
        assert ex.value.code == api.OAR_INVALID_INPUT, str(ex.value)
        st = eng.decode_stats()
        assert (st.steps_limit, st.steps_enqueued, st.steps_executed, st.lookahead) == (0, 0, 0, 0)
    finally:
        eng.close()


def test_captured_replay_skips_on_the_device():
    """OAR_HIP_GRAPH=1 in a child process (tools/formula_stop_check.py: the first case, three infers -- plain, capture, replay): a captured graph reads nothing
    back, so all 96 steps are enqueued and the device guard alone skips the 40 after step 55; the tokens are those of the uncaptured runs"""
    runs = {}
    for graph in ("0", "1"):
        env = dict(os.environ, OAR_HIP_GRAPH=graph)
        r = subprocess.run([sys.executable, str(ROOT / "tools" / "formula_stop_check.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[graph] = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("DIGEST")]      # [run, digest, executed, enqueued]
    print(runs)
    assert len(runs["0"]) == 3 and len(runs["1"]) == 3
    assert len({x[1] for x in runs["0"] + runs["1"]}) == 1, runs
    assert all(int(x[2]) == 56 for x in runs["0"] + runs["1"]), runs
    assert all(56 <= int(x[3]) < 96 for x in runs["0"]), runs
    assert int(runs["1"][2][2]) == 56 and int(runs["1"][2][3]) == 96, runs
