"""Squeeze attention in the FormulaDecode operator (UniMERNet's MBart decoder): the self-attention queries and keys are projected to D / r, the
values to D, so the key cache is [B, nh, t, dh / r] and the scale (dh / r)^-0.5.  The graphs are synth.models.build_formulanet(qk_squeeze=r).

Reference and order of assertions as in test_gpu_formula_decode.py: the recurrence in torch on the CPU in f64 and f32 (synth/formula_reference.py), weights
formula_weights(seed=0, qk_squeeze=r), memory default_rng(1000).standard_normal((B, S, D)); per case
  1. on the reference alone: every step's top-1 / top-2 logit gap >= 8 tol, tol = max(16 noise, 2^-19), no step excluded
  2. the GPU's token_ids equal the f64 tokens at every position
  3. max |logits - f64| <= tol
The measured figures are printed (pytest -s) and recorded in DESIGN 4.33."""
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
#            D   nh    F     V  Ld    S   M   B  r
SHAPES = [(24, 3, 40, 37, 1, 9, 12, 5, 2),                 # dq = 4, nothing a multiple of 16
          (40, 5, 72, 61, 2, 37, 40, 3, 2),                # two layers
          (64, 4, 128, 300, 2, 50, 70, 2, 2),              # the cache passes 64 positions
          (48, 2, 64, 37, 1, 9, 6, 17, 4),                 # dq = 6, dh = 24: no power of two; two chunks
          (1024, 16, 4096, 4099, 1, 144, 16, 2, 2)]        # one UniMERNet-sized layer
IDS = ["D%d_nh%d_F%d_V%d_Ld%d_S%d_M%d_B%d_r%d" % s for s in SHAPES]
SEED = 0


def _memory(shape):
    D, nh, F, V, Ld, S, M, B, r = shape
    return np.random.default_rng(1000 + SEED).standard_normal((B, S, D)).astype(np.float32)


def _build(shape, **kw):
    D, nh, F, V, Ld, S, M, B, r = shape
    return models.build_formulanet(D=D, nh=nh, F=F, V=V, Ld=Ld, M=M, seed=SEED, head_only=True, with_logits=True, **dict(dict(qk_squeeze=r), **kw))


_cache = {}


def _case(shape):
    """model, memory, reference bundle: computed once, never modified"""
    if shape not in _cache:
        model, info = _build(shape)
        mem = _memory(shape)
        _cache[shape] = (model, mem, formula_reference_bundle(info["weights"], mem, shape[6]))
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_squeeze_decode_matches_the_f64_recurrence_and_its_launch_count(shape):
    D, nh, F, V, Ld, S, M, B, r = shape
    model, mem, ref = _case(shape)
    per_infer = M * ((B + 15) // 16) * (8 * Ld + 2)
    eng = api.OrtInfer(model, profile=True)
    try:
        launches = []
        for run in range(2):                 # (the second infer of a plan may replay it as a captured graph: the same launches)
            api.prof_reset()
            api.prof_enable(True)
            outs = dict(eng.infer(mem))
            launches.append({e["name"]: e for e in api.prof_snapshot()}.get("formula_decode", {}).get("launches"))
            api.prof_enable(False)
    finally:
        api.prof_enable(False)
        eng.close()
    assert outs["token_ids"].shape == (B, M) and outs["token_ids"].dtype == np.int64 and outs["logits"].shape == (B, M, V)
    tol = ref["tol"]
    err = float(np.abs(outs["logits"].astype(np.float64) - ref["logits"]).max())
    print(f"{shape}: noise {ref['noise']:.2e} | tol {tol:.2e} | gap {ref['gap']:.2e} token changes {ref['changes']} | gpu err logits {err:.2e} | launches {launches}")
    assert ref["gap"] >= 8 * tol, ("the reference itself is ill conditioned for this seed", ref["gap"], tol)
    assert np.array_equal(outs["token_ids"], ref["tokens"]), ("tokens differ at (image, step)", np.argwhere(outs["token_ids"] != ref["tokens"])[:4])
    assert err <= tol, (err, tol)
    assert launches == [per_infer, per_infer], (launches, per_infer)


#         D  nh   F   V Ld   S   M  B  dq        (dh = 8: the queries and keys are WIDER than the values' heads, nh dq = 128 > D)
WIDE_QK = [(64, 8, 96, 61, 2, 20, 24, 3, 16),        # three images: a q row of 128 floats must not run into the next image's
           (64, 8, 96, 61, 1, 20, 12, 1, 16)]        # one image: nor into the attention output behind the q buffer


@pytest.mark.parametrize("shape", WIDE_QK, ids=["B3", "B1"])
def test_query_and_key_heads_wider_than_the_value_heads(shape):
    """1 <= dq <= 128 holds whatever dh is: Wq / Wk [nh dq, D] with dq = 2 dh.  The q row buffer has rows of max(D, nh dq) floats.  Same three assertions."""
    D, nh, F, V, Ld, S, M, B, dq = shape
    w = models.formula_weights(D, nh, F, V, Ld, M + 2, SEED, qk_head=dq)
    assert w["l0_wq"].shape == (nh * dq, D) and w["l0_wk"].shape == (nh * dq, D) and w["l0_wv"].shape == (D, D)
    model, info = models.build_formulanet(D=D, nh=nh, F=F, V=V, Ld=Ld, M=M, seed=SEED, head_only=True, with_logits=True, weights=w)
    mem = np.random.default_rng(1000 + SEED).standard_normal((B, S, D)).astype(np.float32)
    ref = formula_reference_bundle(info["weights"], mem, M)
    outs = []
    for _ in range(2):                       # two loads: a race between workgroups would not repeat bit for bit
        eng = api.OrtInfer(model)
        try:
            outs.append(dict(eng.infer(mem)))
        finally:
            eng.close()
    tol = ref["tol"]
    err = float(np.abs(outs[0]["logits"].astype(np.float64) - ref["logits"]).max())
    print(f"dq > dh {shape}: noise {ref['noise']:.2e} | tol {tol:.2e} | gap {ref['gap']:.2e} token changes {ref['changes']} | gpu err logits {err:.2e}")
    assert ref["gap"] >= 8 * tol and ref["changes"] >= B * (M - 1) // 2, ("the reference itself is ill conditioned for this seed", ref["gap"], tol, ref["changes"])
    assert np.array_equal(outs[0]["token_ids"], ref["tokens"]), ("tokens differ at (image, step)", np.argwhere(outs[0]["token_ids"] != ref["tokens"])[:4])
    assert err <= tol, (err, tol)
    assert np.array_equal(outs[0]["logits"], outs[1]["logits"]) and np.array_equal(outs[0]["token_ids"], outs[1]["token_ids"])


def test_query_heads_beyond_the_kernels_limits_are_refused_by_name():
    """dq = 129 > 128, and nh dq = 1040 > 1024: both name the Loop and the limit"""
    for nh, dq in ((2, 129), (8, 130)):
        w = models.formula_weights(64, nh, 96, 61, 1, 6, SEED, qk_head=dq)
        model, _ = models.build_formulanet(D=64, nh=nh, F=96, V=61, Ld=1, M=4, head_only=True, weights=w)
        with pytest.raises(api.OCRError) as ex:
            api.OrtInfer(model)
        assert ex.value.code == api.OAR_UNSUPPORTED_OP and "Loop (" in str(ex.value) and f"head size {dq}" in str(ex.value) and "1 <= dq <= 128" in str(ex.value), str(ex.value)


def test_squeeze_with_the_stop_token():
    """the stop token touches no attention code: rows equal the reference up to their first stop token and read it afterwards; the chunk ends where its last
    image does.  The token and its first occurrences come from the f64 reference: what image 0 emits at step M // 2."""
    shape = SHAPES[1]
    D, nh, F, V, Ld, S, M, B, r = shape
    model, mem, ref = _case(shape)
    assert ref["gap"] >= 8 * ref["tol"]
    e = int(ref["tokens"][0, M // 2])
    f = [int(np.nonzero(row == e)[0][0]) if np.any(row == e) else M - 1 for row in ref["tokens"]]
    assert f[0] <= M // 2
    eng = api.OrtInfer(model)
    try:
        eng.set_decode_stop(e)
        outs = dict(eng.infer(mem))
        st = eng.decode_stats()
    finally:
        eng.close()
    print(f"stop token {e}: first occurrences {f}, {st}")
    for b in range(B):
        assert np.array_equal(outs["token_ids"][b, :f[b] + 1], ref["tokens"][b, :f[b] + 1]) and np.all(outs["token_ids"][b, f[b] + 1:] == e), (b, outs["token_ids"][b])
        assert float(np.abs(outs["logits"][b, :f[b] + 1].astype(np.float64) - ref["logits"][b, :f[b] + 1]).max()) <= ref["tol"]
    assert st.steps_executed == max(f) + 1 and max(f) + 1 <= st.steps_enqueued <= min(M, max(f) + 1 + st.lookahead), st


def test_squeeze_under_capture_in_a_child_process():
    """tools/formula_stop_check.py --squeeze 2 --stop 3 with OAR_HIP_GRAPH=0 and =1 (three infers each: plain, capture, replay).  The f64 reference of the
    tool's head (D 24, nh 3, F 40, V 37, Ld 1, S 9, M 96, B 5, seed 0) first emits token 3 at steps [9, 19, 16, 19, 10]: 20 steps are executed everywhere,
    one digest of the tokens -- the reference's, with 3 behind each row's first -- and the replay enqueues all 96 steps and skips on the device"""
    import hashlib
    D, nh, F, V, Ld, S, M, B, e = 24, 3, 40, 37, 1, 9, 96, 5, 3
    w = models.formula_weights(D, nh, F, V, Ld, M + 2, 0, qk_squeeze=2)
    ref = formula_reference_bundle(w, np.random.default_rng(1000).standard_normal((B, S, D)).astype(np.float32), M)
    assert ref["gap"] >= 8 * ref["tol"]
    want = ref["tokens"].copy()
    first = [int(np.nonzero(row == e)[0][0]) for row in want]
    assert first == [9, 19, 16, 19, 10]
    for b in range(B):
        want[b, first[b] + 1:] = e
    digest = hashlib.sha1(np.ascontiguousarray(want.astype(np.int64)).tobytes()).hexdigest()
    runs = {}
    for graph in ("0", "1"):
        env = dict(os.environ, OAR_HIP_GRAPH=graph)
        r = subprocess.run([sys.executable, str(ROOT / "tools" / "formula_stop_check.py"), "--squeeze", "2", "--stop", str(e)], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[graph] = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("DIGEST")]      # [run, digest, executed, enqueued]
    print(runs)
    assert len(runs["0"]) == 3 and len(runs["1"]) == 3
    assert {x[1] for x in runs["0"] + runs["1"]} == {digest}, (runs, digest)
    assert all(int(x[2]) == 20 for x in runs["0"] + runs["1"]), runs
    assert all(20 <= int(x[3]) < 96 for x in runs["0"]), runs
    assert int(runs["1"][2][3]) == 96, runs


def test_squeezed_cross_attention_is_refused_by_name():
    model, _ = models.build_formulanet(D=24, nh=3, F=40, V=37, Ld=1, M=4, head_only=True, qk_squeeze=2, cross_squeeze=True)
    with pytest.raises(api.OCRError) as ex:
        api.OrtInfer(model)
    msg = str(ex.value)
    assert ex.value.code == api.OAR_UNSUPPORTED_OP and "Loop (" in msg and "body node '" in msg and "squeeze attention is supported in the self-attention only" in msg, msg


def test_mismatched_query_and_key_widths_are_refused():
    w = models.formula_weights(24, 3, 40, 37, 1, 6, 0, qk_squeeze=2)
    wk = models.formula_weights(24, 3, 40, 37, 1, 6, 0)
    w["l0_wk"], w["l0_bk"] = wk["l0_wk"], wk["l0_bk"]                    # Wq [12, 24] but Wk [24, 24]
    model, _ = models.build_formulanet(D=24, nh=3, F=40, V=37, Ld=1, M=4, head_only=True, weights=w)
    with pytest.raises(api.OCRError) as ex:
        api.OrtInfer(model)
    assert ex.value.code == api.OAR_UNSUPPORTED_OP and "Loop (" in str(ex.value) and "same row count" in str(ex.value), str(ex.value)


def test_no_squeeze_is_the_same_operator_on_every_load():
    """qk_squeeze = 1 writes the graph it always wrote (its values: test_gpu_formula_decode.py); two loads give bit-identical outputs"""
    shape = (40, 5, 72, 61, 2, 37, 40, 3, 1)
    model, _ = _build(shape)
    D, nh, F, V, Ld, S, M, B, r = shape
    assert model == models.build_formulanet(D=D, nh=nh, F=F, V=V, Ld=Ld, M=M, seed=SEED, head_only=True, with_logits=True)[0]
    outs = []
    for _ in range(2):
        eng = api.OrtInfer(model)
        try:
            outs.append(dict(eng.infer(_memory(shape))))
        finally:
            eng.close()
    assert np.array_equal(outs[0]["token_ids"], outs[1]["token_ids"]) and np.array_equal(outs[0]["logits"], outs[1]["logits"])
