"""Every route of the recognizer's CTC tail against float64, with the route that ran asserted.

The matrix, the Python restatement of the route rule and the references live in oar_ocr_amd/synth/ctc_tail_cases.py.  A case is one ordinary recognition
call through api.TextRecognitionPredictor on a recognizer of one feature layer: the features come from the engine on the graph cut in front of the
Linear (and are known exactly: the layer selects pixels), so the (index, probability) pairs are compared with the float64 soft-max of the float64 head
on those features.  Per case: the route's profiler classes ran and the excluded ones did not; two calls agree byte for byte; every probability lies
within tol = max(4 noise, 2^-21 p) of float64 (noise: two honest f32 evaluations of the same soft-max); the index is float64's wherever its runner-up
lies further below than tol; no index reaches the padding.  Designed rows (w = 0: the logits are the bias in every kernel) give their stated index.
The cases of a process switch run in ONE child per switch (the switches are read once), each under its own time limit; a failed child ends the
module's GPU work."""
import shutil

import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import ctc_tail_cases as C
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth import x6_cases as X
from oar_ocr_amd.synth.child_run import RecResult, recognize_many_in_child

pytestmark = pytest.mark.gpu
_RUNS = {}      # env -> {job key: RecResult}: the environment's child ran (once: a failed child is not started again)

HERE = [c for c in C.CASES if not c.env]
CHILD = [c for c in C.CASES if c.env]


@pytest.fixture(scope="module")
def workroot(tmp_path_factory):
    root = tmp_path_factory.mktemp("ctc_tail")
    yield root
    shutil.rmtree(root, ignore_errors=True)


def _lg(v):
    return f"2^{np.log2(v):.1f}" if v > 0 else "0"


def _recognize(model, V, crops):
    """one predictor, two calls, in this process"""
    pred = api.TextRecognitionPredictor(model, api.read_dict(models.synth_dict(V - 2)))
    try:
        api.prof_enable(True); api.prof_reset()
        first = pred.predict(crops)
        again = pred.predict(crops)
        names = {e["name"] for e in api.prof_snapshot() if e["launches"]}
    finally:
        api.prof_enable(False)
        pred.close()
    same = first.indices.tobytes() == again.indices.tobytes() and first.probs.tobytes() == again.probs.tobytes()
    return RecResult(first.indices, first.probs, names, same)


def _features(c, crops, sel, fb):
    """the head's input as the engine computes it -- and as the selecting layer must: exactly its input's pixels"""
    x = api.k_rec_preprocess(crops)
    eng = api.OrtInfer(C.ctc_model(c.K, c.V, sel, fb, None, None, head=False))
    try:
        F = eng.infer(x)[0][1].reshape(-1, c.K)
    finally:
        eng.close()
    assert x.shape == (c.crops, 3, 48, c.width) and F.shape == (c.M, c.K), (x.shape, F.shape)
    assert np.array_equal(F, X.ctc_select(x, sel, fb))
    assert np.abs(x - X.ctc_pixels(crops)).max() <= 1e-6
    return x, F


def _judge(c, label, res, F, w, b, tie=(), answer=None):
    """one recognition result against the route's classes and the float64 bounds"""
    p = c.plan()
    detail = c.envd.get("OAR_PROF_DETAIL") == "1"
    missing, forbidden = C.classes_ran(p, res.names, c.M, c.K, detail)
    assert not missing and not forbidden, (c.name, label, p.route, "missing", missing, "must not run", forbidden, sorted(res.names))
    assert res.same, (c.name, label, "two calls on the same crops differ")
    assert res.indices.shape == (c.crops, c.T) and res.probs.shape == (c.crops, c.T), (res.indices.shape, c.crops, c.T)
    B = C.bounds(F, w, b, tie)
    r = C.check(B, res.indices, res.probs, c.V)
    ran = sorted({n.split(" ")[0] for n in res.names} & (p.must | {"conv_igemm_x6"}))      # (conv_igemm_x6: the detail spelling of conv_igemm_ws_x6)
    print(f"\n[ctc] {c.name} | {label} | {p.route} {'+'.join(ran)} | noise {_lg(B['noise'])} | tol {_lg(float(B['tol'].max()))} | err {_lg(r['err'])} | err/tol {r['ratio']:.3f}"
          f" | clear {B['clear'].mean():.3f}")
    assert np.isfinite(res.probs).all() and r["ratio"] <= 1.0, (c.name, label, r["err"], r["ratio"])
    assert len(r["out_of_range"]) == 0, (c.name, label, "index outside the vocabulary", r["out_of_range"][:8], res.indices.reshape(-1)[r["out_of_range"][:8]])
    assert len(r["bad_index"]) == 0, (c.name, label, r["bad_index"][:8], res.indices.reshape(-1)[r["bad_index"][:8]], B["idx"][r["bad_index"][:8]])
    if answer is None:
        assert B["clear"].mean() >= 0.9, (c.name, B["clear"].mean())
    else:
        assert B["clear"].all() and (res.indices == answer).all(), (c.name, label, answer, np.unique(res.indices))
    return B


# ------------------------------------------------------------------------------------------------ the default environment, in this process
@pytest.mark.parametrize("name", [c.name for c in HERE if c.family != "designed"])
def test_ctc_tail_route(name):
    c = C.case_by_name(name)
    crops, sel, fb, w, b = C.inputs(c)
    _, F = _features(c, crops, sel, fb)
    res = _recognize(C.ctc_model(c.K, c.V, sel, fb, w, b, spelling=c.spelling), c.V, crops)
    _judge(c, c.family, res, F, w, b)


@pytest.mark.parametrize("name", [c.name for c in HERE if c.family == "designed"])
def test_ctc_tail_designed_rows(name):
    """w = 0: the logits are the bias.  The repeated maximum's later column wins wherever the pair sits (one fragment, two tiles, one ctc_combine lane,
    two lanes, the ragged last tile); a maximum of exactly 0.0 does not lose to the padding's 0; columns 0 and V - 1 are found; twin weight columns tie"""
    c = C.case_by_name(name)
    crops, sel, fb, rows = C.designed_rows(c)
    _, F = _features(c, crops, sel, fb)
    for r in rows:
        res = _recognize(C.ctc_model(c.K, c.V, sel, fb, r.w, r.b, spelling=c.spelling), c.V, crops)
        _judge(c, r.name, res, F, r.w, r.b, r.tie, r.answer)


# ------------------------------------------------------------------------------------------------ the process switches, one child each
def _jobs(c):
    if c.family == "designed":
        crops, sel, fb, rows = C.designed_rows(c)
        for r in rows:
            yield (c.name, r.name), C.ctc_model(c.K, c.V, sel, fb, r.w, r.b, spelling=c.spelling), crops
    else:
        crops, sel, fb, w, b = C.inputs(c)
        yield (c.name, c.family), C.ctc_model(c.K, c.V, sel, fb, w, b, spelling=c.spelling), crops


def _runs(env, workroot):
    if env not in _RUNS:
        assert None not in _RUNS.values(), "an earlier child failed: no further GPU work is started by this module"
        _RUNS[env] = None
        keys, jobs = [], []
        for c in C.env_groups()[env]:
            for key, m, crops in _jobs(c):
                keys.append(key)
                jobs.append((m, c.V, crops))
        res = recognize_many_in_child(jobs, dict(env), workroot / f"child{len(_RUNS)}", timeout=240.0)
        _RUNS[env] = dict(zip(keys, res))
    assert _RUNS[env] is not None, f"the child of {env} failed in an earlier test"
    return _RUNS[env]


@pytest.mark.parametrize("name", [c.name for c in CHILD])
def test_ctc_tail_route_under_a_switch(name, workroot):
    c = C.case_by_name(name)
    runs = _runs(c.env, workroot)
    if c.family == "designed":
        crops, sel, fb, rows = C.designed_rows(c)
        _, F = _features(c, crops, sel, fb)
        for r in rows:
            _judge(c, r.name, runs[(name, r.name)], F, r.w, r.b, r.tie, r.answer)
    else:
        crops, sel, fb, w, b = C.inputs(c)
        _, F = _features(c, crops, sel, fb)
        _judge(c, f"{c.family} {dict(c.env)}", runs[(name, c.family)], F, w, b)


# ------------------------------------------------------------------------------------------------ the OrtInfer seam: the whole probability tensor
@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.seam])
def test_ortinfer_seam_probabilities(name):
    """softmax_wave_kernel (V <= 1024) and softmax_block_kernel (above) write every probability: each within tol_full of float64 relative to its row's
    largest, the row sums within tol_sum of 1; and the recognizer seam's index is k_ctc_argmax of these probabilities on the clear rows (not bit
    equality: the partial epilogue's tie set is __expf's)"""
    c = C.case_by_name(name)
    crops, sel, fb, w, b = C.inputs(c)
    x, F = _features(c, crops, sel, fb)
    model = C.ctc_model(c.K, c.V, sel, fb, w, b, spelling=c.spelling)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_enable(True); api.prof_reset()
        y = eng.infer(x)[0][1]
        again = eng.infer(x)[0][1]
        names = {e["name"] for e in api.prof_snapshot() if e["launches"]}
    finally:
        api.prof_enable(False)
        eng.close()
    assert "softmax" in names and not names & {"softmax_argmax", "ctc_combine", "ctc_head_x6"}, sorted(names)
    assert y.shape == (c.crops, c.T, c.V) and y.tobytes() == again.tobytes()
    B = C.bounds(F, w, b)
    P = B["P"]
    y2 = y.reshape(c.M, c.V).astype(np.float64)
    err = float((np.abs(y2 - P) / P.max(-1, keepdims=True)).max())
    esum = float(np.abs(y2.sum(-1) - 1.0).max())
    print(f"\n[ctc] {c.name} | OrtInfer seam V={c.V} | noise_full {_lg(B['noise_full'])} | tol_full {_lg(B['tol_full'])} | err {_lg(err)} | err/tol {err / B['tol_full']:.3f}"
          f" | row sums: tol {_lg(B['tol_sum'])} err {_lg(esum)} err/tol {esum / B['tol_sum']:.3f}")
    assert np.isfinite(y).all() and err <= B["tol_full"], (name, err, B["tol_full"])
    assert esum <= B["tol_sum"], (name, esum, B["tol_sum"])
    ki, kp = api.k_ctc_argmax(y)
    clear = B["clear"]
    assert np.array_equal(ki[clear], B["idx"][clear]) and (np.abs(kp.astype(np.float64) - B["p"]) <= B["tol"]).all()
    fused = _recognize(model, c.V, crops)
    assert np.array_equal(fused.indices.reshape(-1)[clear], ki[clear]), name
    assert (np.abs(fused.probs.reshape(-1).astype(np.float64) - kp) <= 2.0 * B["tol"]).all()      # (both within tol of float64)
