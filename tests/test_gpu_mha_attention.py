"""Multi-head attention with separate q / k / v sources on the GPU (synth.models.build_mha): with OAR_FUSE_MHA_ATTENTION=1 the block's core is
ONE launch of class mha_attention and no softmax launch exists; with =0 it runs op by op.  On both routes the output is within tol of the f64 reference
(tol = max(16 noise, 2^-19), noise = max |torch f32 - f64|; synth/mha_reference.py), and two fused runs give identical bytes.  Near misses and shapes the
kernel rejects keep the op-by-op route with the knob on.  Every test sets the knob itself: none depends on the default."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.mha_reference import mha_reference, reference_bundle

pytestmark = pytest.mark.gpu

KNOB = "OAR_FUSE_MHA_ATTENTION"
#         N   Tq   Tk nh  dh  scale
CASES = [(1, 5, 5, 2, 8, "pre"),            # less than one tile in every dimension
         (2, 20, 20, 4, 8, "post"),         # the test decoder's shape
         (1, 70, 33, 1, 64, "pre"),         # cross-attention; a query tail past one workgroup tile; one key past a block; the largest head
         (2, 64, 100, 3, 20, "post"),       # a head size that is no multiple of 16; more than three key blocks: both LDS stages are reused
         (1, 300, 300, 8, 32, "post"),      # the production decoder shape, both scale positions
         (1, 300, 300, 8, 32, "pre"),
         (1, 400, 400, 8, 32, "post"),      # the production AIFI shape, both scale positions
         (1, 400, 400, 8, 32, "pre")]
IDS = ["N%d_Tq%d_Tk%d_nh%d_dh%d_%s" % c for c in CASES]

_cache = {}


def _case(key, **kw):
    """model, info, feeds, reference bundle: computed once, never modified"""
    ck = (key, tuple(sorted(kw.items())))
    if ck not in _cache:
        N, Tq, Tk, nh, dh, scale = key
        model, info = models.build_mha(N, Tq, Tk, nh, dh, seed=3, scale=scale, **kw)
        rng = np.random.default_rng(11)
        feeds = {"x": rng.standard_normal((N, Tq, nh * dh)).astype(np.float32)}
        if not info["self"]:
            feeds["mem"] = rng.standard_normal((N, Tk, nh * dh)).astype(np.float32)
        _cache[ck] = (model, info, feeds, reference_bundle(mha_reference, info, feeds["x"], feeds.get("mem")))
    return _cache[ck]


def _run(model, feeds, runs=1):
    """-> the outputs of each run and the launch classes of the first"""
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        outs = [dict(eng.infer(list(feeds.items())))]
        snap = {e["name"]: e["launches"] for e in api.prof_snapshot()}
        api.prof_enable(False)
        for _ in range(runs - 1):
            outs.append(dict(eng.infer(list(feeds.items()))))
        return outs, snap
    finally:
        api.prof_enable(False)
        eng.close()


@pytest.mark.parametrize("fuse", ["1", "0"], ids=["fused", "op_by_op"])
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_block_matches_f64_on_both_routes(key, fuse, monkeypatch):
    model, info, feeds, ref = _case(key)
    monkeypatch.setenv(KNOB, fuse)
    outs, snap = _run(model, feeds, runs=2 if fuse == "1" else 1)
    err = float(np.abs(outs[0]["y"].astype(np.float64) - ref["f64"]).max())
    print(f"{key} {'fused' if fuse == '1' else 'op by op'}: {sum(snap.values())} launches | noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    if fuse == "1":
        assert snap.get("mha_attention", 0) == 1 and snap.get("softmax", 0) == 0, sorted(snap.items())
        assert outs[0]["y"].tobytes() == outs[1]["y"].tobytes()
    else:
        assert snap.get("mha_attention", 0) == 0, sorted(snap.items())
    assert outs[0]["y"].shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])


@pytest.mark.parametrize("key,kw", [((1, 12, 12, 1, 80, "post"), {}), ((1, 12, 12, 2, 6, "post"), {}),
                                    ((2, 20, 20, 4, 8, "post"), {"mask": True}), ((2, 20, 20, 4, 8, "post"), {"scores_output": True})],
                         ids=["dh80", "dh6", "additive_mask", "scores_are_an_output"])
def test_near_misses_keep_the_op_by_op_route(key, kw, monkeypatch):
    model, info, feeds, ref = _case(key, **kw)
    monkeypatch.setenv(KNOB, "1")
    outs, snap = _run(model, feeds)
    err = float(np.abs(outs[0]["y"].astype(np.float64) - ref["f64"]).max())
    print(f"{key} {kw}: {sum(snap.values())} launches | tol {ref['tol']:.2e} err {err:.2e}")
    assert snap.get("mha_attention", 0) == 0, sorted(snap.items())
    assert err <= ref["tol"], (err, ref["tol"])
    if "scores_output" in kw:
        assert outs[0]["scores"].shape == (key[0], key[3], key[1], key[2])
