"""The SLA structure head on the GPU: an ONNX Loop of M greedy attention-GRU steps that the engine replaces by one Linear (the loop-invariant
feature projection) and ONE launch of the fused decode kernel (csrc/sla_decode.hip).

Reference: the same recurrence in torch on the CPU, in f64 and in f32 (synth/sla_reference.py).  The weights follow synth.models.sla_weights, a recipe
under which a 501-step free-running decode is well conditioned: f32 and f64 agree to 1e-7 .. 1e-6 although the emitted token changes tens to
hundreds of times per sequence.  Each case measures that `noise` itself and asserts, in this order:
  1. on the reference alone: every step's top-1 / top-2 probability gap >= 8 tol, tol = max(16 noise, 2^-19) -- the greedy path never comes close
     enough to a fork for an error of size tol to change it (the seeds are chosen so that this holds; no step is excluded)
  2. the GPU's tokens equal the f64 tokens at every step
  3. probabilities and locations lie within tol / tol_loc of f64, the last hidden state within 16 noise_h
The measured figures are printed (pytest -s) and recorded in DESIGN 4.30."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.sla_reference import sla_head_reference, sla_reference_bundle

pytestmark = pytest.mark.gpu

#          C    H   V  L   HW    M  B  seed
SHAPES = [(20, 24, 11, 4, 9, 24, 5, 3),            # nothing a multiple of 16 / 64; C, H multiples of 4: vector loads, one partial group
          (33, 40, 13, 8, 37, 40, 3, 5),           # C odd: scalar feature loads, padded weight rows
          (96, 256, 50, 8, 256, 501, 3, 3),        # the SLANet_plus head
          (96, 256, 30, 4, 256, 501, 1, 0),
          (20, 24, 11, 4, 9, 1, 1, 3)]             # a single step


def _fea(shape):
    C, H, V, L, HW, M, B, seed = shape
    return np.random.default_rng(1000 + seed).standard_normal((B, HW, C)).astype(np.float32)


def _run(model, fea):
    eng = api.OrtInfer(model)
    try:
        return dict(eng.infer(fea))
    finally:
        eng.close()


_cache = {}


def _case(shape):
    """reference bundle and GPU outputs of one shape: computed once, never modified"""
    if shape not in _cache:
        C, H, V, L, HW, M, B, seed = shape
        model, info = models.build_slanet(C=C, H=H, V=V, L=L, M=M, seed=seed, head_only=True)
        fea = _fea(shape)
        _cache[shape] = (sla_reference_bundle(info["weights"], fea, M), _run(model, fea))
    return _cache[shape]


def _check_against(ref, outs, M, label):
    r64 = ref["f64"]
    B, V, L = r64["probs"].shape[0], r64["probs"].shape[2], r64["loc"].shape[2]
    assert outs["structure_probs"].shape == (B, M, V) and outs["bbox"].shape == (B, M, L)
    tol, tol_loc, tol_h = ref["tol"], ref["tol_loc"], 16 * ref["noise_h"]
    err_p = float(np.abs(outs["structure_probs"].astype(np.float64) - r64["probs"]).max())
    err_l = float(np.abs(outs["bbox"].astype(np.float64) - r64["loc"]).max())
    err_h = float(np.abs(outs["h_last"].astype(np.float64) - r64["h"]).max())
    print(f"{label}: noise {ref['noise']:.2e} loc {ref['noise_loc']:.2e} h {ref['noise_h']:.2e} | tol {tol:.2e} / {tol_loc:.2e} / {tol_h:.2e} | "
          f"gap {ref['gap']:.2e} token changes {ref['changes']} | gpu err probs {err_p:.2e} loc {err_l:.2e} h {err_h:.2e}")
    assert ref["gap"] >= 8 * tol, ("the reference itself is ill conditioned for this seed", ref["gap"], tol)
    tokens = outs["structure_probs"].argmax(2)
    assert np.array_equal(tokens, r64["tokens"]), ("tokens differ at (image, step)", np.argwhere(tokens != r64["tokens"])[:4])
    assert outs["pre_last"].dtype == np.int64 and np.array_equal(outs["pre_last"], r64["tokens"][:, -1])
    assert err_p <= tol, (err_p, tol)
    assert err_l <= tol_loc, (err_l, tol_loc)
    assert err_h <= tol_h, (err_h, tol_h)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_H%d_V%d_L%d_HW%d_M%d_B%d" % s[:7])
def test_fused_decode_matches_the_f64_recurrence(shape):
    ref, outs = _case(shape)
    _check_against(ref, outs, shape[5], str(shape[:7]))


def test_equal_logits_go_to_the_lowest_index():
    """two identical rows of W_s2 / b_s2, scaled so that they win most steps: the higher index is never emitted (ONNX ArgMax, select_last_index = 0)"""
    C, H, V, L, HW, M, B, seed = 20, 24, 11, 4, 9, 24, 5, 3
    w = models.sla_weights(C, H, V, L, seed)
    lo, hi = 2, 7
    w["s2w"][lo] *= np.float32(3.0)
    w["s2b"][lo] = np.float32(2.0)
    w["s2w"][hi], w["s2b"][hi] = w["s2w"][lo], w["s2b"][lo]
    model, _ = models.build_slanet(C=C, H=H, V=V, L=L, M=M, seed=seed, head_only=True, weights=w)
    fea = _fea((C, H, V, L, HW, M, B, seed))
    ref = sla_head_reference(w, fea, M, "float64")
    assert np.array_equal(ref["logits"][..., lo], ref["logits"][..., hi]) and (ref["tokens"] == lo).sum() >= M     # the tie really decides steps
    outs = _run(model, fea)
    assert np.array_equal(outs["structure_probs"][..., lo], outs["structure_probs"][..., hi])
    assert np.array_equal(outs["pre_last"], ref["tokens"][:, -1]) and not np.any(outs["pre_last"] == hi)
    # argmax of the softmax output ties the same way as the kernel's argmax of the logits had to: the fed-back token decides every later step
    assert np.array_equal(outs["structure_probs"].argmax(2), ref["tokens"])
    assert not np.any(outs["structure_probs"].argmax(2) == hi)


def test_one_launch_per_infer():
    C, H, V, L, HW, M, B, seed = SHAPES[1]
    model, _ = models.build_slanet(C=C, H=H, V=V, L=L, M=M, seed=seed, head_only=True)
    eng = api.OrtInfer(model, profile=True)
    try:
        fea = _fea(SHAPES[1])
        eng.infer(fea)                       # plan
        for runs in (1, 2):                  # (the second infer of a plan may replay it as a captured graph: still one launch each)
            api.prof_reset()
            api.prof_enable(True)
            for _ in range(runs):
                eng.infer(fea)
            snap = {e["name"]: e for e in api.prof_snapshot()}
            assert "sla_decode" in snap and snap["sla_decode"]["launches"] == runs, snap.get("sla_decode")
        fl, by, nk = eng.cost(list(fea.shape))
        step_macs = 4 * H * H + HW * H + HW * C + 3 * H * C + 2 * H * H + (V + L) * H
        assert fl >= 2.0 * step_macs * M * B and by >= 4.0 * step_macs * M * B       # the step's cost is counted M times
    finally:
        api.prof_enable(False)
        eng.close()


def test_matmul_add_spelling_with_outer_weights_fuses_too():
    shape = SHAPES[1]
    C, H, V, L, HW, M, B, seed = shape
    model, _ = models.build_slanet(C=C, H=H, V=V, L=L, M=M, seed=seed, head_only=True, spelling="matmul")
    ref, _ = _case(shape)
    _check_against(ref, _run(model, _fea(shape)), M, "matmul+add " + str(shape[:7]))


def _counter_loop():
    """Loop(M, true, acc0) { acc = acc + 1 }: a valid Loop that is not the SLA step"""
    from oar_ocr_amd.synth.onnx_writer import BOOL, INT64, GraphBuilder
    b = GraphBuilder("counter")
    b.add_input("it", [], INT64)
    b.add_input("cond_in", [], BOOL)
    b.add_input("acc", [4])
    b.op("Identity", ["cond_in"], outputs=["cond_out"])
    b.op("Add", ["acc", b.init(np.ones(4, np.float32), "one")], outputs=["acc_new"])
    b.add_output("cond_out", [], BOOL)
    b.add_output("acc_new", [4])
    g = GraphBuilder("outer")
    g.add_input("x", [4])
    g.op("Loop", [g.init(np.array(3, np.int64), "trip"), g.init(np.array(True), "cond"), "x"], outputs=["y"], body=b)
    g.add_output("y", [4])
    return g.model()


def test_other_loop_bodies_are_refused_by_name():
    m, _ = models.build_slanet(C=20, H=24, V=11, L=4, M=4, head_only=True, first_act="Relu")
    with pytest.raises(api.OCRError) as ex:
        api.OrtInfer(m)
    assert ex.value.code == api.OAR_UNSUPPORTED_OP and "Loop" in str(ex.value) and "Relu" in str(ex.value), str(ex.value)
    with pytest.raises(api.OCRError) as ex:
        api.OrtInfer(_counter_loop())
    assert ex.value.code == api.OAR_UNSUPPORTED_OP and "Loop" in str(ex.value), str(ex.value)
    m, _ = models.build_slanet(C=20, H=24, V=11, L=4, M=5000, head_only=True)          # M beyond the kernel's limit
    with pytest.raises(api.OCRError) as ex:
        api.OrtInfer(m)
    assert ex.value.code == api.OAR_UNSUPPORTED_OP and "Loop" in str(ex.value), str(ex.value)
