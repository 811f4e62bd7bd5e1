"""The DeformableAttention operator (csrc/deformable_attention.hip): the core of multi-scale deformable attention -- per level a GridSample of
the value viewed as [N nh, c, h, w], the L P samples summed with softmax weights -- which the engine's rewrite pass 3c turns into ONE launch that reads the
taps from the value [N, Lv, nh, c] by address.  Graphs: synth.models.build_deformable_attention, in both weight modes.

Reference: the same math in torch on the CPU, in f64 and f32 (synth/rtdetr_reference.py); noise = max |f32 - f64|, tol = max(16 noise, 2^-19).  The logits are
3 N(0, 1), a peaked softmax, so a tap from another level, point or head moves the output by O(1); a third of the coordinates lie outside the image.
Per case: exactly one launch of class deformable_attention with the pass on and neither grid_sample nor permute launches; with
OAR_FUSE_DEFORMABLE_ATTENTION=0 none, and one grid_sample launch per level; both outputs within tol of f64; two fused runs bit-identical."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.rtdetr_reference import deformable_attention_inputs, deformable_attention_reference
from oar_ocr_amd.synth.unimernet_reference import reference_bundle

pytestmark = pytest.mark.gpu

#          N   Q  nh  c  levels (h, w)                        P
SHAPES = [(2, 7, 2, 8, ((5, 7), (3, 4)), 3),                      # h / w swapped; level start offsets; two lanes per head; batch stride
          (1, 5, 3, 4, ((1, 1), (2, 9), (6, 1)), 4),              # 1 x 1, one-row and one-column levels; one lane per head; three heads
          (1, 300, 8, 32, ((10, 10), (5, 5), (3, 3)), 4),         # RT-DETR's own head layout: one wave per query
          (3, 33, 4, 16, ((4, 6),), 1),                           # a softmax over one value; Q and N Q that fill no wave
          (1, 9, 1, 64, ((3, 5), (2, 2), (2, 3), (1, 2)), 8)]     # the limits c = 64, L = 4, L P = 32
IDS = ["N%d_Q%d_nh%d_c%d_L%d_P%d" % (s[0], s[1], s[2], s[3], len(s[4]), s[5]) for s in SHAPES]
FALLBACK = (1, 6, 2, 6, ((4, 4),), 2)                              # c % 4 != 0: k::deformable_attention_supported says no
KNOB = "OAR_FUSE_DEFORMABLE_ATTENTION"

_cache = {}


def _case(shape, mode, align_corners=0):
    """model, info, feeds, reference bundle: computed once, never modified"""
    key = (shape, mode, align_corners)
    if key not in _cache:
        model, info = models.build_deformable_attention(*shape, weights=mode, align_corners=align_corners)
        value, loc, logit = deformable_attention_inputs(info, seed=5)
        _cache[key] = (model, info, (value, loc, logit), reference_bundle(deformable_attention_reference, info, value, loc, logit))
    return _cache[key]


def _run(model, feeds, monkeypatch, fuse):
    """-> (y, {class: launches} of one infer)"""
    if fuse is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, fuse)                              # (read when the graph is loaded)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        y = dict(eng.infer(list(zip(("value", "loc", "logit"), feeds))))["y"]
        return y, {e["name"]: e["launches"] for e in api.prof_snapshot()}
    finally:
        api.prof_enable(False)
        eng.close()


def _err(y, ref):
    return float(np.abs(y.astype(np.float64) - ref["f64"]).max())


@pytest.mark.parametrize("mode", ["softmax", "input"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_launch_and_both_routes_match_f64(shape, mode, monkeypatch):
    model, info, feeds, ref = _case(shape, mode)
    fused, snap = _run(model, feeds, monkeypatch, None)
    again, _ = _run(model, feeds, monkeypatch, None)
    plain, snap0 = _run(model, feeds, monkeypatch, "0")
    e1, e0 = _err(fused, ref), _err(plain, ref)
    print(f"{shape} {mode}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} | fused err {e1:.2e} ({sum(snap.values())} launches) | "
          f"op-by-op err {e0:.2e} ({sum(snap0.values())} launches)")
    assert snap.get("deformable_attention", 0) == 1, sorted(snap.items())
    assert snap.get("grid_sample", 0) == 0 and snap.get("permute", 0) == 0, sorted(snap.items())
    assert snap0.get("deformable_attention", 0) == 0 and snap0.get("grid_sample", 0) == len(shape[4]), sorted(snap0.items())
    assert fused.shape == ref["f64"].shape and e1 <= ref["tol"], (e1, ref["tol"])
    assert plain.shape == ref["f64"].shape and e0 <= ref["tol"], (e0, ref["tol"])
    assert np.array_equal(fused, again)                             # no atomics, no dependence on scheduling


def test_explicit_knob_on_is_the_default(monkeypatch):
    model, info, feeds, ref = _case(SHAPES[0], "softmax")
    a, sa = _run(model, feeds, monkeypatch, None)
    b, sb = _run(model, feeds, monkeypatch, "1")
    assert sa.get("deformable_attention", 0) == sb.get("deformable_attention", 0) == 1 and np.array_equal(a, b)


@pytest.mark.parametrize("mode", ["softmax", "input"])
def test_unsupported_head_size_keeps_the_op_by_op_route(mode, monkeypatch):
    model, info, feeds, ref = _case(FALLBACK, mode)
    y, snap = _run(model, feeds, monkeypatch, None)
    y0, snap0 = _run(model, feeds, monkeypatch, "0")
    err = _err(y, ref)
    print(f"fallback {FALLBACK} {mode}: err {err:.2e} tol {ref['tol']:.2e}")
    assert snap.get("deformable_attention", 0) == 0 and snap0.get("deformable_attention", 0) == 0, sorted(snap.items())
    assert snap.get("grid_sample", 0) == 1
    assert np.array_equal(y, y0) and err <= ref["tol"], (err, ref["tol"])


@pytest.mark.parametrize("mode", ["softmax", "input"])
def test_samples_outside_every_level_give_exact_zeros(mode, monkeypatch):
    """needs no reference: every location of head 0 of query 0 at 2.5 (outside each level by more than a pixel) -> its c channels are exactly 0.0"""
    shape = SHAPES[0]
    model, info, (value, loc, logit), _ = _case(shape, mode)
    loc = loc.copy()
    loc[0, 0, 0] = 2.5
    c = shape[3]
    for fuse in (None, "0"):
        y, snap = _run(model, (value, loc, logit), monkeypatch, fuse)
        assert snap.get("deformable_attention", 0) == (1 if fuse is None else 0)
        assert np.all(y[0, 0, :c] == 0.0), (fuse, y[0, 0, :c])
        assert np.all(y[0, 0, c:] != 0.0) and np.all(y[0, 1] != 0.0)     # (the neighbours are not zeroed with it)


def test_other_alignment_is_not_matched(monkeypatch):
    """the same graph with align_corners = 1: the kernel does not compute that, so the op-by-op route stays -- and meets its own reference"""
    shape = SHAPES[0]
    model, info, feeds, ref = _case(shape, "softmax", align_corners=1)
    _, _, _, ref0 = _case(shape, "softmax")
    y, snap = _run(model, feeds, monkeypatch, None)
    err = _err(y, ref)
    print(f"align_corners=1: err {err:.2e} tol {ref['tol']:.2e}; distance of the two references {np.abs(ref['f64'] - ref0['f64']).max():.2e}")
    assert snap.get("deformable_attention", 0) == 0 and snap.get("grid_sample", 0) == len(shape[4]), sorted(snap.items())
    assert err <= ref["tol"], (err, ref["tol"])
    assert np.abs(ref["f64"] - ref0["f64"]).max() > 1e3 * ref["tol"]   # (the two alignments really differ on these inputs)
