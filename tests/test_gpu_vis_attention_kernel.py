"""vis_attention.hip called directly (api.k_vis_attention) against the attention alone in f64, rotary included (synth/vision_reference.py):
tol = max(16 noise, 2^-19) with noise = max |numpy f32 - f64| on these very inputs.  Head sizes 8, 24, 40, 56, 72, 80 (every instantiation, DH16 = 5 partial
and full) times the segment sets (1), (31, 32, 33), (64, 65), (4, 140), each dense and with a row stride above 3 D whose padding is NaN.
Every run: o sits between two guards of 64 sentinel floats in a sentinel-filled buffer; afterwards the guards are untouched, every output element was
written, the output is finite and within tol.  Both layouts and a second run give identical bytes."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import vision_reference as vr

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = np.uint32(0x7FA5C3E1)      # a NaN with a payload: no finite output equals it, and a copy of it is recognised by its bits
CASES = [(dh, lens) for dh in vr.HEAD_SIZES for lens in vr.SEGMENT_SETS]
IDS = ["dh%d_%s" % (dh, "_".join(map(str, lens))) for dh, lens in CASES]

_cache = {}


def _case(dh, lens):
    """inputs and the reference bundle: computed once, never modified"""
    if (dh, lens) not in _cache:
        c = vr.attention_case(dh, lens, seed=31)
        _cache[(dh, lens)] = (c, vr.reference_bundle(vr.vis_attention_core, c["qkv"], c["cos"], c["sin"], c["lens"], c["nh"], c["dh"]))
    return _cache[(dh, lens)]


def _o_io(n):
    return np.full(GUARD + n + GUARD, SENTINEL, np.uint32).view(np.float32)


def _run(c, pad=0, off=0, qkv=None, finite=True):
    T, D = sum(c["lens"]), c["nh"] * c["dh"]
    buf, qkv_off, ld = vr.packed_layout(c if qkv is None else {**c, "qkv": qkv}, pad=pad, off=off)
    n = T * D
    out = api.k_vis_attention(buf, qkv_off, ld, c["lens"], c["nh"], c["dh"], c["cos"], c["sin"], _o_io(n), GUARD)
    bits = out.view(np.uint32)
    assert out.size == GUARD + n + GUARD
    assert (bits[:GUARD] == SENTINEL).all() and (bits[GUARD + n:] == SENTINEL).all(), "a guard word changed"
    assert not (bits[GUARD:GUARD + n] == SENTINEL).any(), f"{int((bits[GUARD:GUARD + n] == SENTINEL).sum())} output elements were never written"
    o = out[GUARD:GUARD + n].reshape(T, D)
    assert not finite or np.isfinite(o).all(), "non-finite output"
    return o


@pytest.mark.parametrize("dh,lens", CASES, ids=IDS)
def test_vis_attention_matches_f64(dh, lens):
    c, ref = _case(dh, lens)
    dense = _run(c)
    err = float(np.abs(dense.astype(np.float64) - ref["f64"]).max())
    print(f"vis_attention dh {dh} segments {lens}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    assert dense.shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])
    padded = _run(c, pad=12, off=8)                                          # the loop's arithmetic does not depend on addresses; NaN between the rows
    assert padded.tobytes() == dense.tobytes(), f"padded differs from dense by {np.abs(padded - dense).max():.3e}"
    assert _run(c).tobytes() == dense.tobytes()                              # run to run
    if lens == (1,):                                                         # p = 1, l = 1: o is the v row, bit for bit
        assert dense.tobytes() == c["qkv"][:, 2].reshape(1, -1).tobytes()


@pytest.mark.parametrize("dh", [24, 72])
def test_a_segment_of_nan_stays_in_its_segment(dh):
    """k and v of the middle segment all NaN: the other segments' outputs are bitwise those of the run without the NaN, its own output is NaN"""
    lens = (31, 32, 33)
    c, _ = _case(dh, lens)
    clean = _run(c)
    qkv = c["qkv"].copy()
    qkv[31:63, 1:] = np.nan
    o = _run(c, qkv=qkv, finite=False)
    assert o[:31].tobytes() == clean[:31].tobytes() and o[63:].tobytes() == clean[63:].tobytes()
    assert np.isnan(o[31:63]).all()


def test_rejected_head_sizes_launch_nothing():
    for dh in (12, 88):
        T, nh = 8, 2
        o_io, z = _o_io(T * nh * dh), lambda n: np.zeros(n, np.float32)
        lens = np.asarray((5, 3), np.int32)
        code = api.lib().oar_k_vis_attention(api._p(z(T * 3 * nh * dh)), T * 3 * nh * dh, 0, 3 * nh * dh, api._p(lens), 2, nh, dh, api._p(z(T * dh // 2)), api._p(z(T * dh // 2)),
                                             api._p(o_io), o_io.size, GUARD)
        assert code == api.OAR_UNSUPPORTED_OP, (dh, code)
        assert (o_io.view(np.uint32) == SENTINEL).all()                      # the very buffer the library was given
    c, ref = _case(8, (1,))                                                  # and the library still works afterwards
    assert np.abs(_run(c) - ref["f64"]).max() <= ref["tol"]
