"""add_layernorm.hip through its direct entry point (oar_k_add_layernorm): s = a + b[r % b_rows], y = LN(s) gamma + beta.
The stored sum is bit-equal to numpy's f32 addition, y is within tol of LN in f64 of that sum (tol = max(16 noise, 2^-19), noise = max |f32 numpy - f64|;
synth/layernorm_cases.py), and nothing outside the two output ranges of o_io is written.  Shapes: every register count of the half-wave form
(C = 4 .. 1024 around the multiples of 128), the eight-rows-per-workgroup tail, the one-wave form (C no multiple of 4, C > 1024, an odd offset)."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import layernorm_cases as lc

pytestmark = pytest.mark.gpu

ROWS = (1, 7, 8, 9, 17)
V4_C = (4, 32, 124, 128, 132, 256, 260, 384, 512, 516, 1024)
GENERIC_C = (1, 3, 30, 65, 1028, 1500)
GUARD = 12                                     # sentinel floats in front of, between and behind the outputs

_cache = {}


def _case(family, rows, C, b_rows, eps=1e-5, gamma=True, beta=True, seed=3):
    """inputs and the reference bundle: computed once, never modified"""
    key = (family, rows, C, b_rows, eps, gamma, beta, seed)
    if key not in _cache:
        a, b, g, be = lc.inputs(family, rows, C, b_rows, seed=seed)
        g, be = (g if gamma else None), (be if beta else None)
        _cache[key] = (a, b, g, be, lc.reference_bundle(a, b, b_rows, g, be, eps))
    return _cache[key]


def _launch(a, b, g, be, eps, write_sum, y_off=GUARD, s_gap=GUARD, b_rows=None):
    """-> (y, s or None, o_io before, o_io after, y_off, s_off): o_io = sentinel | y | sentinel | s | sentinel, every sentinel float a distinct finite bit pattern"""
    rows, C = a.shape
    cnt = rows * C
    s_off = y_off + cnt + s_gap
    o = (np.arange(s_off + cnt + GUARD, dtype=np.uint32) + np.uint32(0xC2AD0000)).view(np.float32)
    out = api.k_add_layernorm(a, b, g, be, eps, write_sum, o, y_off, s_off, b_rows=b_rows)
    return out[y_off:y_off + cnt].reshape(rows, C), (out[s_off:s_off + cnt].reshape(rows, C) if write_sum else None), o, out, y_off, s_off


def _check(a, b, g, be, ref, eps, write_sum=True, y_off=GUARD, s_gap=GUARD, b_rows=None, label=""):
    y, s, before, after, y_off, s_off = _launch(a, b, g, be, eps, write_sum, y_off, s_gap, b_rows)
    cnt = a.size
    outside = np.ones(before.size, bool)
    outside[y_off:y_off + cnt] = False
    if write_sum:
        outside[s_off:s_off + cnt] = False
    assert before.view(np.uint32)[outside].tobytes() == after.view(np.uint32)[outside].tobytes(), f"{label}: a float outside the outputs was written"
    if write_sum:
        assert s.tobytes() == ref["sum"].tobytes(), f"{label}: the sum is not numpy's f32 sum"
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max()) if np.isfinite(y).all() else float("inf")
    print(f"{label}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    assert err <= ref["tol"], (label, err, ref["tol"])
    return y


@pytest.mark.parametrize("C", V4_C)
def test_half_wave_form_at_every_register_count_and_row_tail(C):
    for rows in ROWS:
        for family in ("normal", "offset"):
            a, b, g, be, ref = _case(family, rows, C, rows)
            _check(a, b, g, be, ref, 1e-5, label=f"rows {rows} C {C} {family}")


@pytest.mark.parametrize("C", GENERIC_C)
def test_one_wave_form(C):
    for rows in ROWS:
        a, b, g, be, ref = _case("offset" if C > 1 else "normal", rows, C, rows)
        y = _check(a, b, g, be, ref, 1e-5, label=f"rows {rows} C {C}")
        if C == 1:
            assert y.tobytes() == np.broadcast_to(be, (rows, 1)).astype(np.float32).tobytes()      # (s - mean) is exactly 0: y = beta


@pytest.mark.parametrize("y_off,s_gap", [(GUARD + 1, GUARD), (GUARD, GUARD + 1), (GUARD + 3, GUARD + 2)], ids=["y_odd", "s_odd", "both_odd"])
def test_an_offset_that_is_no_multiple_of_4_floats_takes_the_one_wave_form(y_off, s_gap):
    a, b, g, be, ref = _case("offset", 9, 128, 9)
    y = _check(a, b, g, be, ref, 1e-5, y_off=y_off, s_gap=s_gap, label=f"C 128 y_off {y_off} s_gap {s_gap}")
    aligned = _check(a, b, g, be, ref, 1e-5, label="C 128 aligned")
    assert float(np.abs(y.astype(np.float64) - aligned.astype(np.float64)).max()) <= 2 * ref["tol"]     # another order of sums, the same row


@pytest.mark.parametrize("C", [132, 30])
@pytest.mark.parametrize("b_rows", [15, 5, 1])
def test_broadcast_forms_affine_sum_and_eps(b_rows, C):
    rows = 15
    for family in ("periodic", "cancel"):
        for gamma, beta in ((True, True), (True, False), (False, True), (False, False)):
            for eps in (1e-5, 1e-6):
                a, b, g, be, ref = _case(family, rows, C, b_rows, eps, gamma, beta)
                for write_sum in (True, False):
                    _check(a, b, g, be, ref, eps, write_sum=write_sum, label=f"C {C} b_rows {b_rows} {family} g {gamma} b {beta} eps {eps} sum {write_sum}")


@pytest.mark.parametrize("C", [260, 65])
@pytest.mark.parametrize("r", [4, 5], ids=["even_row", "odd_row"])
def test_a_nan_or_inf_stays_in_its_row(r, C):
    """rows 4 and 5 share a wave in the half-wave form"""
    rows = 9
    a, b, g, be, ref = _case("normal", rows, C, rows)
    clean = _check(a, b, g, be, ref, 1e-5, label=f"C {C} clean")
    for bad in (np.nan, np.inf):
        a2 = a.copy()
        a2[r, C // 3] = bad
        y, s, *_ = _launch(a2, b, g, be, 1e-5, True)
        assert not np.isfinite(y[r]).any(), (bad, "row", r)
        keep = np.arange(rows) != r
        assert y[keep].tobytes() == clean[keep].tobytes(), (bad, "another row changed")
        assert s[keep].tobytes() == ref["sum"][keep].tobytes()


def test_a_bad_b_rows_is_refused_and_a_good_call_still_works():
    a, b, g, be, ref = _case("periodic", 15, 132, 5)
    for b_rows in (4, 0, -5, 30):
        with pytest.raises(api.OCRError) as e:
            api.k_add_layernorm(a, np.zeros((30, 132), np.float32), g, be, 1e-5, False, np.zeros(a.size, np.float32), 0, b_rows=b_rows)
        assert e.value.code == api.OAR_INVALID_INPUT, b_rows
    _check(a, b, g, be, ref, 1e-5, label="after the refusals")
