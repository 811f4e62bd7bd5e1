"""qvis_misc.hip through its direct entries (vl.k_qvis_rmsnorm / k_qvis_act / k_qvis_row_gather).  The gather is exact; RMSNorm and the activations
are held to the project's rule on unit-scale inputs: tol = max(16 noise, 2^-19), noise = max |f32 - f64| of the numpy reference on the same input.  Guard
words around every output come back untouched, a NaN stays where it is, and two runs give the same bytes."""
import numpy as np
import pytest

from oar_ocr_amd import vl
from oar_ocr_amd.synth import qwen_vision_reference as qr

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = np.uint32(0x7FA5C3E1)   # a quiet NaN pattern no kernel produces


def _o_io(n):
    return np.full(GUARD + n + GUARD, SENTINEL, np.uint32).view(np.float32)


def _payload(o_io, n):
    bits = o_io.view(np.uint32)
    assert (bits[:GUARD] == SENTINEL).all() and (bits[GUARD + n:] == SENTINEL).all(), "a guard word was written"
    return o_io[GUARD:GUARD + n]


def _tol(f32, f64):
    noise = float(np.abs(f32.astype(np.float64) - f64).max())
    return noise, max(16 * noise, 2.0 ** -19)


@pytest.mark.parametrize("row_floats", [48, 96, 640, 5120])
@pytest.mark.parametrize("rows", [1, 5, 117])
def test_row_gather_is_exact(row_floats, rows):
    rng = np.random.default_rng([row_floats, rows])
    x = rng.standard_normal((rows, row_floats)).astype(np.float32)
    for name, idx in (("identity", np.arange(rows)), ("reversed", np.arange(rows)[::-1]), ("random", rng.permutation(rows))):
        out = vl.k_qvis_row_gather(x, idx, _o_io(rows * row_floats), GUARD)
        assert _payload(out, rows * row_floats).tobytes() == x[idx].tobytes(), name
    # fewer output rows than input rows, an input row taken twice
    idx = rng.integers(0, rows, max(rows // 2, 1))
    out = vl.k_qvis_row_gather(x, idx, _o_io(idx.size * row_floats), GUARD)
    assert _payload(out, idx.size * row_floats).tobytes() == x[idx].tobytes()


def test_row_gather_refuses_an_index_outside_the_input():
    from oar_ocr_amd import api
    x = np.zeros((3, 8), np.float32)
    for idx in ([0, 3], [-1]):
        with pytest.raises(api.OCRError) as e:
            vl.k_qvis_row_gather(x, idx, _o_io(16), GUARD)
        assert e.value.code == api.OAR_INVALID_INPUT


@pytest.mark.parametrize("D", [24, 160, 1280])
@pytest.mark.parametrize("rows", [1, 3, 64, 65])
def test_rmsnorm_matches_f64(D, rows):
    rng = np.random.default_rng([D, rows, 1])
    x = rng.standard_normal((rows, D)).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    if rows >= 3:
        x[1] = 0.0                                                  # a zero row gives zeros
        x[0] *= 1e-3                                                # mean(x^2) near eps, the output still unit-scale: eps misplaced (inside the mean's divisor) moves it by tens of percent
    r64, r32 = qr.rms_norm(x.astype(np.float64), g.astype(np.float64)), qr.rms_norm(x, g)
    noise, tol = _tol(r32, r64)
    out = vl.k_qvis_rmsnorm(x, g, 1e-6, _o_io(rows * D), GUARD)
    y = _payload(out, rows * D).reshape(rows, D).copy()
    err = float(np.abs(y.astype(np.float64) - r64).max())
    print(f"rmsnorm D={D} rows={rows}: noise {noise:.2e} tol {tol:.2e} err {err:.2e}")
    assert np.isfinite(y).all() and err <= tol, (err, tol)
    if rows >= 3:
        assert not y[1].any()
    assert vl.k_qvis_rmsnorm(x, g, 1e-6, _o_io(rows * D), GUARD).tobytes() == out.tobytes()     # two runs, the same bytes
    if rows >= 3:                                                   # a NaN stays inside its own row
        xn = x.copy()
        xn[2, D // 2] = np.nan
        yn = _payload(vl.k_qvis_rmsnorm(xn, g, 1e-6, _o_io(rows * D), GUARD), rows * D).reshape(rows, D)
        assert np.isnan(yn[2]).all()
        keep = np.arange(rows) != 2
        assert yn[keep].tobytes() == y[keep].tobytes()


@pytest.mark.parametrize("F", [36, 200, 5120])
@pytest.mark.parametrize("act", ["quick_gelu", "silu", "gelu"])
@pytest.mark.parametrize("gated", [False, True])
def test_act_matches_f64(F, act, gated):
    rows = 5 if F == 5120 else 67
    rng = np.random.default_rng([F, len(act), int(gated)])
    width = 2 * F if gated else F
    x = rng.standard_normal((rows, width)).astype(np.float32)
    x[0, 0], x[0, 1] = 0.0, -0.0
    if gated:
        x[0, F], x[0, F + 1] = 1.0, 1.0

    def ref(v):
        return qr.act_fn(act, v[:, :F]) * v[:, F:] if gated else qr.act_fn(act, v)
    r64, r32 = ref(x.astype(np.float64)), ref(x)
    noise, tol = _tol(r32, r64)
    # NaN behind the last row the kernel may read (a wrong stride in a middle row shows in the values, not here)
    buf = np.concatenate([x.reshape(-1), np.full(256, np.nan, np.float32)])
    out = vl.k_qvis_act(buf, rows, F, act, gated, _o_io(rows * F), GUARD)
    y = _payload(out, rows * F).reshape(rows, F).copy()
    err = float(np.abs(y.astype(np.float64) - r64).max())
    print(f"act {act} gated={gated} F={F}: noise {noise:.2e} tol {tol:.2e} err {err:.2e}")
    assert np.isfinite(y).all() and err <= tol, (err, tol)
    assert y[0, 0] == 0.0 and not np.signbit(y[0, 0]) and y[0, 1] == 0.0 and np.signbit(y[0, 1])      # +0 and -0 keep their signs
    assert vl.k_qvis_act(buf, rows, F, act, gated, _o_io(rows * F), GUARD).tobytes() == out.tobytes()
    for col in ((3, F + 7) if gated else (3,)):                     # a NaN stays in its element
        xn = x.copy()
        xn[1, col] = np.nan
        yn = _payload(vl.k_qvis_act(np.concatenate([xn.reshape(-1), np.full(256, np.nan, np.float32)]), rows, F, act, gated, _o_io(rows * F), GUARD), rows * F).reshape(rows, F)
        mask = np.zeros((rows, F), bool)
        mask[1, col % F] = True
        assert np.isnan(yn[mask]).all() and yn[~mask].tobytes() == y[~mask].tobytes()
