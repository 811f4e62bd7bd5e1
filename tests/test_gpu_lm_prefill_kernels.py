"""The two kernels of the GEMM-based prefill alone, through their direct entries, against f64: api.k_lm_gemm (lm_prefill_gemm.hip, plain epilogue, f32
and bf16 weights) and api.k_lm_prefill_attention (lm_prefill_attn.hip).  Tolerance as everywhere: noise = max |f32 - f64| of the torch reference of the op itself,
tol = max(16 noise, 2^-19).  Shapes: synth/lm_prefill_cases.py."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import lm_prefill_cases as P

pytestmark = pytest.mark.gpu

GUARD = np.float32(-777.25)


def _guarded(n, off):
    return np.full(off + n + 37, GUARD, np.float32)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,N", P.GEMM_KN)
def test_lm_gemm_against_f64(K, N, bf16):
    """every M of GEMM_MS (below, at and above one and two 64-token tiles; 130 = three tiles) at this (K, N); the output sits 5 floats into a buffer of guard words"""
    for M in P.GEMM_MS:
        x, w, y64, y32 = P.gemm_case(M, K, N, bf16)
        noise, tol = P.tol_of(y32, y64)
        off = 5
        out = api.k_lm_gemm(x, w, _guarded(M * N, off), off)
        y = out[off:off + M * N].reshape(M, N)
        err = float(np.abs(y.astype(np.float64) - y64).max())
        print(f"lm_gemm M={M} K={K} N={N} {'bf16' if bf16 else 'f32'}: noise {noise:.3e} tol {tol:.3e} error {err:.3e} ({err / tol:.3f} tol)")
        assert np.isfinite(y).all() and err <= tol, (M, K, N, err, tol)
        assert (out[:off] == GUARD).all() and (out[off + M * N:] == GUARD).all()


@pytest.mark.parametrize("M,row", [(17, 16), (65, 0), (130, 64)])
def test_a_nan_row_of_x_stays_in_its_output_row(M, row):
    x, w, y64, _ = P.gemm_case(M, 36, 34, False)
    clean = api.k_lm_gemm(x, w, np.zeros(M * 34, np.float32), 0).reshape(M, 34)
    x = x.copy()
    x[row, 7] = np.nan
    y = api.k_lm_gemm(x, w, np.zeros(M * 34, np.float32), 0).reshape(M, 34)
    assert np.isnan(y[row]).all()
    keep = np.arange(M) != row
    assert y[keep].tobytes() == clean[keep].tobytes()


def test_lm_gemm_output_does_not_depend_on_m_or_on_the_rows_place():
    """row 3 of a 130-row call, the same row alone and as row 64 of another call: the same bits (an element's sum order is fixed by K)"""
    x, w, _, _ = P.gemm_case(130, 1028, 34, True)
    full = api.k_lm_gemm(x, w, np.zeros(130 * 34, np.float32), 0).reshape(130, 34)
    alone = api.k_lm_gemm(x[3:4], w, np.zeros(34, np.float32), 0)
    moved = np.roll(x, 61, axis=0)          # row 3 -> row 64
    other = api.k_lm_gemm(moved, w, np.zeros(130 * 34, np.float32), 0).reshape(130, 34)
    assert alone.tobytes() == full[3].tobytes() == other[64].tobytes()


@pytest.mark.parametrize("G", P.ATTN_GS)
@pytest.mark.parametrize("dh", P.ATTN_DHS)
def test_lm_prefill_attention_against_f64(dh, G):
    """every sequence set of ATTN_SEQS at this head size and group size; query 0 of every sequence returns the v row of key 0 bit for bit"""
    kvh = 2
    for lens in P.ATTN_SEQS:
        q, kc, vc, o64, o32 = P.attn_case(lens, dh, G, kvh)
        noise, tol = P.tol_of(o32, o64)
        n, off = o64.size, 8
        out = api.k_lm_prefill_attention(q, kc, vc, [0] * len(lens), list(lens), kvh * G, _guarded(n, off), off)
        o = out[off:off + n].reshape(o64.shape)
        err = float(np.abs(o.astype(np.float64) - o64).max())
        print(f"lm_prefill_attention dh={dh} G={G} lens={lens}: noise {noise:.3e} tol {tol:.3e} error {err:.3e} ({err / tol:.3f} tol)")
        assert np.isfinite(o).all() and err <= tol, (dh, G, lens, err, tol)
        assert (out[:off] == GUARD).all() and (out[off + n:] == GUARD).all()
        row = 0
        for i, T in enumerate(lens):
            want = np.repeat(vc[i, :, 0, :], G, axis=0).reshape(-1)          # head h reads kv head h // G
            assert o[row].tobytes() == want.tobytes(), (dh, G, lens, i)
            row += T


def test_queries_that_start_inside_the_cache_equal_the_same_positions_of_a_full_call():
    """positions 40 .. 139 of a 140-position sequence as one call's queries (their tiles cut at 40 and at 64 and 128): the bits of the full call's rows"""
    q, kc, vc, _, _ = P.attn_case((4, 140), 20, 3)
    H = 6
    full = api.k_lm_prefill_attention(q, kc, vc, [0, 0], [4, 140], H, np.zeros(q.size, np.float32), 0).reshape(144, -1)
    part = api.k_lm_prefill_attention(np.concatenate([q[2:4], q[4 + 40:]]), kc, vc, [2, 40], [2, 100], H, np.zeros(102 * H * 20, np.float32), 0).reshape(102, -1)
    assert part[:2].tobytes() == full[2:4].tobytes() and part[2:].tobytes() == full[44:].tobytes()


def test_a_nan_in_one_sequences_cache_stays_in_that_sequence():
    q, kc, vc, _, _ = P.attn_case((31, 32, 33), 12, 3)
    clean = api.k_lm_prefill_attention(q, kc, vc, [0, 0, 0], [31, 32, 33], 6, np.zeros(q.size, np.float32), 0).reshape(96, -1)
    kc = kc.copy()
    kc[1, 0, 5, 3] = np.nan
    o = api.k_lm_prefill_attention(q, kc, vc, [0, 0, 0], [31, 32, 33], 6, np.zeros(q.size, np.float32), 0).reshape(96, -1)
    assert o[:31].tobytes() == clean[:31].tobytes() and o[63:].tobytes() == clean[63:].tobytes()
    seq1 = o[31:63].reshape(32, 6, 12)
    assert np.isnan(seq1[5:, :3]).all()                                         # kv head 0 serves heads 0 .. 2: every query from position 5 on sees the key
    assert seq1[:5].tobytes() == clean[31:36].tobytes() and seq1[:, 3:].tobytes() == clean[31:63].reshape(32, 6, 12)[:, 3:].tobytes()
