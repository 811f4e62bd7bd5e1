"""The two flash-attention kernels called directly (api.k_mha_attention / api.k_relpos_attention), not through an engine graph: the
reference is the attention alone in f64 (synth/attention_cases.py), tol = max(16 noise, 2^-19) with noise = max |numpy f32 - f64| on these very inputs.
What the engine tests cannot reach: row strides and offsets (q / k / v interleaved in one tensor, or padded with NaN between the rows), every
instantiation DH16 = ceil(dh / 16) = 1..4 of both kernels with partial groups, dh = 4, the tile edges of Tq and Tk, the relpos launches above 64 KB of LDS,
scores of +-200 (a running maximum that must rise in every block, or blocks that underflow to 0), and the bytes around the output.
Every run: o sits between two guards of 64 sentinel floats in a sentinel-filled buffer; afterwards the guards are untouched, no output element still holds
the sentinel, the output is finite and within tol of f64.  All layouts of a case, and a second run, give identical bytes."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import attention_cases as ac

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = np.uint32(0x7FA5C3E1)      # a NaN with a payload: no finite output equals it, and a copy of it is recognised by its bits


def _o_io(n):
    return np.full(GUARD + n + GUARD, SENTINEL, np.uint32).view(np.float32)


def _checked_output(out, n, what):
    """the guards are bit-for-bit what went in and every output element was written -> the output"""
    bits = out.view(np.uint32)
    assert out.size == GUARD + n + GUARD
    assert (bits[:GUARD] == SENTINEL).all() and (bits[GUARD + n:] == SENTINEL).all(), f"{what}: a guard word changed"
    assert not (bits[GUARD:GUARD + n] == SENTINEL).any(), f"{what}: {int((bits[GUARD:GUARD + n] == SENTINEL).sum())} output elements were never written"
    o = out[GUARD:GUARD + n]
    assert np.isfinite(o).all(), f"{what}: non-finite output"
    return o


# ------------------------------------------------------------------------------------------------ mha_attention
#            N   Tq  Tk nh  dh  family     scale_pre
MHA_CASES = [(1, 1, 1, 1, 4, "normal", False),        # DH16 = 1.  one query, one key, the smallest head: every load is clamped to column 0
             (1, 3, 31, 1, 4, "equal", True),         # one key short of a block
             (1, 64, 65, 1, 4, "equal", False),       # one key past two blocks
             (2, 65, 97, 2, 12, "rising", False),     # a partial group below 16; four blocks, a query tail, two images
             (2, 33, 33, 2, 12, "normal", True),
             (1, 16, 64, 3, 16, "falling", True),     # exactly two blocks: no tail, even block count
             (1, 63, 32, 2, 16, "normal", False),     # exactly one block, one query short of a tile
             (2, 65, 33, 3, 20, "normal", False),     # DH16 = 2
             (1, 129, 65, 2, 32, "rising", True),     # three query tiles, the last holding one query
             (1, 64, 64, 2, 20, "falling", False),
             (1, 16, 97, 1, 32, "equal", True),
             (1, 1, 97, 2, 20, "normal", True),
             (2, 65, 97, 3, 36, "normal", False),     # DH16 = 3
             (1, 129, 65, 1, 48, "rising", False),
             (1, 63, 64, 2, 36, "falling", True),
             (1, 65, 65, 2, 48, "equal", False),
             (1, 64, 1, 1, 36, "normal", True),       # one key: o is the v row
             (1, 16, 31, 2, 48, "normal", False),
             (2, 70, 33, 2, 52, "normal", True),      # DH16 = 4
             (1, 64, 64, 2, 64, "rising", False),
             (1, 129, 97, 1, 52, "falling", False),
             (1, 65, 32, 2, 64, "equal", True),
             (2, 63, 65, 1, 64, "normal", False),
             (1, 1, 64, 2, 52, "rising", True),
             (1, 16, 32, 1, 64, "normal", True)]
MHA_IDS = ["N%d_Tq%d_Tk%d_nh%d_dh%d_%s_%s" % (c[:6] + ("pre" if c[6] else "post",)) for c in MHA_CASES]

_cache = {}


def _mha_case(case):
    """inputs and the reference bundle: computed once, never modified"""
    if case not in _cache:
        N, Tq, Tk, nh, dh, family, pre = case
        q, k, v = ac.mha_inputs(family, N, Tq, Tk, nh, dh, seed=21)
        _cache[case] = (q, k, v, ac.reference_bundle(ac.mha_core, q, k, v, ac.scale_of(dh), pre))
    return _cache[case]


def _mha_run(case, q, k, v, layout):
    N, Tq, Tk, nh, dh, _, pre = case
    L = ac.mha_layout(layout, q, k, v)
    n = N * Tq * nh * dh
    out = api.k_mha_attention(L["buf"], L["q_off"], L["k_off"], L["v_off"], L["ldq"], L["ldk"], L["ldv"], N, Tq, Tk, nh, dh, float(ac.scale_of(dh)), pre, _o_io(n), GUARD)
    return _checked_output(out, n, f"{case} {layout}").reshape(N, Tq, nh * dh)


def test_the_case_list_covers_what_it_claims():
    dh16 = lambda c: (c[4] + 15) // 16
    assert {c[4] for c in MHA_CASES} == {4, 12, 16, 20, 32, 36, 48, 52, 64}
    assert {c[2] for c in MHA_CASES} == {1, 31, 32, 33, 64, 65, 97}
    assert {c[1] for c in MHA_CASES} >= {1, 16, 63, 64, 65, 129}
    assert {c[6] for c in MHA_CASES} == {False, True}
    for d in (1, 2, 3, 4):
        mine = [c for c in MHA_CASES if dh16(c) == d]
        assert {c[5] for c in mine} == set(ac.FAMILIES), d
        assert any(c[2] > 64 and c[1] % 64 for c in mine), d                  # more than two key blocks together with a query tail
        assert any(c[1] == c[2] for c in mine), d                             # a case the fused layouts can run
    assert any(c[0] == 2 and c[1] % 64 for c in MHA_CASES)                    # two images together with a query tail
    assert all(c[2] >= 64 for c in MHA_CASES if c[5] in ("rising", "falling"))
    assert len(set(MHA_CASES)) == len(MHA_CASES)


@pytest.mark.parametrize("case", MHA_CASES, ids=MHA_IDS)
def test_mha_attention_matches_f64_in_every_layout(case):
    N, Tq, Tk, nh, dh, family, pre = case
    q, k, v, ref = _mha_case(case)
    layouts = [lay for lay in ac.LAYOUTS if Tq == Tk or lay in ("dense", "padded")]
    outs = {lay: _mha_run(case, q, k, v, lay) for lay in layouts}
    err = float(np.abs(outs["dense"].astype(np.float64) - ref["f64"]).max())
    print(f"mha {case} {'+'.join(layouts)}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    assert outs["dense"].shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])
    for lay in layouts[1:]:                                                   # the loop's arithmetic does not depend on addresses
        assert outs[lay].tobytes() == outs["dense"].tobytes(), f"{lay} differs from dense by {np.abs(outs[lay] - outs['dense']).max():.3e}"
    assert _mha_run(case, q, k, v, "dense").tobytes() == outs["dense"].tobytes()   # run to run
    if Tk == 1:                                                               # p = 1, l = 1: o is the v row, bit for bit
        assert outs["dense"].tobytes() == np.broadcast_to(v.reshape(N, 1, nh * dh), (N, Tq, nh * dh)).tobytes()
    if family == "equal":                                                     # a miscounted tail key shows at full size: the mean over exactly Tk keys
        assert np.abs(outs["dense"] - v.astype(np.float64).mean(1).reshape(N, 1, nh * dh)).max() <= ref["tol"]


# ------------------------------------------------------------------------------------------------ relpos_attention
#               B   H   W nh  dh ws  bias   family    scale_pre
RELPOS_CASES = [(1, 4, 8, 1, 4, 0, True, "normal", False),        # exactly 32 keys, DH16 = 1
                (1, 4, 8, 1, 4, 0, True, "rising", True),
                (1, 8, 8, 2, 20, 0, True, "normal", True),        # exactly 64 keys, one full query tile, DH16 = 2
                (1, 8, 8, 2, 20, 0, True, "rising", False),
                (2, 5, 13, 1, 36, 0, True, "normal", False),      # 65 keys, DH16 = 3 partial, a batch stride
                (2, 5, 13, 1, 36, 0, True, "rising", True),
                (1, 1, 7, 1, 48, 0, True, "normal", True),        # a one-row grid
                (1, 1, 7, 1, 48, 0, True, "rising", False),
                (1, 7, 1, 1, 48, 0, True, "normal", False),       # a one-column grid
                (1, 7, 1, 1, 48, 0, True, "rising", True),
                (1, 9, 11, 3, 52, 6, True, "normal", False),      # windows padded on both axes, the padding keys carrying bqkv ...
                (1, 9, 11, 3, 52, 6, True, "rising", True),
                (1, 9, 11, 3, 52, 6, False, "normal", True),      # ... or zeros
                (1, 9, 11, 3, 52, 6, False, "rising", False),
                (1, 8, 8, 1, 32, 8, True, "normal", True),        # the window is the grid
                (1, 8, 8, 1, 32, 8, True, "rising", False),
                (1, 64, 64, 1, 4, 0, True, "rising", False),      # 68,352 bytes of LDS: the opt-in above 64 KB, DH16 = 1
                (1, 60, 62, 1, 64, 0, True, "normal", True)]      # 66,816 bytes: the opt-in of another instantiation, DH16 = 4
RELPOS_IDS = ["B%d_H%d_W%d_nh%d_dh%d_ws%d_%s_%s_%s" % (c[:6] + ("bias" if c[6] else "nobias", c[7], "pre" if c[8] else "post")) for c in RELPOS_CASES]


def _relpos_run(case, qkv, rh, rw, bqkv):
    B, H, W, nh, dh, ws, _, _, pre = case
    n = B * H * W * nh * dh
    out = api.k_relpos_attention(qkv, B, H, W, ws, nh, dh, rh, rw, bqkv, float(ac.scale_of(dh)), pre, _o_io(n), GUARD)
    return _checked_output(out, n, str(case)).reshape(B * H * W, nh * dh)      # (every token is a real one: each row of o must have been written)


def test_the_relpos_case_list_covers_what_it_claims():
    grid = lambda c: (c[5], c[5]) if c[5] else (c[1], c[2])
    lds = lambda c: 34816 + 256 + 256 * ((grid(c)[0] | 1) + (grid(c)[1] | 1))                               # kernels.h: relpos_attention_lds_bytes
    assert {(c[4] + 15) // 16 for c in RELPOS_CASES} == {1, 2, 3, 4}
    assert sorted({(lds(c), (c[4] + 15) // 16) for c in RELPOS_CASES if lds(c) > 65536}) == [(66816, 4), (68352, 1)]
    assert {grid(c)[0] * grid(c)[1] for c in RELPOS_CASES} >= {32, 64, 65, 7, 36}
    assert {c[7] for c in RELPOS_CASES} == {"normal", "rising"} and {c[8] for c in RELPOS_CASES} == {False, True} and {c[6] for c in RELPOS_CASES} == {False, True}


@pytest.mark.parametrize("case", RELPOS_CASES, ids=RELPOS_IDS)
def test_relpos_attention_matches_f64(case):
    B, H, W, nh, dh, ws, bias, family, pre = case
    qkv, rh, rw, bqkv = ac.relpos_inputs(family, B, H, W, nh, dh, ws, seed=23, bias=bias)
    ref = ac.reference_bundle(ac.relpos_core, qkv, rh, rw, bqkv, B, H, W, ws, nh, dh, ac.scale_of(dh), pre)
    o = _relpos_run(case, qkv, rh, rw, bqkv)
    err = float(np.abs(o.astype(np.float64) - ref["f64"]).max())
    print(f"relpos {case}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    assert o.shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])
    assert _relpos_run(case, qkv, rh, rw, bqkv).tobytes() == o.tobytes()       # run to run


# ------------------------------------------------------------------------------------------------ rejected arguments: checks, not launches
def test_rejected_arguments_are_reported_and_nothing_is_launched():
    z = lambda n: np.zeros(n, np.float32)

    def mha(code, buf_floats=120, q_off=0, k_off=40, v_off=80, ld=8, dh=4, o_floats=40, o_off=0):
        with pytest.raises(api.OCRError) as e:
            api.k_mha_attention(z(buf_floats), q_off, k_off, v_off, ld, ld, ld, 1, 5, 5, 2, dh, 0.5, False, z(o_floats), o_off)
        assert e.value.code == code, (e.value.code, str(e.value))
    mha(api.OAR_UNSUPPORTED_OP, dh=6)
    mha(api.OAR_UNSUPPORTED_OP, dh=68, buf_floats=3 * 5 * 136, k_off=680, v_off=1360, ld=136, o_floats=680)
    mha(api.OAR_INVALID_INPUT, v_off=84)            # the v view ends 4 floats behind the buffer
    mha(api.OAR_INVALID_INPUT, buf_floats=116)
    mha(api.OAR_INVALID_INPUT, k_off=42)            # misaligned
    mha(api.OAR_INVALID_INPUT, o_off=2, o_floats=44)
    mha(api.OAR_INVALID_INPUT, o_off=4)             # the output ends behind o_io
    mha(api.OAR_INVALID_INPUT, ld=12)               # rows 12 floats apart need 3 * 56 floats

    def relpos(code, H=3, W=5, ws=0, dh=4, rh=True, rw=True, o_off=0):
        gh, gw = (ws, ws) if ws else (H, W)
        with pytest.raises(api.OCRError) as e:
            api.k_relpos_attention(z(H * W * 3 * 2 * dh), 1, H, W, ws, 2, dh, z(gh * dh * gh) if rh else None, z(gw * dh * gw) if rw else None, None, 0.5, True,
                                   z(H * W * 2 * dh + 8), o_off)
        assert e.value.code == code, (e.value.code, str(e.value))
    relpos(api.OAR_UNSUPPORTED_OP, dh=6)
    relpos(api.OAR_UNSUPPORTED_OP, dh=68)
    relpos(api.OAR_UNSUPPORTED_OP, ws=65)
    relpos(api.OAR_UNSUPPORTED_OP, H=65, W=3)
    relpos(api.OAR_INVALID_INPUT, rh=False)
    relpos(api.OAR_INVALID_INPUT, rw=False)
    relpos(api.OAR_INVALID_INPUT, o_off=2)
    relpos(api.OAR_INVALID_INPUT, o_off=12)
    # and the library still works afterwards
    q, k, v, ref = _mha_case(MHA_CASES[0])
    assert np.abs(_mha_run(MHA_CASES[0], q, k, v, "dense") - ref["f64"]).max() <= ref["tol"]
