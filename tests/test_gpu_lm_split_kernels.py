"""The attention of one step of the language-model chain alone, through its direct entry api.k_lm_decode_attention, against f64: the split pair of
lm_decode_split.hip (lm_attn_split + lm_attn_merge over a workspace the entry fills with 0xFF bytes) and, with split_keys = 0, the serial lm_attn_kernel of lm_decode.hip.
Tolerance as everywhere: noise = max |f32 - f64| of the torch reference of the op itself, tol = max(16 noise, 2^-19).  Shapes: synth/lm_split_cases.py."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import lm_split_cases as S

pytestmark = pytest.mark.gpu

GUARD = np.float32(-777.25)
OFF = 8


def _run(c, split_keys, rows=None, kc=None, vc=None):
    """The case's rows `rows` (all 11 when None) as one call: the output [len(rows), heads dh], after the guard words around it have been checked."""
    rows = list(range(len(c["row_seq"]))) if rows is None else list(rows)
    n = len(rows) * c["heads"] * c["dh"]
    buf = np.full(OFF + n + 37, GUARD, np.float32)
    out = api.k_lm_decode_attention(c["q"][rows], c["kc"] if kc is None else kc, c["vc"] if vc is None else vc, c["row_seq"][rows], c["row_pos"][rows], c["heads"], buf, OFF,
                                    split_keys=split_keys)
    assert (out[:OFF] == GUARD).all() and (out[OFF + n:] == GUARD).all()
    return out[OFF:OFF + n].reshape(len(rows), -1)


def _check(c, o, what):
    err = float(np.abs(o.astype(np.float64) - c["o64"]).max())
    print(f"{what} dh={c['dh']} G={c['G']}: noise {c['noise']:.3e} tol {c['tol']:.3e} error {err:.3e} ({err / c['tol']:.3f} tol)")
    assert np.isfinite(o).all() and err <= c["tol"], (what, c["dh"], c["G"], err, c["tol"])


@pytest.mark.parametrize("G", S.GS)
@pytest.mark.parametrize("dh", S.DHS)
def test_split_attention_against_f64(dh, G):
    """the 11-row call (rows that see 63 .. 193 keys of one sequence, the one-position sequence, positions 129 and 64 of a third), split_keys 64, and 128 at two head sizes"""
    c = S.split_case(dh, G)
    for sk in (64, 128) if dh in S.WIDE_DHS else (64,):
        _check(c, _run(c, sk), f"lm_attn_split S={sk}")


@pytest.mark.parametrize("G", S.GS)
@pytest.mark.parametrize("dh", S.DHS)
def test_serial_attention_against_f64(dh, G):
    """the same call through lm_attn_kernel: its first direct test"""
    c = S.split_case(dh, G)
    _check(c, _run(c, 0), "lm_attn serial")


@pytest.mark.parametrize("sk", [0, 64, 128])
def test_a_row_with_one_key_returns_that_keys_values(sk):
    for dh, G in ((8, 12), (80, 3), (128, 8)):
        c = S.split_case(dh, G)
        o = _run(c, sk, rows=[8])                                                   # (sequence 0, position 0)
        want = np.repeat(c["vc"][0, :, 0, :], G, axis=0).reshape(-1)                # head h reads kv head h // G
        assert o[0].tobytes() == want.tobytes(), (sk, dh, G)


@pytest.mark.parametrize("sk", [64, 128])
def test_a_rows_bits_do_not_depend_on_its_slot_or_on_the_other_rows(sk):
    """row (sequence 1, position 128) alone, as the first of 16 rows and in slot 15: the same bits; two runs of the 16-row call: the same bytes"""
    c = S.split_case(20, 7)
    alone = _run(c, sk, rows=[5])
    others = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 0, 3, 7, 9, 10]
    first = _run(c, sk, rows=[5] + others)
    last = _run(c, sk, rows=others + [5])
    again = _run(c, sk, rows=others + [5])
    assert alone[0].tobytes() == first[0].tobytes() == last[15].tobytes()
    assert last.tobytes() == again.tobytes()
    assert first[1:].tobytes() == last[:15].tobytes()
    full = _run(c, sk)
    assert full[5].tobytes() == alone[0].tobytes()


@pytest.mark.parametrize("sk", [0, 64])
def test_a_nan_in_another_sequences_cache_changes_no_byte(sk):
    c = S.split_case(12, 3)
    clean = _run(c, sk)
    kc, vc = c["kc"].copy(), c["vc"].copy()
    kc[1, 0, 5, 3] = np.nan
    vc[1, 1, 70, 0] = np.nan
    o = _run(c, sk, kc=kc, vc=vc)
    mine = c["row_seq"] != 1
    assert o[mine].tobytes() == clean[mine].tobytes()
    seq1 = o[~mine].reshape(8, 2, 3, 12)
    assert np.isnan(seq1[:, 0]).all()                                               # kv head 0 serves heads 0 .. 2; every row of sequence 1 sees key 5
    assert np.isnan(seq1[3:, 1, :, 0]).all() and not np.isnan(seq1[:3, 1]).any()    # the rows from position 126 on see the value at key 70


@pytest.mark.parametrize("sk", [0, 64])
def test_a_nan_just_past_a_rows_position_changes_no_byte_of_the_row(sk):
    c = S.split_case(20, 8)
    clean = _run(c, sk)
    kc, vc = c["kc"].copy(), c["vc"].copy()
    for row in (0, 1, 4, 7, 8, 10):                                                 # positions 62, 63, 127, 192 of sequence 1, 0 of sequence 0, 64 of sequence 2
        s, p = int(c["row_seq"][row]), int(c["row_pos"][row])
        kc2, vc2 = kc.copy(), vc.copy()
        kc2[s, :, p + 1] = np.nan
        vc2[s, :, p + 1] = np.nan
        o = _run(c, sk, rows=[row], kc=kc2, vc=vc2)
        assert o[0].tobytes() == clean[row].tobytes(), (sk, row)


def _code(fn, *a, **kw):
    with pytest.raises(api.OCRError) as e:
        fn(*a, **kw)
    return e.value.code


def test_bad_arguments_return_their_statuses_and_launch_nothing():
    c = S.split_case(8, 1)
    f = api.k_lm_decode_attention
    n = 11 * c["heads"] * 8
    o = np.zeros(n + 4, np.float32)
    api.prof_reset()
    api.prof_enable(True)
    try:
        assert _code(f, c["q"], c["kc"], c["vc"], c["row_seq"], c["row_pos"], c["heads"], o, 2, split_keys=64) == api.OAR_INVALID_INPUT
        assert _code(f, c["q"], c["kc"], c["vc"], c["row_seq"], c["row_pos"], c["heads"], o, 8, split_keys=64) == api.OAR_INVALID_INPUT
        assert _code(f, c["q"], c["kc"], c["vc"], c["row_seq"], c["row_pos"], c["heads"], o, 0, split_keys=96) == api.OAR_INVALID_INPUT
        assert _code(f, c["q"], c["kc"], c["vc"], c["row_seq"], c["row_pos"] + 100, c["heads"], o, 0, split_keys=64) == api.OAR_INVALID_INPUT
        assert _code(f, c["q"], c["kc"], c["vc"], c["row_seq"] + 2, c["row_pos"], c["heads"], o, 0) == api.OAR_INVALID_INPUT
        assert _code(f, None, c["kc"], c["vc"], c["row_seq"], c["row_pos"], c["heads"], o, 0) == api.OAR_INVALID_INPUT
        k4 = np.zeros((1, 1, 4, 4), np.float32)
        assert _code(f, np.zeros((1, 4), np.float32), k4, k4, [0], [0], 1, np.zeros(4, np.float32), 0, split_keys=64) == api.OAR_UNSUPPORTED_OP
        assert not [e for e in api.prof_snapshot() if e["name"].startswith("lm_") and e["launches"]]
        f(c["q"], c["kc"], c["vc"], c["row_seq"], c["row_pos"], c["heads"], o, 4, split_keys=64)
        names = {e["name"]: e["launches"] for e in api.prof_snapshot() if e["name"].startswith("lm_") and e["launches"]}
        assert names == {"lm_attn_split": 1, "lm_attn_merge": 1}, names
    finally:
        api.prof_enable(False)
