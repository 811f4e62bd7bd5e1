"""The split-key decode attention (lm_decode_split.hip) without a GPU: the arithmetic of csrc/lm_decode.h compiled for the host against the same formulas
in Python, the public names, the argument checks that run before a device is asked for, and the sensitivity of the cases of synth/lm_split_cases.py: losing any one
key at a span edge moves the f64 output of every head by at least 4 tol."""
import inspect

import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_split_cases as S


def test_header_arithmetic():
    keys = (1, 63, 64, 65, 127, 128, 129, 192, 193, 2048, 2049, 4096)
    for sk in (64, 128, 192, 4096):
        g = S.split_arithmetic(sk, heads=16, dh=128, maxpos=4096, layers=18, n_keys=keys)
        assert g["supported"] == 1
        assert g["spans"] == {n: -(-n // sk) for n in keys}                                     # spans of a row that sees n = p + 1 keys
        assert g["ws_bytes"] == 16 * 16 * -(-4096 // sk) * (128 + 2) * 4                        # [16 rows][H][ceil(maxpos / S)][dh + 2] floats
        assert g["launches"] == 6 * 18 + 2 and g["launches_serial"] == 5 * 18 + 2
    for bad in (0, 32, 63, 65, 96, 4160, 8192, -64):
        assert S.split_arithmetic(bad)["supported"] == 0, bad
    g = S.split_arithmetic()
    assert (g["threads"], g["tile"], g["min"], g["max"], g["merge_threads"]) == (256, 64, 64, 4096, 128)
    assert g["default"] % 64 == 0 and 64 <= g["default"] <= 4096
    assert g["stop_stride"] >= 1 and g["stop_lookahead"] >= 1 and g["stop_ring"] * g["stop_stride"] > g["stop_lookahead"] + 2 * g["stop_stride"]   # no slot is reused while a copy the host may still read is in it
    assert g["gt"] == {G: (8 if G >= 8 else 4 if G > 2 else G) for G in range(1, 17)}
    for dh, ldk in g["ldk"].items():
        assert ldk in (dh, dh + 4) and (ldk // 4) % 2 == 1                                      # an odd number of float4s: 16 rows read 16 bytes at a time cover 64 banks
        for gt in (1, 2, 4, 8):
            assert g["lds"][(dh, gt)] == 4 * (gt * dh + 64 * ldk + 64 * dh + gt * 64)           # q | K tile | V tile | weights
    assert g["lds"][(128, 8)] == 72704 and 2 * g["lds"][(128, 8)] <= 160 * 1024


def test_the_public_names_exist():
    assert {"oar_lm_set_decode", "oar_lm_decode_stats", "oar_k_lm_decode_attention"} <= set(api.EXPORTS)
    for fn in (vl.CausalLM.generate, vl.PaddleOCRVL.generate_tokens):
        sig = inspect.signature(fn).parameters
        assert sig["decode_attention"].default == "serial" and sig["split_keys"].default is None and sig["stop_at_eos"].default is False
    sig = inspect.signature(vl.CausalLM.set_decode).parameters
    assert sig["attention"].default == "serial" and sig["split_keys"].default is None and sig["stop_at_eos"].default is False
    assert vl.ATTENTION_MODES == {"serial": 0, "split": 1} and hasattr(vl.CausalLM, "decode_stats")
    assert inspect.signature(api.k_lm_decode_attention).parameters["split_keys"].default == 0


def _code(fn, *a, **kw):
    with pytest.raises(api.OCRError) as e:
        fn(*a, **kw)
    return e.value.code


def test_unknown_mode_names_are_refused_without_a_device():
    lm = vl.CausalLM(None, None)
    assert _code(lm.set_decode, "flash") == api.OAR_INVALID_INPUT
    assert _code(lm.generate, input_ids=[1, 2], decode_attention="splitk") == api.OAR_INVALID_INPUT
    assert _code(lm.generate, input_ids=[1, 2], prefill="matmul", decode_attention="split") == api.OAR_INVALID_INPUT
    m = vl.PaddleOCRVL.__new__(vl.PaddleOCRVL)
    assert _code(m.generate_tokens, [], [1], [2], decode_attention="both") == api.OAR_INVALID_INPUT
    L = vl._lib()
    assert L.oar_lm_set_decode(None, 0, 0, 0) == api.OAR_INVALID_INPUT and L.oar_lm_decode_stats(None, None, None) == api.OAR_INVALID_INPUT


def test_lm_decode_attention_refuses_bad_arguments_before_it_asks_for_a_device():
    kc = np.zeros((2, 2, 10, 8), np.float32)
    q = np.zeros((3, 4 * 8), np.float32)
    o = np.zeros(3 * 32 + 4, np.float32)
    f = api.k_lm_decode_attention
    assert _code(f, None, kc, kc, [0, 1, 1], [3, 4, 9], 4, o, 0) == api.OAR_INVALID_INPUT
    assert _code(f, q, kc, kc, [0, 1, 1], [3, 4, 9], 4, o, 2) == api.OAR_INVALID_INPUT                       # o_off no multiple of 4
    assert _code(f, q, kc, kc, [0, 1, 1], [3, 4, 9], 4, o, 8) == api.OAR_INVALID_INPUT                       # does not fit
    assert _code(f, np.zeros((3, 3 * 8), np.float32), kc, kc, [0, 1, 1], [3, 4, 9], 3, o, 0) == api.OAR_INVALID_INPUT   # 3 heads on 2 kv heads
    assert _code(f, q, kc, kc, [0, 1, 1], [3, 4, 10], 4, o, 0) == api.OAR_INVALID_INPUT                      # position 10 of a cache of 10
    assert _code(f, q, kc, kc, [0, 1, 1], [3, -1, 9], 4, o, 0) == api.OAR_INVALID_INPUT
    assert _code(f, q, kc, kc, [0, 2, 1], [3, 4, 9], 4, o, 0) == api.OAR_INVALID_INPUT                       # sequence 2 of 2
    assert _code(f, q, kc, kc, [0, -1, 1], [3, 4, 9], 4, o, 0) == api.OAR_INVALID_INPUT
    assert _code(f, q[:0], kc, kc, [], [], 4, o, 0) == api.OAR_INVALID_INPUT                                 # no row
    assert _code(f, np.zeros((17, 32), np.float32), kc, kc, [0] * 17, [1] * 17, 4, np.zeros(17 * 32, np.float32), 0) == api.OAR_INVALID_INPUT   # 17 rows
    for sk in (32, 65, 96, 4160, -64):
        assert _code(f, q, kc, kc, [0, 1, 1], [3, 4, 9], 4, o, 0, split_keys=sk) == api.OAR_INVALID_INPUT, sk
    for dh in (4, 6, 132):
        k2 = np.zeros((2, 2, 10, dh), np.float32)
        for sk in (0, 64):
            assert _code(f, np.zeros((3, 4 * dh), np.float32), k2, k2, [0, 1, 1], [3, 4, 9], 4, np.zeros(3 * 4 * dh, np.float32), 0, split_keys=sk) == api.OAR_UNSUPPORTED_OP
    with pytest.raises(ValueError):
        f(q[:2], kc, kc, [0, 1, 1], [3, 4, 9], 4, o, 0)
    with pytest.raises(ValueError):
        f(q, kc, kc[:1], [0, 1, 1], [3, 4, 9], 4, o, 0)
    with pytest.raises(ValueError):
        f(q, kc, kc, [0, 1], [3, 4, 9], 4, o, 0)


def test_the_rows_of_the_cases():
    assert S.SPLIT_LENS == (1, 193, 130) and S.SPLIT_KEYS == 64
    assert S.ROWS == ((1, 62), (1, 63), (1, 64), (1, 126), (1, 127), (1, 128), (1, 191), (1, 192), (0, 0), (2, 129), (2, 64))
    c = S.split_case(12, 3)
    assert c["q"].shape == (11, 2 * 3 * 12) and c["kc"].shape == (3, 2, 196, 12) and c["o64"].shape == (11, 72)
    assert (c["kc"][1, :, 193:] == np.float32(1e30)).all() and (c["vc"][0, :, 1:] == np.float32(1e30)).all()      # the unused positions show a kernel that reads them
    assert c["tol"] == max(16.0 * c["noise"], 2.0 ** -19)
    for row in range(11):                                                                                         # attend64 is the reference's own arithmetic
        assert np.abs(S.attend64(c, row).reshape(-1) - c["o64"][row]).max() < 1e-12
    assert S.sensitive_keys(62) == [0, 61, 62] and S.sensitive_keys(64) == [0, 62, 63, 64]
    assert S.sensitive_keys(192) == [0, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192]


@pytest.mark.parametrize("dh", S.DHS)
def test_losing_one_key_moves_every_head_by_four_tol(dh):
    """rows that see 63 .. 193 keys of the 193-position sequence, S = 64: without key 0, 62 .. 65, 126 .. 129, 191, 192, p - 1 or p (those the row sees) the f64
    output of every head moves by at least 4 tol, tol being tol_of over all query rows of attn_case (at least the tol of the call's 11 rows, which the kernels are
    held to).  Seed 0, on the CPU this was written on: the least movement over all head sizes and group sizes is 6.9 tol (head size 12, G = 8)."""
    for G in S.GS:
        c = S.split_case(dh, G)
        least = S.least_movement(c)
        print(f"dh={dh} G={G}: noise {c['noise_all']:.3e} tol {c['tol_all']:.3e} least movement {least / c['tol_all']:.1f} tol ({least / c['tol']:.1f} of the 11 rows' tol)")
        assert c["tol_all"] >= c["tol"]
        assert least >= S.SENSITIVITY_TOLS * c["tol_all"], (dh, G, least, c["tol_all"])
