"""The cases of the GEMM-based prefill (synth/lm_prefill_cases.py) without a GPU: the tile-edge prompts are greedy-safe (the f64 margin between the best
and the second-best logit exceeds 4 tol at every forced step), the tile and chunk arithmetic of csrc/lm_prefill.h compiled for the host is what the design says, and the
two direct kernel entries refuse bad arguments before they ask for a device."""
import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_prefill_cases as P
from oar_ocr_amd.synth import lm_reference as R


@pytest.mark.parametrize("name", list(P.EDGE_CASES))
def test_the_tile_edge_prompts_are_greedy_safe(name):
    ref = P.edge_reference_for(name)
    assert [p[0].shape[0] - 1 for p in ref["prompts"]] == [63, 64, 65, 128]          # one short of a tile, a tile, one past it, two tiles
    assert ref["tol"] == max(16.0 * ref["noise"], 2.0 ** -19)
    for i, (t64, l64) in enumerate(ref["runs"]):
        m = R.greedy_margins(l64)
        print(f"{name} T={P.EDGE_LENGTHS[i]}: noise {ref['noise']:.3e} tol {ref['tol']:.3e} least margin {m.min() / ref['tol']:.1f} tol")
        assert len(t64) == P.EDGE_STEPS and m.min() > P.EDGE_MARGIN_TOLS * ref["tol"], (name, i, m.min(), ref["tol"])


def test_the_edge_cases_are_the_geometries_of_a_and_la():
    import dataclasses
    for mine, theirs in (("TA", R.CASES["A"]), ("TLA", R.LONG_CASES["LA"][0])):
        a, b = dataclasses.asdict(P.EDGE_CASES[mine]), dataclasses.asdict(theirs)
        a.pop("name"), b.pop("name")
        assert a == b


def test_tile_table_of_lengths_1_64_65_506():
    """GEMM rows are positions 0 .. T - 2: 0, 63, 64 and 505 of them; tiles are aligned to the sequence's own positions, two heads"""
    g = P.prefill_arithmetic((1, 64, 65, 506), heads=2, chunk_rows=2048)
    assert g["default_chunk"] == 2048 and g["max_chunk"] == 65536
    assert len(g["chunks"]) == 1 and g["launches"] == 5 * 2 + 1
    c = g["chunks"][0]
    assert c["rows"] == 63 + 64 + 505
    assert c["spans"] == [[1, 0, 63, 0], [2, 0, 64, 63], [3, 0, 505, 127]]              # the one-position prompt has no row
    want = []
    for seq, n, row0 in ((1, 63, 0), (2, 64, 63), (3, 505, 127)):
        for h in range(2):
            for qt in range(-(-n // 64)):
                want.append([seq, h, qt, 64 * qt, min(64 * qt + 64, n), row0 + 64 * qt])
    assert c["tiles"] == want and c["count"] == len(want) == 2 * (1 + 1 + 8)


def test_chunk_cuts_keep_the_tiles_aligned_to_the_sequence():
    """chunks of 100 rows over (1, 64, 65, 506): 63 + 37 | 27 + 73 | 100 x 4 | 32; a tile that a chunk cuts appears in both chunks with its own [lo, hi), the same qt"""
    g = P.prefill_arithmetic((1, 64, 65, 506), heads=1, chunk_rows=100)
    ch = g["chunks"]
    assert [c["rows"] for c in ch] == [100, 100, 100, 100, 100, 100, 32] and g["launches"] == 7 * 11
    assert ch[0]["spans"] == [[1, 0, 63, 0], [2, 0, 37, 63]] and ch[1]["spans"] == [[2, 37, 27, 0], [3, 0, 73, 27]]
    assert ch[0]["tiles"] == [[1, 0, 0, 0, 63, 0], [2, 0, 0, 0, 37, 63]]
    assert ch[1]["tiles"] == [[2, 0, 0, 37, 64, 0], [3, 0, 0, 0, 64, 27], [3, 0, 1, 64, 73, 91]]
    assert ch[2]["spans"] == [[3, 73, 100, 0]] and ch[2]["tiles"] == [[3, 0, 1, 73, 128, 0], [3, 0, 2, 128, 173, 55]]
    assert ch[6]["spans"] == [[3, 473, 32, 0]] and ch[6]["tiles"] == [[3, 0, 7, 473, 505, 0]]
    # every position of every sequence is a query exactly once, in a tile qt = position // 64
    seen = {}
    for c in ch:
        assert c["count"] == len(c["tiles"])
        for seq, _, qt, lo, hi, row_lo in c["tiles"]:
            assert 64 * qt <= lo < hi <= 64 * qt + 64 and 0 <= row_lo and row_lo + hi - lo <= c["rows"]
            for p in range(lo, hi):
                assert (seq, p) not in seen
                seen[(seq, p)] = 1
    assert len(seen) == 63 + 64 + 505
    one = P.prefill_arithmetic((1, 64, 65, 506), heads=1, chunk_rows=1)
    assert len(one["chunks"]) == 632 and all(c["rows"] == 1 and len(c["tiles"]) == 1 for c in one["chunks"])
    assert P.prefill_arithmetic((1, 1, 1), heads=3, chunk_rows=16)["chunks"] == []


def test_lds_bytes_of_the_two_kernels():
    g = P.prefill_arithmetic((2,))
    assert g["gemm_lds"] == 2 * (64 + 64) * 36 * 4 + 64 * 4                             # two stages of 64 weight rows and 64 tokens, 32 + 4 columns; 1 / rms per token
    for dh, b in g["attn_lds"].items():
        ld = 16 * ((dh + 15) // 16) + 4
        assert b == 2 * 2 * 32 * ld * 4 and (ld // 4) % 2 == 1 and ld >= dh + 4, (dh, b)
    assert g["attn_lds"][128] == 67584 and g["attn_lds"][8] == 10240 and 2 * g["attn_lds"][128] <= 160 * 1024


def _code(fn, *a, **kw):
    with pytest.raises(api.OCRError) as e:
        fn(*a, **kw)
    return e.value.code


def test_lm_gemm_refuses_bad_arguments_before_it_asks_for_a_device():
    x, w = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    o = np.zeros(15, np.float32)
    assert _code(api.k_lm_gemm, None, w, o, 0, m=3, k=8) == api.OAR_INVALID_INPUT
    assert _code(api.k_lm_gemm, x, None, o, 0, n=5) == api.OAR_INVALID_INPUT
    assert _code(api.k_lm_gemm, x, w, o, 1) == api.OAR_INVALID_INPUT                    # 1 + 15 floats do not fit 15
    assert _code(api.k_lm_gemm, x, w, o[:14], 0) == api.OAR_INVALID_INPUT
    assert _code(api.k_lm_gemm, x, w, o, 16) == api.OAR_INVALID_INPUT
    assert _code(api.k_lm_gemm, x[:0], w, o, 0, m=0, k=8) == api.OAR_INVALID_INPUT
    assert _code(api.k_lm_gemm, x, w[:0], o, 0, n=0) == api.OAR_INVALID_INPUT
    assert _code(api.k_lm_gemm, np.zeros((3, 6), np.float32), np.zeros((5, 6), np.float32), o, 0) == api.OAR_UNSUPPORTED_OP   # k no multiple of 4
    L = api.lib()
    assert L.oar_k_lm_gemm(x.ctypes.data, 3, 8, w.ctypes.data, 2, 5, o.ctypes.data, 15, 0) == api.OAR_INVALID_INPUT           # no such dtype
    with pytest.raises(ValueError):
        api.k_lm_gemm(x, w[:, :4], o, 0)


def test_lm_prefill_attention_refuses_bad_arguments_before_it_asks_for_a_device():
    kc = np.zeros((2, 2, 10, 8), np.float32)
    q = np.zeros((7, 4 * 8), np.float32)
    o = np.zeros(7 * 32 + 4, np.float32)
    f = api.k_lm_prefill_attention
    assert _code(f, None, kc, kc, [0, 0], [3, 4], 4, o, 0) == api.OAR_INVALID_INPUT
    assert _code(f, q, kc, kc, [0, 0], [3, 4], 4, o, 2) == api.OAR_INVALID_INPUT                      # o_off no multiple of 4
    assert _code(f, q, kc, kc, [0, 0], [3, 4], 4, o, 8) == api.OAR_INVALID_INPUT                      # does not fit
    assert _code(f, np.zeros((6, 3 * 8), np.float32), kc, kc, [0, 0], [3, 3], 3, o, 0) == api.OAR_INVALID_INPUT                  # 3 heads on 2 kv heads
    assert _code(f, q[:3], kc, kc, [0, 0], [3, 0], 4, o, 0) == api.OAR_INVALID_INPUT                  # an empty sequence
    assert _code(f, q, kc, kc, [0, 7], [3, 4], 4, o, 0) == api.OAR_INVALID_INPUT                      # positions 7 .. 10 of a cache of 10
    assert _code(f, q, kc, kc, [0, -1], [3, 4], 4, o, 0) == api.OAR_INVALID_INPUT
    for dh in (4, 6, 132):
        k2 = np.zeros((2, 2, 10, dh), np.float32)
        assert _code(f, np.zeros((7, 4 * dh), np.float32), k2, k2, [0, 0], [3, 4], 4, np.zeros(7 * 4 * dh, np.float32), 0) == api.OAR_UNSUPPORTED_OP
    with pytest.raises(ValueError):
        f(q[:5], kc, kc, [0, 0], [3, 4], 4, o, 0)
    with pytest.raises(ValueError):
        f(q, kc, kc[:1], [0, 0], [3, 4], 4, o, 0)


def test_the_public_names_exist():
    import inspect
    assert {"oar_lm_set_prefill", "oar_lm_prefill_cost", "oar_k_lm_gemm", "oar_k_lm_prefill_attention"} <= set(api.EXPORTS)
    for fn in (vl.CausalLM.generate, vl.PaddleOCRVL.generate_tokens):
        assert inspect.signature(fn).parameters["prefill"].default == "rows"
    assert inspect.signature(vl.CausalLM.generate).parameters["prefill_chunk"].default is None
    assert vl.PREFILL_MODES == {"rows": 0, "gemm": 1} and hasattr(vl.CausalLM, "prefill_cost")
