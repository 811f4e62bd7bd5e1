"""oar_ocr_amd/synth/chain_cases.py on the CPU: the matrix reaches every path of the chain kernel or lists it in NOT_REACHED, the Python restatement of the
dispatch and of the planner's work split agrees with the C++ sources, every case's LDS tensors stay inside the budget, the numpy reference agrees with the
ONNX oracle on the case's graph, and the tolerance tells nine wrong references from the right one.  tests/test_gpu_chain_kernel.py runs the
same matrix on the GPU."""
import re
from pathlib import Path

import numpy as np

from oar_ocr_amd.synth import chain_cases as C

CSRC = Path(C.__file__).resolve().parent.parent / "csrc"


def _src(name):
    return (CSRC / name).read_text()


def _plans(c):
    """the case's plans: the default child's, and the OAR_CHAIN_LDS=0 child's where the case runs there"""
    return [C.plan(c)] + ([C.plan(c, C.ENV_HBM)] if c.hbm_too else [])


# ------------------------------------------------------------------------------------------------ coverage
def test_matrix_reaches_every_path_or_lists_it():
    reached = set()
    for c in C.CASES:
        if c.overflow:
            continue                      # (no exact plan: the GPU test asserts a general-path product next to an LDS one in its launch)
        for p in _plans(c):
            reached |= p.features
            assert p.name is not None and len(p.name) <= C.K_NAME_FIT and p.name.startswith(f"chain n={c.n} T={c.T} "), (c.name, p.name)
    want = C.features()
    assert reached <= want, sorted(reached - want)
    assert want - reached == set(C.NOT_REACHED), (sorted(want - reached - set(C.NOT_REACHED)), sorted(set(C.NOT_REACHED) - (want - reached)))
    assert len({c.name for c in C.CASES}) == len(C.CASES)


def test_product_rows_take_the_path_the_table_says():
    """DESIGN 4.49's (T, N, K) table: the planner's mb / ksplit / kper and the kernel's path of the product under test"""
    for name, T, N, (cin, kw), _, res, (path, ks, kper) in C.PRODUCT_ROWS:
        c = C.case_by_name(f"product {name} T{T} N{N} K{kw * cin}")
        e = [e for e in C.plan(c).table if e["type"] == "gemm"][-1]
        assert (e["K"], e["N"]) == (kw * cin, N), (c.name, e)
        assert (C.gemm_path(e["in_lds"], e["mb"], e["K"], e["ksplit"]), e["ksplit"], e["kper"]) == (path, ks, kper), (c.name, e)
        assert bool(res) == (e["res"] is not None and e["res_lds"])
    by = {r[0]: C.plan(C.case_by_name(f"product {r[0]} T{r[1]} N{r[2]} K{r[3][0] * r[3][1]}")) for r in C.PRODUCT_ROWS}
    assert "empty slice" in by["short k8 two empty slices"].features              # K = 272: KB = 17, 8 slices of 3 steps: slices 6 and 7 start past KB
    e = [e for e in by["lds3 ragged group"].table if e["type"] == "gemm"][-1]
    assert e["mb"] == 3 and (65 + 15) // 16 == 5                                  # MT = 5, mb = 3: the second group computes a tile past MT


def test_matrix_shapes():
    """the rules of the matrix, computed from the cases alone"""
    assert all(c.n >= 2 for c in C.CASES) and any(c.n >= 9 for c in C.CASES)
    fixed_T = lambda c: c.name.startswith(("product ", "attn ")) or c.overflow                                          # the table's rows, the attention's tile edges
    assert all(c.T % 16 for c in C.CASES if not fixed_T(c))                                                             # ragged wherever T is free
    attn = [(c, next(o for o in c.ops if o.kind == "attn")) for c in C.CASES if any(o.kind == "attn" for o in c.ops)]
    assert {o.hd for _, o in attn} == {4, 8, 12, 16}
    assert {c.T for c, _ in attn} >= {1, 16, 17, 32, 33, 48, 49, 64, 65, 100}
    assert any(o.heads * ((c.T + 15) // 16) > C.K_WAVES and c.T <= 64 for c, o in attn) and any(o.heads == 1 for _, o in attn)
    assert any(o.scale is not None and abs(o.scale - o.hd ** -0.5) > 0.01 for _, o in attn)
    ln = [(c, o, C.widths(c)[i]) for c in C.CASES for i, o in enumerate(c.ops) if o.kind == "ln"]
    assert {w for _, _, w in ln} >= {16, 64, 256, 272, 384} and {o.affine for _, o, _ in ln} == {"gb", "g"}
    assert {c.T for c, _, _ in ln} >= {1, 4, 5, 67}
    pools = [(c, o) for c in C.CASES for o in c.ops if o.kind == "pool"]
    assert {(o.kh, o.kw) for _, o in pools} >= {(6, 2), (4, 2), (5, 3), (8, 8)} and any(c.odd for c, _ in pools) and any(c.c == 20 for c, _ in pools)
    assert any(c.n >= 3 for c, _ in pools)
    prods = [o for c in C.CASES for o in c.ops if o.kind in ("conv", "lin")]
    assert {(o.kw, o.pl) for o in prods if o.kw == 2} == {(2, 0), (2, 1)} and {o.kw for o in prods} == {1, 2, 3, 5}
    assert any(o.act == "hsigmoid" and (o.alpha, o.beta) != (0.2, 0.5) for o in prods)
    assert {c.input for c in C.CASES} == {"tok", "map", "pool"}                   # the run's input: the graph input (kind 2) and arena tensors (kind 1)
    # poison: sample 1, never behind an activation that swallows a NaN; one case per product path, a LayerNorm, an attention, one at token T - 1 of a ragged T
    pois = [c for c in C.CASES if c.poison]
    for c in pois:
        assert c.n >= 2 and 0 <= c.poison[0] < c.T and 0 <= c.poison[1] < c.c and c.input in ("tok", "map"), c.name
        assert all(o.act in C.NAN_KEEPING_ACTS for o in c.ops), c.name
    paths = set()
    for c in pois:
        for p in _plans(c):
            paths |= {t[:2] for t in p.tokens if t[0] == "g"}
    assert paths == {"gs", "g1", "g2", "g3", "gh"}, paths
    assert any(c.ops[0].kind == "ln" for c in pois) and any(o.kind == "attn" for c in pois for o in c.ops)
    assert any(c.poison[0] == c.T - 1 and c.T % 16 for c in pois)
    # `large`: where the QKV product reads the input itself; its scores reach about +-60
    top = 0.0
    for c, _ in attn:
        if not c.name.startswith("attn "):
            continue
        assert "large" in c.families and c.ops[0].kind == "lin" and c.ops[1].kind == "attn", c.name
        st = {}
        C.ref(c, C.case_inputs(c, "large"), "float64", stats=st)
        top = max(top, st["score"])
    print(f"\n[chain] large: the largest |attention score| is {top:.1f}")
    assert 40.0 <= top <= 90.0, top


def test_lds_budget_is_far_away():
    """plan() takes 'written in the run, not read after it -> LDS' for granted: that holds while the planner's first-fit placement (restated: first_fit_peak)
    plus the constants and the table stay inside kChainLdsBudget.  Every case but the recognizer's own neck stays under 60 % of it; the neck, whose shapes
    are the real model's, fits with its constants counted exactly as the planner counts them."""
    for c in C.CASES:
        if c.overflow:
            assert C.plan(c).lds_bytes > C.K_LDS_BUDGET, c.name
            continue
        for p in _plans(c):
            small = sum((e["N"] + 3) // 4 * 4 * (2 if e["type"] == "ln" else 1) for e in p.table if e["type"] in ("gemm", "ln"))
            fixed = ((small * 4 + 255) & ~255) + ((len(p.table) * 128 + 255) & ~255)          # biases / affine vectors, the table (sizeof(ChainOpD) <= 128)
            assert p.lds_bytes + fixed <= (C.K_LDS_BUDGET if c.name.startswith("neck") else 0.6 * C.K_LDS_BUDGET), (c.name, p.lds_bytes, fixed)


# ------------------------------------------------------------------------------------------------ the restatement against the sources
def test_restatement_agrees_with_the_sources():
    kh, ch, en = _src("kernels.h"), _src("chain.hip"), _src("engine.cc")
    assert int(re.search(r"constexpr int kChainMaxHd = (\d+);", kh).group(1)) == C.K_CHAIN_MAX_HD
    assert re.search(r"constexpr size_t kChainLdsBudget = 159 \* 1024;", kh) and C.K_LDS_BUDGET == 159 * 1024
    assert int(re.search(r"static constexpr int kMinChain = (\d+);", en).group(1)) == C.K_MIN_CHAIN
    assert float(re.search(r"max_mflop = mf_env \? atof\(mf_env\) : ([\d.]+);", en).group(1)) == C.K_MAX_MFLOP
    assert int(re.search(r"constexpr size_t kFit = (\d+);", ch).group(1)) == C.K_NAME_FIT
    assert re.search(r"constexpr int kChainThreads = 1024;", ch) and C.K_WAVES == 1024 // 64
    # the product dispatch: kernels.h's chain_gemm_path and the kernel's own switch, condition for condition in the same order
    host = re.findall(r"if \((in_lds[^\n]*?)\) return (CH_G_\w+);", kh)
    dev = re.findall(r"if \((in\.lds[^\n]*?)\) (ch_gemm_lds_short|ch_gemm_lds<\d>)\(", ch)
    fn = {"ch_gemm_lds_short": "CH_G_SHORT", "ch_gemm_lds<1>": "CH_G_LDS1", "ch_gemm_lds<2>": "CH_G_LDS2", "ch_gemm_lds<3>": "CH_G_LDS3"}
    assert len(host) == 4 and [(c.replace("in.lds", "in_lds").replace("op.", ""), fn[f]) for c, f in dev] == host, (host, dev)
    assert re.search(r"else ch_gemm_slow\(", ch) and re.search(r"if \(in_lds\) return CH_G_LDS3;\s*return CH_G_HBM;", kh)
    assert re.search(r"enum ChainGemmPath : int \{ CH_G_SHORT = 0, CH_G_LDS1 = 1, CH_G_LDS2 = 2, CH_G_LDS3 = 3, CH_G_HBM = 4 \};", kh)
    assert 'kPath[] = {"gs", "g1", "g2", "g3", "gh"}' in ch
    for in_lds in (False, True):                                                # ... and the Python one, over the rule's whole domain
        for mb in (1, 2, 3):
            for K in range(16, 1040, 16):
                for ks in (1, 2, 4, 8, 16):
                    want = "gh" if not in_lds else ("gs" if ((K >> 4) + ks - 1) // ks < 4 else "g1") if mb == 1 else "g2" if mb == 2 else "g3"
                    assert C.gemm_path(in_lds, mb, K, ks) == want
    # LayerNorm
    assert "return C <= 256 && (C & 3) == 0; }" in kh and "if (C <= 256 && (C & 3) == 0) {" in ch
    assert [C.ln_float4(v) for v in (4, 18, 256, 260, 272)] == [True, False, True, False, False]
    # attention
    assert "if (T <= 64 && (hd & 3) == 0) return T <= 16 ? 1 : T <= 32 ? 2 : T <= 48 ? 3 : 4;" in kh
    dev = re.search(r"if \(T <= 64 && \(op\.hd & 3\) == 0\) \{(.*?)\} else ch_attention_any<HD>", ch, re.S).group(1)
    assert re.findall(r"(?:if \(T <= (\d+)\) |else )ch_attention_mfma<(\d)>", dev) == [("16", "1"), ("32", "2"), ("48", "3"), ("", "4")]
    assert [C.attn_tiles(T, 16) for T in (1, 16, 17, 32, 33, 48, 49, 64, 65)] == [1, 1, 2, 2, 3, 3, 4, 4, 0] and C.attn_tiles(16, 6) == 0
    # the planner's work split: the expressions mb_ksplit restates, the 24-tile and KB <= 8 limits among them
    assert "d.mb = (NT * MT <= 16 && KB <= 8) ? 1 : (MT <= 3 ? MT : (MT % 3 == 0 ? 3 : (MT % 2 == 0 ? 2 : 3)));" in en
    assert "while (NT * MG * ks < 16 && KB / (ks * 2) >= 2 && NT * MG * d.mb * ks * 2 <= 24) ks *= 2;" in en
    assert "const int kper = (KB + KS - 1) / KS" in ch
    assert "return (size_t)(op.N / 16) * ((MT + mb - 1) / mb) * mb * op.ksplit * 64 * 16;" in ch
    assert C.mb_ksplit(16, 16, 272) == (1, 8, 3) and C.mb_ksplit(65, 64, 64) == (3, 1, 4) and C.mb_ksplit(16, 64, 128) == (1, 4, 2) and C.mb_ksplit(16, 64, 144)[0] == 1
    # the token letters
    for act, letter in (("RELU", "R"), ("HSWISH", "H"), ("HSIGMOID", "G"), ("SIGMOID", "S"), ("SWISH", "W")):
        assert f'case ACT_{act}: t += "{letter}"; break;' in ch
    assert sorted(C.ACT_LETTER.values()) == sorted(["", "R", "H", "G", "S", "W"])


def test_detail_name_forms():
    assert C.detail_name(2, 7, ["c", "gs", "n4"]) == "chain n=2 T=7 c gs n4"
    long = ["g3k4W"] * 10 + ["n4"] * 10 + ["gsk2r"] * 4
    assert C.detail_name(2, 40, long) == "chain n=2 T=40 g3k4Wx10 n4x10 gsk2rx4"
    many = [f"g{p}k{k}{a}" for p in "s123" for k in (2, 4) for a in "RHW"]
    assert C.detail_name(64, 40, many) == "chain n=64 T=40 ~ gsx6 g1x6 g2x6 g3x6"
    neck = C.plan(C.case_by_name("neck tiny T40"))
    assert " n4x5 " in neck.name and len(neck.tokens) == 22 and len(neck.name) <= C.K_NAME_FIT       # the pool, 19 products / LayerNorms / attentions and the pool output's real copy


# ------------------------------------------------------------------------------------------------ references
def test_reference_agrees_with_the_onnx_oracle():
    """ref in float64 against oracle/onnx_ref (f32, torch) run on the case's own graph: equal at float32 rounding.  The oracle is one more f32 evaluation in
    an order of its own (torch's blocked products), so its distance from float64 is of the size of numpy's f32 noise, not equal to it: the bound is 2 tol =
    8 max |f32 numpy - f64|, half of what the weakest wrong edit below must move the output by."""
    from oracle import onnx_ref
    for c in C.CASES:
        for fam in c.families:
            inp = C.case_inputs(c, fam)
            y = onnx_ref.run(C.model(c, inp), {"x": inp["x"]})[0]
            b = C.bundle(c, inp)
            assert y.shape == b["f64"].shape and np.isfinite(b["tol"]) and b["tol"] > 0, (c.name, fam)
            assert np.abs(y.astype(np.float64) - b["f64"]).max() <= 2 * b["tol"], (c.name, fam)


def test_tolerance_tells_wrong_references_apart():
    """Each wrong edit of the float64 reference must move the output of every case it touches by at least 4 tol (`normal` inputs).  The smallest margin of
    each edit is printed (DESIGN 4.49 records them).  'res before act' touches no case: a product with residual AND activation is in NOT_REACHED."""
    margins = {e: [] for e in C.EDITS}
    for c in C.CASES:
        inp = C.case_inputs(c, "normal")
        b = C.bundle(c, inp)
        for e in C.EDITS:
            if not C.touches(c, e):
                continue
            wrong = C.ref(c, inp, "float64", edit=e)
            margins[e].append((float(np.abs(wrong - b["f64"]).max()) / b["tol"], c.name))
    for e, v in margins.items():
        if e == "res before act":
            assert not v and "res+act" in C.NOT_REACHED
            continue
        m, name = min(v)
        print(f"\n[chain] wrong edit '{e}': {len(v)} cases, smallest error / tol = {m:.3g} ({name})")
        assert m >= 4.0, (e, m, name)
    assert len(margins["k step"]) >= 40 and len(margins["last key"]) >= 9 and len(margins["ln 256"]) >= 2 and len(margins["pool div"]) >= 3


def test_poison_reaches_what_the_case_says():
    """the float64 reference of every poisoned case: non-finite outputs in sample 1 only, whole tokens; a convolution's taps, every token behind an attention"""
    for c in C.CASES:
        if not c.poison:
            continue
        inp = C.case_inputs(c, "normal")
        with np.errstate(invalid="ignore", over="ignore"):
            bad = ~np.isfinite(C.ref(c, inp, "float64", x=C.poisoned(c, inp["x"])))
        assert bad[1].any() and not bad[0].any() and not bad[2:].any() and np.array_equal(bad.all(2), bad.any(2)), c.name
        rows = set(np.flatnonzero(bad[1].any(1)).tolist())
        if any(o.kind == "attn" for o in c.ops):
            assert rows == set(range(c.T)), c.name
        else:
            t0, lo, hi = c.poison[0], 0, 0
            for o in c.ops:
                if o.kind == "conv" and o.kw > 1:                 # input token t0 reaches outputs t0 - (kw - 1 - pl) .. t0 + pl
                    lo, hi = lo - (o.kw - 1 - o.pl), hi + o.pl
            assert rows == {t for t in range(t0 + lo, t0 + hi + 1) if 0 <= t < c.T}, (c.name, sorted(rows))
