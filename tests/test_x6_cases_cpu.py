"""oar_ocr_amd/synth/x6_cases.py on the CPU: the split and the emulator are what they claim, and the cases of tests/test_gpu_x6_accuracy.py discriminate --
the tolerance each GPU case applies (tol_S = 4 max(noise_S, emu_S) of its sample) lies at least four times under the error of every emulated fault ON THE
`cancel` FAMILY ONLY; on the other families it does not, as measured below.

Reading of "every case catches every fault": a GPU case runs every input family against its own tol_S, so a broken kernel fails the case as soon as ONE
family catches it.  Measured, that family is `cancel` for every case and every fault (8.6 tol_S or more): its honest partial sums are 1e-3 of S, so both
f32 orders sit near 2^-27 S while a lost slice product costs 2^-20 S.  The signed and the coherent families (normal, positive, dense) carry f32 noise of
2^-17 ... 2^-22 S at these K, which hides a lost l-plane product (0.1 ... 2 tol_S, printed below) -- they catch mh / hm / hh and check what `cancel`
does not: coherent growth, full mantissas, the exponent range.  The test asserts the margin on `cancel` and prints the whole table."""
import functools

import numpy as np
import pytest

from oar_ocr_amd.synth import x6_cases as C

IDS = [c.name for c in C.GPU_CASES]


@functools.lru_cache(maxsize=None)
def _sample(name, family):
    case = C.case_by_name(name)
    x, w, b = C.case_inputs(case, family)
    return C.sample_bundle(case, C.gated(case, x), w, b)


def _err_S(out, sb, rows=slice(None)):
    return float((np.abs(out.astype(np.float64) - sb["f64"][rows]) / sb["S"][rows]).max())


def test_split_is_exact_and_every_slice_is_bf16():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096), rng.uniform(1, 2, 4096), np.ldexp(rng.standard_normal(4096), rng.integers(-60, 60, 4096)),
                        [0.0, -0.0, 1.0, -1.0, 3.0e38, 1.0e-30, np.float32(1) + np.float32(2 ** -23), np.float32(2) - np.float32(2 ** -23)]]).astype(np.float32)
    h, m, l = C.split3(x)
    assert np.array_equal((h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)).astype(np.float32), x)
    assert np.array_equal((h + m) + l, x)                                   # exact in f32 as well: the pieces do not overlap
    for s in (h, m, l):
        assert not (s.view(np.uint32) & np.uint32(0xFFFF)).any()             # bf16: the low 16 bits are zero
    assert np.array_equal(h.view(np.uint32), x.view(np.uint32) & np.uint32(0xFFFF0000))
    # what the device function does to a non-finite value: the inputs the poison cases feed
    for v in (np.inf, -np.inf, np.nan):
        hv, mv, lv = C.split3(np.array([v], np.float32))
        assert np.isnan(mv[0]) and not np.isfinite(hv[0])


def test_fault_list_is_the_documented_one():
    assert C.CLASSES == ("mm", "lh", "hl", "mh", "hm", "hh") and C.DROPPED == ("ml", "lm", "ll")
    assert len(C.FAULTS) == 11 and len(set(C.FAULTS)) == 11                  # six classes left out, x l, w l, m / l swapped, round to nearest, one class twice
    assert set(C.FAULTS) >= {f"no {c}" for c in C.CLASSES}
    with pytest.raises(AssertionError):
        C.x6_matmul(np.ones((1, 32), np.float32), np.ones((32, 1), np.float32), fault="no such fault")


def test_nine_products_are_the_exact_product():
    """all nine classes of one 32-deep chunk, from a zero accumulator: the f32 rounding of the exact sum -- the emulator drops nothing but ml, lm, ll"""
    rng = np.random.default_rng(1)
    X, W = rng.standard_normal((8, 32)).astype(np.float32), rng.standard_normal((32, 8)).astype(np.float32)
    xs, ws = [a.astype(np.float64) for a in C.split3(X)], [a.astype(np.float64) for a in C.split3(W)]
    exact = sum(x @ w for x in xs for w in ws)
    assert np.abs(exact - X.astype(np.float64) @ W.astype(np.float64)).max() <= 2.0 ** -44
    six = C.x6_matmul(X, W).astype(np.float64)
    assert 0 < np.abs(six - exact).max() <= 2.0 ** -16


@pytest.mark.parametrize("order", ["chunk", "class", "chunk, bias last"])
def test_pow2_inputs_give_the_scaled_bits(order):
    case = C.case_by_name("os_x6 3x3 40->64 K tail")                         # K = 360: the zero-padded tail chunk as well
    a, b = _sample(case.name, "normal"), _sample(case.name, "pow2")
    assert np.array_equal(b["X"], np.ldexp(a["X"], C.POW2_X)) and np.array_equal(b["W"], np.ldexp(a["W"], C.POW2_W)) and np.array_equal(b["b"], np.ldexp(a["b"], C.POW2_B))
    for fault in (None, "no mm", "round to nearest"):
        u = C.x6_matmul(a["X"][:64], a["W"], a["b"], order=order, fault=fault)
        s = C.x6_matmul(b["X"][:64], b["W"], b["b"], order=order, fault=fault)
        assert np.array_equal(s.view(np.uint32), np.ldexp(u, C.POW2_B).view(np.uint32)), (order, fault)


def test_families_are_what_they_say():
    case = C.case_by_name("ws_x6 K96 pf1")
    x, w, b = C.case_inputs(case, "dense")
    for a in (x, w):
        assert ((a.view(np.uint32) & np.uint32(0xFFFF)) >= 0x8000).all() and (a > 0).all()
    x, w, b = C.case_inputs(case, "cancel")
    sb = _sample(case.name, "cancel")
    ratio = np.abs(sb["f64"]) / sb["S"]
    assert 1e-5 < np.median(ratio) < 1e-2, np.median(ratio)                   # the output is about 1e-3 of S
    x0, x1 = x[:, 0::2], x[:, 1::2]
    assert np.array_equal(x0.view(np.uint32) >> 8, x1.view(np.uint32) >> 8) and (x0 != x1).mean() > 0.9   # neighbours differ in the low 8 bits only
    for kind in C.POISONS:
        xp, _, _ = C.poison_inputs(case, kind)
        bad = ~np.isfinite(xp)
        assert bad.sum() == 1 and bad[C.poison_at(case)]
        assert np.array_equal(xp[~bad], C.case_inputs(case, "normal")[0][~bad])


@pytest.mark.parametrize("name", IDS)
def test_every_case_tells_every_fault_from_the_right_arithmetic(name):
    case = C.case_by_name(name)
    print()
    caught = {}
    for family in C.FAMILIES:
        sb = _sample(name, family)
        X, W, b = sb["X"][:64], sb["W"], sb["b"]
        rows = slice(0, 64)
        right = C.x6_matmul(X, W, b, order=case.order)
        nine = C.x6_matmul(X, W, b, order=case.order, extra=C.DROPPED)
        moved = float((np.abs(nine.astype(np.float64) - right.astype(np.float64)) / sb["S"][rows]).max())
        print(f"{name} / {family}: K {case.K} noise_S 2^{np.log2(sb['noise_S']):.1f} emu_S 2^{np.log2(sb['emu_S']):.1f} tol_S 2^{np.log2(sb['tol_S']):.1f}"
              f"  ml+lm+ll move {moved / sb['tol_S']:.2f} tol_S")
        assert moved < sb["tol_S"], (family, moved, sb["tol_S"])            # the classes left out by design stay inside the tolerance
        assert _err_S(right, sb, rows) <= sb["tol_S"] / 4 + 1e-30            # (the definition of tol_S, on the first 64 rows of the sample)
        faults = C.FAULTS if family == "cancel" else ("no mm", "no mh", "round to nearest")   # the table's columns for the other families
        line = []
        for fault in faults:
            e = _err_S(C.x6_matmul(X, W, b, order=case.order, fault=fault), sb, rows)
            line.append(f"{fault} {e / sb['tol_S']:.1f}")
            if e >= 4 * sb["tol_S"]:
                caught.setdefault(fault, []).append(family)
            if family == "cancel":
                assert e >= 4 * sb["tol_S"], (fault, e, sb["tol_S"])
        print("    fault errors in tol_S: " + ", ".join(line))
    assert set(caught) == set(C.FAULTS)
    assert all(len(caught[f]) == len(C.FAMILIES) for f in ("no mh",)), caught   # a lost m x h product is 2^-9 S: every family sees it


def test_breaking_the_emulator_fails_the_definition():
    """the fault-free path with mm left out is not within tol_S / 4 of f64 on `cancel` any more: the assertion above that pins emu_S notices a broken emulator"""
    sb = _sample("ws_x6 K96 pf1", "cancel")
    broken = C.x6_matmul(sb["X"][:64], sb["W"], sb["b"], fault="no mm")
    assert _err_S(broken, sb, slice(0, 64)) > sb["tol_S"]


@pytest.mark.parametrize("case", C.DS_CASES, ids=[c.name for c in C.DS_CASES])
def test_fused_dsblock_tolerance_catches_a_lost_mm_product(case):
    """the fused kernels' tolerance is 4 max |f32 - f64| (absolute); the pointwise product -- their last one -- emulated with mm left out misses it on
    every family, the fault-free emulator meets it, and pow2 gives the scaled bits"""
    outs = {}
    for family in C.FUSED_FAMILIES:
        inp = C.ds_inputs(case, family)
        b = C.fused_bundle(lambda dt: C.ds_ref(case, *inp, dtype=dt))
        outs[family] = right = C.ds_ref(case, *inp, dtype="float32", fault="")
        e_right = float(np.abs(right.astype(np.float64) - b["f64"]).max())
        e_fault = float(np.abs(C.ds_ref(case, *inp, dtype="float32", fault="no mm").astype(np.float64) - b["f64"]).max())
        print(f"\n{case.name} / {family}: noise 2^{np.log2(b['noise'] / b['scale']):.1f} of the output scale, emulator {e_right / b['tol']:.2f} tol, mm left out {e_fault / b['tol']:.2f} tol")
        assert e_right <= b["tol"] < e_fault, (family, e_right, e_fault, b["tol"])
    assert np.array_equal(outs["pow2"].view(np.uint32), np.ldexp(outs["normal"], C.POW2_B).view(np.uint32))


@pytest.mark.parametrize("case", C.ATTN_CASES, ids=[c[0] for c in C.ATTN_CASES])
def test_attention_tolerance_against_a_lost_mm_product(case):
    """attention_x6's last product is P V over T keys: emulated on the f32 probabilities with mm left out, against the bound of the GPU test: the
    fault-free product meets it, the faulty one misses it."""
    name, dim, heads, n, T = case
    hd = dim // heads
    for family in ("normal", "positive"):
        x, w, bq = C.attn_inputs(dim, heads, n, T, family)
        b = C.fused_bundle(lambda dt: C.attn_ref(x, w, bq, heads, dt))
        p = (x.astype(np.float64) @ w.astype(np.float64) + bq).reshape(n, T, 3, heads, hd).transpose(2, 0, 3, 1, 4)
        s = (p[0] * float(np.float32(hd ** -0.5))) @ p[1].transpose(0, 1, 3, 2)
        e = np.exp(s - s.max(-1, keepdims=True))
        P, V = (e / e.sum(-1, keepdims=True)).astype(np.float32), p[2].astype(np.float32)
        worst = 0.0
        for i in range(n):
            for h in range(heads):
                exact = P[i, h].astype(np.float64) @ V[i, h].astype(np.float64)
                worst = max(worst, float(np.abs(C.x6_matmul(P[i, h], V[i, h], fault="no mm").astype(np.float64) - exact).max()))
                assert np.abs(C.x6_matmul(P[i, h], V[i, h]).astype(np.float64) - exact).max() <= b["tol"]
        print(f"\n{name} / {family}: noise 2^{np.log2(b['noise'] / b['scale']):.1f} of the output scale, P V with mm left out {worst / b['tol']:.2f} tol")
        assert worst > b["tol"], (family, worst, b["tol"])


@pytest.mark.parametrize("case", C.CTC_CASES, ids=[c[0] for c in C.CTC_CASES])
def test_ctc_head_tolerance_against_a_lost_mm_product(case):
    """ctc_head_x6's product is the Linear K -> V in front of the soft-max; the GPU test bounds the arg max's probability by 4 max |f32 - f64|.  With mm left
    out the emulated head misses that bound on `normal` (asserted); on `positive` -- 1100 nearly equal probabilities of 1.6e-3 -- the ratio is printed and
    recorded in DESIGN 4.38 as measured (0.7 ... 1.1: not discriminating at this shape)."""
    name, K, V = case
    for family in ("normal", "positive"):
        crops, sel, fb, w, b = C.ctc_inputs(K, V, family)
        F = C.ctc_features(crops, sel, fb)
        i64, p64 = C.ctc_ref(F, w, b, "float64")
        _, p32 = C.ctc_ref(F, w, b, "float32")
        tol = 4.0 * float(np.abs(p32 - p64).max())
        e_right = float(np.abs(C.ctc_ref(F, w, b, fault="")[1] - p64).max())
        e_fault = float(np.abs(C.ctc_ref(F, w, b, fault="no mm")[1] - p64).max())
        print(f"\n{name} / {family}: largest probability {p64.min():.3g} ... {p64.max():.3g}, emulator {e_right / tol:.2f} tol, mm left out {e_fault / tol:.2f} tol")
        assert e_right <= tol
        if family == "normal":
            assert e_fault > tol, (e_fault, tol)
