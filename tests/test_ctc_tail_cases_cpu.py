"""The CTC tail matrix of oar_ocr_amd/synth/ctc_tail_cases.py held to its own claims, without a GPU: the restated rule sends a case to
every route and every cross, the input families are what they say, the designed rows' stated answers are float64's, and three wrong tails -- the
soft-max over the padded width, first index wins, a merge that stops after 16 tiles -- fall outside the bounds on the cases meant to catch them."""
import numpy as np
import pytest

from oar_ocr_amd.synth import ctc_tail_cases as C
from oar_ocr_amd.synth import x6_cases as X

RANDOM = [c for c in C.CASES if c.family != "designed"]
DESIGNED = [c for c in C.CASES if c.family == "designed"]
_B = {}


def _bundle(c):
    """the case's inputs, CPU features and bounds (kept for the one case at hand)"""
    if c.name not in _B:
        _B.clear()
        crops, sel, fb, w, b = C.inputs(c)
        F = X.ctc_features(crops, sel, fb)
        _B[c.name] = (F, w, b, C.bounds(F, w, b))
    return _B[c.name]


def test_names_are_unique_and_every_case_takes_its_route():
    assert len({c.name for c in C.CASES}) == len(C.CASES)
    for c in C.CASES:
        p = c.plan()
        assert p.route == c.route, (c.name, p)
        assert not (p.must & p.must_not) and p.linear in p.must
        assert all(k in C.SWITCHES or k == "OAR_PROF_DETAIL" for k in c.envd), c.env
        # the crops need no resize: the recognizer's tensor is exactly as wide as they are, 8 columns per time step
        assert c.width % 8 == 0 and C.tensor_width([c.width] * c.crops, [48] * c.crops) == c.width, c.name


def test_every_route_and_every_cross_has_a_case():
    plans = {c.name: c.plan() for c in C.CASES}
    have = lambda pred: [c.name for c in C.CASES if pred(c, plans[c.name])]
    for r in C.ROUTES:
        assert have(lambda c, p: p.route == r and not c.env), r
        assert have(lambda c, p: p.route == r and c.family == "designed"), r
        assert have(lambda c, p: p.route == r and c.family == "negative"), r
    need = {
        "R1 at K 32, 64, 96": all(have(lambda c, p, K=K: p.route == "R1" and c.K == K) for K in (32, 64, 96)),
        "R2 at K 48, 120, 288": all(have(lambda c, p, K=K: p.route == "R2" and c.K == K and not c.env) for K in (48, 120, 288)),
        "R3 at K 120, 192": all(have(lambda c, p, K=K: p.route == "R3" and c.K == K) for K in (120, 192)),
        "R4 at K 16, 384 and K 120 without partials": all(have(lambda c, p, K=K: p.route == "R4" and c.K == K) for K in (16, 384, 120)),
        "R4 under OAR_CTC_PARTIALS=0": have(lambda c, p: p.route == "R4" and c.envd.get("OAR_CTC_PARTIALS") == "0"),
        "R5 at V 1104, 2080": all(have(lambda c, p, V=V: p.route == "R5" and c.V == V) for V in (1104, 2080)),
        "R6 at K 30, 67": all(have(lambda c, p, K=K: p.route == "R6" and c.K == K) for K in (30, 67)),
        "R7 at V 97, 1024": all(have(lambda c, p, V=V: p.route == "R7" and c.V == V) for V in (97, 1024)),
        "V 1025 is fused": have(lambda c, p: c.V == 1025 and p.route != "R7"),
        "R1 spelled Gemm": have(lambda c, p: p.route == "R1" and c.spelling == "gemm"),
        "R2 spelled Gemm": have(lambda c, p: p.route == "R2" and c.spelling == "gemm"),
        "R1's shape under OAR_CTC_HEAD_OS=0": have(lambda c, p: c.K in (32, 64, 96) and c.envd.get("OAR_CTC_HEAD_OS") == "0" and p.route == "R2"),
        "R3's shape under OAR_IGEMM_X6=0": have(lambda c, p: c.envd.get("OAR_IGEMM_X6") == "0" and p.route == "R2" and C.route(c.K, c.V, c.M).route == "R3"),
        "R1 one row past 384": have(lambda c, p: p.route == "R1" and c.M % 384 == 1),
        "the bf16x6 Linear in front of softmax_argmax": have(lambda c, p: p.route == "R4" and p.linear == "conv_igemm_ws_x6"),
    }
    for r in ("R1", "R2", "R3"):
        need[f"{r} tiles <= 16"] = have(lambda c, p: p.route == r and 0 < p.tiles <= 16) or r == "R3"      # (R3 needs 4096 passes: 33 tiles at 2000 rows)
        need[f"{r} tiles 17 .. 32"] = have(lambda c, p: p.route == r and 17 <= p.tiles <= 32) or r == "R3"
        need[f"{r} tiles > 32"] = have(lambda c, p: p.route == r and p.tiles > 32)
        need[f"{r} single valid column in the last tile"] = have(lambda c, p: p.route == r and c.V == 128 * (p.tiles - 1) + 1)
        need[f"{r} rows no multiple of 16"] = have(lambda c, p: p.route == r and c.M % 16)
    for r in ("R1", "R2", "R4", "R6"):
        need[f"{r} a single crop"] = have(lambda c, p: p.route == r and c.crops == 1 and c.T == 40)
    for v in C.SEAM_SIZES:
        need[f"OrtInfer seam at V {v}"] = have(lambda c, p: c.seam and c.V == v)
    missing = [k for k, v in need.items() if not v]
    assert not missing, missing
    # every switch has exactly one child, the detail names one more
    assert len(C.env_groups()) == 4, list(C.env_groups())


def test_rule_thresholds():
    """the restated rule at the edges the issue names"""
    assert C.partials_supported(288) and not C.partials_supported(292) and not C.partials_supported(28)
    assert C.partials_supported_x6(192) and not C.partials_supported_x6(200) and not C.partials_supported_x6(124)
    assert [C.ctc_tiles(C.pad16(v)) for v in (1100, 2049, 2065, 4097, 4113, 18385)] == [9, 17, 17, 33, 33, 144]
    assert C.route(120, 18385, 40).route == "R2" and C.route(120, 18385, 8000).route == "R3"      # the PP-OCRv5 mobile head: few rows, many rows
    assert C.route(384, 6625, 8000).route == "R4" and C.route(384, 6624, 8000).route == "R5"        # an SVTRv2 head; a dictionary of 16 n entries
    assert C.route(64, 1025, 200).route == "R1" and C.route(64, 1024, 200).route == "R7"
    assert C.route(120, 4113, 1984).route == "R2" and C.route(120, 4113, 1985).route == "R3"        # 124 x 33 = 4092 passes, 125 x 33 = 4125


@pytest.mark.parametrize("name", [c.name for c in RANDOM])
def test_random_case_is_what_it_says(name):
    c = C.case_by_name(name)
    F, w, b, B = _bundle(c)
    assert F.shape == (c.M, c.K) and w.shape == (c.K, c.V)
    assert B["clear"].mean() >= 0.9, (name, B["clear"].mean())
    assert np.isfinite(B["tol"]).all() and (B["tol"] < 2.0 ** -14).all(), (name, B["tol"].max())
    z = C.logits64(F, w, b)
    if c.family == "negative":
        assert z.max() < 0.0, (name, z.max())
    # the bf16x6 routes: the fault-free emulator lies inside the bound, a dropped correction term outside (on the rows sampled)
    if c.route in ("R1", "R3") and c.family == "normal":
        rows = np.unique(np.linspace(0, c.M - 1, 64).astype(np.int64))
        Bs = C.bounds(F[rows], w, b)
        for fault, inside in (("", True), ("no mm", False)):
            _, p = X.ctc_ref(F[rows], w, b, fault=fault)
            ok = bool((np.abs(p - Bs["p"]) <= Bs["tol"]).all())
            assert ok == inside, (name, fault or "emulator", float((np.abs(p - Bs["p"]) / Bs["tol"]).max()))


@pytest.mark.parametrize("name", [c.name for c in RANDOM if c.family == "negative"])
def test_padded_softmax_is_caught(name):
    """wrong tail 1: a missing `c < ctc_valid` mask.  On the negative family the padding wins every row of a padded head"""
    c = C.case_by_name(name)
    F, w, b, B = _bundle(c)
    idx, p = C.wrong_padded(F, w, b)
    r = C.check(B, idx, p, c.V)
    if C.pad16(c.V) != c.V:
        assert len(r["out_of_range"]) == c.M and r["ratio"] > 1.0, (name, len(r["out_of_range"]), r["ratio"])
    else:
        assert len(r["out_of_range"]) == 0 and r["ratio"] == 0.0      # (no padding: the wrong tail is the right one)


@pytest.mark.parametrize("name", [c.name for c in RANDOM if c.V > 2048])
def test_short_merge_is_caught(name):
    """wrong tail 3: a merge that drops the tiles from 16 on"""
    c = C.case_by_name(name)
    F, w, b, B = _bundle(c)
    idx, p = C.wrong_merge(F, w, b)
    r = C.check(B, idx, p, c.V)
    print(f"\n{name}: short merge {r['ratio']:.3g} tol, {len(r['bad_index'])} of {c.M} clear rows with another index")
    if c.V - 2048 > 16:
        assert r["ratio"] > 1.0, (name, r["ratio"])
    if c.V >= 4096 and c.family != "positive":      # half the columns lie past the 16th tile, and so does about half the rows' arg max (positive: one column wins nearly every row)
        assert len(r["bad_index"]) > c.M // 4, (name, len(r["bad_index"]))
    # (a single column or one fragment past the 16th tile: random rows need not notice -- the designed rows do, below)


@pytest.mark.parametrize("name", [c.name for c in DESIGNED])
def test_designed_rows(name):
    c = C.case_by_name(name)
    crops, sel, fb, rows = C.designed_rows(c)
    F = X.ctc_features(crops, sel, fb)
    kinds = {r.name.split(" ")[0] + " " + r.name.split(" ")[1] for r in rows}
    assert {"pair one", "pair across", "pair other", "pair into", "zero max", "max at", "twin columns"} <= kinds, kinds
    tiles = C.ctc_tiles(C.pad16(c.V))
    assert ("pair same" in kinds) == (tiles > 16), (name, tiles, kinds)
    caught = {"padded": False, "merge": False}
    for r in rows:
        B = C.bounds(F, r.w, r.b, r.tie)
        # the stated answer is float64's with last index wins; every row is clear of the others, or an exact tie whose later column is the answer
        assert (B["idx"] == r.answer).all() and B["clear"].all(), (name, r.name)
        z = C.logits64(F, r.w, r.b)
        if r.tie:
            assert r.answer == max(r.tie) and np.array_equal(np.asarray(r.w)[:, r.tie[0]], np.asarray(r.w)[:, r.tie[1]]) and r.b[r.tie[0]] == r.b[r.tie[1]]
            # wrong tail 2: first index wins
            idx, p = C.wrong_first(F, r.w, r.b, r.tie)
            assert len(C.check(B, idx, p, c.V)["bad_index"]) == c.M, (name, r.name)
        if not r.name.startswith("twin"):
            assert not np.asarray(r.w).any() and np.array_equal(z, np.broadcast_to(r.b.astype(np.float64), z.shape))
            if not r.name.startswith("max at"):
                assert z.max() <= 0.0
        if C.pad16(c.V) != c.V and not r.name.startswith("twin") and not r.name.startswith("max at"):
            idx, p = C.wrong_padded(F, r.w, r.b)
            chk = C.check(B, idx, p, c.V)
            assert len(chk["out_of_range"]) == c.M, (name, r.name)      # the padding (logit 0) wins or ties as the later column
            caught["padded"] = True
        if c.V > 2048 and r.answer >= 2048:
            idx, p = C.wrong_merge(F, r.w, r.b)
            chk = C.check(B, idx, p, c.V)
            assert len(chk["bad_index"]) == c.M and chk["ratio"] > 1.0, (name, r.name)
            caught["merge"] = True
    assert caught["padded"] == (C.pad16(c.V) != c.V) and caught["merge"] == (c.V > 2048), (name, caught)


def test_detail_names_and_class_check():
    c = C.case_by_name("r3 K120 V4113 detail")
    p = c.plan()
    assert C.detail_name(p, c.M, c.K) == "conv_igemm_x6 M=2025 K=120 N=4128 k1x1 s1"
    feature = "conv_igemm M=2025 K=1152 N=120 k48x8 s48 small NT=4"
    ran = {feature, "conv_igemm_x6 M=2025 K=120 N=4128 k1x1 s1", "ctc_combine", "transpose"}
    assert C.classes_ran(p, ran, c.M, c.K, detail=True) == ([], [])
    assert C.classes_ran(p, (ran - {"ctc_combine"}) | {"softmax_argmax"}, c.M, c.K, detail=True) == (["ctc_combine"], ["softmax_argmax"])
    # the feature layer cannot stand in for the head
    c4 = C.case_by_name("r4 K384 V1100 detail")
    missing, _ = C.classes_ran(c4.plan(), {"conv_igemm M=200 K=1152 N=384 k48x8 s48 small NT=4", "softmax_argmax"}, c4.M, c4.K, detail=True)
    assert missing == ["conv_igemm M=200 K=384 N=1104 k1x1 s1"]
    c1 = C.case_by_name("r1 K32 V1100 normal")
    assert C.classes_ran(c1.plan(), {"conv_igemm", "ctc_head_x6", "ctc_combine"}, c1.M, c1.K) == ([], [])
    assert C.classes_ran(c1.plan(), {"conv_igemm", "conv_igemm_ws", "ctc_combine"}, c1.M, c1.K) == (["ctc_head_x6"], ["conv_igemm_ws"])
