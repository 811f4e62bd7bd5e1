"""oar_ocr_amd/synth/ds_cases.py on the CPU: the matrix names every compiled instantiation of the fused depthwise-separable block, the hand-kept host
tables agree with the instantiation units, the shape rules of the matrix hold, and the tolerance tells six wrong references from the right one
(DESIGN 4.48).  tests/test_gpu_dsblock_kernels.py runs the same matrix on the GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from oar_ocr_amd.synth import ds_cases as D

CSRC = Path(D.__file__).resolve().parent.parent / "csrc"
_INT = r"\s*(\d+)\s*"


def _src(name):
    return (CSRC / name).read_text()


def _tuples(text, head, n):
    """every head(i, i, ...) with n integer arguments -> tuples of int"""
    return [tuple(int(v) for v in m) for m in re.findall(head + r"\(" + ",".join([_INT] * n) + r"\)", text)]


# ------------------------------------------------------------------------------------------------ what the sources compile
RS_UNITS = {(1, 1): "dsblock_rs_k3s11.hip", (2, 1): "dsblock_rs_k3s21.hip", (1, 2): "dsblock_rs_k3s12.hip", (2, 2): "dsblock_rs_k3s22.hip"}


def rs_unit_rows():
    """the OAR_RS_CASE lines of the four units -> [(sh, sw, nch, nf, x6, waves)], in file order"""
    rows = []
    for (sh, sw), f in RS_UNITS.items():
        got = _tuples(_src(f), "OAR_RS_CASE", 7)
        assert got and all(r[:3] == (3, sh, sw) for r in got), (f, got)
        rows += [(sh, sw, nch, nf, x6, wpw) for _, _, _, nch, nf, wpw, x6 in got]
    return rows


def rs_host_table():
    line = re.search(r"static const int T\[\]\[6\] = \{(.*?)\};", _src("dsblock.hip")).group(1)
    return [tuple(int(v) for v in m) for m in re.findall(r"\{" + ",".join([_INT] * 6) + r"\}", line)]


def cs_host_table():
    body = re.search(r"constexpr CsInst kInst\[\] = \{(.*?)\};", _src("dsblock_cs.hip")).group(1)
    return [tuple(int(v) for v in m) for m in re.findall(r"\{" + ",".join([_INT] * 6) + r"\}", body)]


def cs_unit_rows():
    return _tuples(_src("dsblock_cs.hip"), "OAR_CS_CASE", 6)


def pc_unit_rows():
    line = re.search(r"#define OAR_PC_INSTANCES\(X\)(.*)", _src("dsblock_pc.hip")).group(1).split("//")[0]
    return _tuples(line, "X", 6)


def rs2_host_table():
    body = re.search(r"constexpr Rs2Inst kRs2\[\] = \{(.*?)\};", _src("dsblock_rs2.hip")).group(1)
    return [tuple(int(v) for v in m) for m in re.findall(r"\{" + ",".join([_INT] * 4) + r"\}", body)]


def rs2_unit_rows():
    """-> [(nch1, nf1, nf2, waves, regw, lag)]"""
    rows = re.findall(r"OAR_RS2_CASE\(" + ",".join([_INT] * 4) + r",\s*(true|false)\s*,\s*(true|false)\s*\)", _src("dsblock_rs2.hip"))
    return [(*(int(v) for v in r[:4]), int(r[4] == "true"), int(r[5] == "true")) for r in rows]


def wa_unit_rows():
    rows = []
    for f in ("dsblock_wa_a.hip", "dsblock_wa_b.hip"):
        got = re.findall(r"case (\d+): dsblock_wa_one<(\d+), (\d+)>\(dsblock_wa_kernel<(\d+), (\d+)>", _src(f))
        assert got and all(a == b == d and c == e for a, b, c, d, e in got), (f, got)
        rows += [(int(b), int(c)) for _, b, c, _, _ in got]
    return rows


def ds_unit_rows():
    """-> [(ks, sw, nfw, pfw)]: the layouts of OAR_DSBLOCK_INSTANTIATE x the four units that use it"""
    lay = re.findall(r"case (\d+): NAME##_one<(\d+), (\d+)>", _src("dsblock_dev.h"))
    assert lay and all(int(k) == 10 * int(a) + int(b) for k, a, b in lay), lay
    units = []
    for f in sorted(CSRC.glob("dsblock_k*s*.hip")):
        m = re.search(r"OAR_DSBLOCK_INSTANTIATE\(dsblock_launch_k(\d)s(\d), (\d), (\d)\)", f.read_text())
        assert m and m.group(1) == m.group(3) and m.group(2) == m.group(4), f.name
        units.append((int(m.group(3)), int(m.group(4))))
    assert sorted(units) == [(3, 1), (3, 2), (5, 1), (5, 2)], units
    return [(ks, sw, int(a), int(b)) for ks, sw in units for _, a, b in lay]


def ablations():
    """the timing-ablation instantiations (built only with OAR_DSB_ABLATIONS: wrong results by design)"""
    out = {f"rs_dbg<{d}>" for d in re.findall(r"dsblock_rs_kernel<3, 1, 1, 3, 3, 12, 1, 0, (\d+)>", _src("dsblock_rs_dbg.hip"))}
    out |= {f"cs_dbg<{d}>" for d in re.findall(r"OAR_CS_DBG\((\d+)\)", _src("dsblock_cs.hip"))}
    out |= {f"pc_dbg<{d}>" for d in re.findall(r"OAR_PC_DBG\((\d+)\)", _src("dsblock_pc.hip"))}
    return out


def compiled():
    out = set()
    for sh, sw, nch, nf, x6, wpw in rs_unit_rows():
        out |= {f"rs<{sh},{sw},{nch},{nf},{wpw},{a},{x6}>" for a in (0, 1)}
    for ks, sh, sw, nch, nf, rows in cs_unit_rows():
        out |= {f"cs<{ks},{sh},{sw},{nch},{nf},{rows},{a}>" for a in (0, 1)}
    for ks, sh, sw, nch, nf, rows in pc_unit_rows():
        out |= {f"pc<{ks},{sh},{sw},{nch},{nf},{rows},{a}>" for a in (0, 1)}
    for nch1, nf1, nf2, wpw, rw, lag in rs2_unit_rows():
        out |= {f"rs2<{nch1},{nf1},{nf2},{wpw},{a},{rw},{lag}>" for a in (0, 1)}
    out |= {f"wa<{nf},{P}>" for nf, P in wa_unit_rows()}
    out |= {f"ds<{ks},{sw},{nfw},{pfw}>" for ks, sw, nfw, pfw in ds_unit_rows()}
    return out | ablations()


# compiled (under a build option), and run by no case: they leave ingredients out to time the rest, their results are wrong by design
NOT_RUN = ablations()


def test_matrix_names_every_instantiation():
    planned = {D.plan(c).inst for c in D.CASES}
    built = compiled()
    assert len(built - NOT_RUN) == 148 and len(rs_unit_rows()) == 42          # a new instantiation changes these counts on purpose: add its case
    assert planned <= built, sorted(planned - built)
    assert built - planned == NOT_RUN, (sorted(built - planned - NOT_RUN), sorted(NOT_RUN - (built - planned)))
    assert all("_dbg<" in i for i in NOT_RUN)
    assert len({c.name for c in D.CASES}) == len(D.CASES)
    for c in D.CASES:
        p = D.plan(c)
        assert p.family == c.family, (c.name, p)                               # no case has drifted onto another kernel family
        assert len(p.name) < 96, p.name                                        # the native buffer
        assert p.cls == {"rs": "dsblock_rs", "rs2": "dsblock_rs", "wa": "dsblock_wa", "cs": "dsblock_cs", "pc": "dsblock_cs", "ds": "dsblock"}[c.family]
        assert p.name.startswith(("dsblock px=", "dsblock2 px="))
    assert all(D.plan(c).name.endswith(" pc") for c in D.CASES if c.family == "pc") and all(D.plan(c).name.endswith(" cs") for c in D.CASES if c.family == "cs")


def test_host_tables_agree_with_the_units():
    """a mismatch means the host sizes LDS (and counts waves) for another workgroup than the one launched"""
    assert rs_host_table() == rs_unit_rows()                                   # row for row, wave count included
    assert list(D.RS_TABLE) == rs_host_table()
    assert cs_host_table() == cs_unit_rows() and list(D.CS_INST) == cs_host_table()
    assert list(D.PC_INST) == pc_unit_rows() and set(pc_unit_rows()) <= set(cs_unit_rows())     # the producer / consumer kernel takes dsblock_cs's items: same tile rows
    lagged = [r for r in rs2_unit_rows() if r[5]]
    assert {r[:4] for r in lagged} == set(rs2_host_table()) and list(D.RS2_INST) == rs2_host_table()
    assert [r for r in rs2_unit_rows() if not r[5]] == [(2, 3, 3, 12, 0, 0)]                      # dsblock_rs2_wpw's literal 12 for the variant without lag
    assert [r for r in rs2_unit_rows() if r[4]] == [(2, 3, 3, 8, 1, 1)]                           # dsblock_rs2_regw's one shape
    assert sorted(nf for nf, _ in wa_unit_rows()) == sorted(D.WA_NF) and all(P == (1 if nf == 12 else 2) for nf, P in wa_unit_rows())
    assert {(a, b) for _, _, a, b in ds_unit_rows()} == set(D.DS_LAYOUTS)
    assert int(re.search(r"constexpr int kWaRing = (\d+);", _src("dsblock_dev.h")).group(1)) == D.WA_RING


def _fam(f):
    return [c for c in D.CASES if c.family == f]


def test_matrix_shapes():
    """the rules of the issue, computed from plan alone"""
    for c in D.CASES:
        ho, wo = c.out_hw
        assert c.in_bytes <= 60e6 and c.n >= 2, c.name
        assert c.c >= 8 and c.c % 4 == 0 and c.cout % 4 == 0, c.name               # (the graph pass fuses from 8 depthwise channels)
        if c.family == "rs2":                                                       # strips of 14: one strip, or a ragged last one
            assert c.w <= 14 or c.w % 14, c.name
            continue
        assert c.poison or "single strip" in c.name or (wo % 16 != 0 and wo > 16), c.name
        for s, v in zip(c.strides, (c.h, c.w)):
            assert s == 1 or v % 2 == 1, c.name
        if c.residual:
            assert c.acts[1] == "relu"
    # channel tails: every family has an exact multiple of 16 and a tail on both sides (cs / pc take multiples only)
    for f in ("rs", "wa", "ds"):
        assert {c.c % 16 == 0 for c in _fam(f)} == {True, False} and {c.cout % 16 == 0 for c in _fam(f)} == {True, False}, f
    assert {c.c % 16 == 0 for c in _fam("rs2")} == {True, False} and {c.c3 % 16 == 0 for c in _fam("rs2")} == {True, False}
    assert all(c.c % 16 == 0 and c.cout % 16 == 0 for c in _fam("cs") + _fam("pc"))
    # ---- row-streaming
    rs = [(c, D.plan(c)) for c in _fam("rs")]
    for u in RS_UNITS:
        mine = [(c, p) for c, p in rs if c.strides == u]
        assert {p.info["acts"] for _, p in mine} == {0, 1}
        assert any(c.pads4 == (0, 0, 1, 1) for c, _ in mine), u
        assert any(dict(c.env).get("OAR_DSB_RS_R") == "1" and p.info["R"] == 1 for c, p in mine), u
        assert any("OAR_DSB_RS_R" in dict(c.env) and p.info["R"] > 1 and c.out_hw[0] % p.info["R"] for c, p in mine), u            # a forced R with a ragged last segment
        many = [p.info for _, p in mine if p.info["items"] > p.info["waves"]]
        assert many and all(i["items"] < 2 * i["waves"] and i["items"] % i["waves"] for i in many), u                               # some waves take two items, others one
        assert any(c.out_hw[0] % p.info["R"] for c, p in mine if not c.env), u                                                      # ragged last segment under the planner's own R
    assert any(c.pads4 == (0, 0, 0, 0) and c.strides == (1, 1) and c.out_hw[0] == c.h - 2 for c, _ in rs)
    assert any(p.info["items"] < p.info["waves"] for _, p in rs)
    assert {p.info["NR"] - c.strides[0] for c, p in rs} == {1, 2}
    assert {(bool(p.info["x6"]), p.info["pwreg"]) for _, p in rs} == {(True, False), (False, True), (False, False)}                 # bf16x6; f32 fragments in registers; f32 from the LDS table
    for c, p in rs:                                                              # the per-call switch appears only where it is needed: the default rule is what runs otherwise
        if "OAR_DSB_RS_X6" in dict(c.env):
            assert D.plan(c, {}).info["x6"] != p.info["x6"], c.name
    assert any(D.plan(c).info["x6"] == 0 and _nfnch(c) >= 6 and not c.env for c, _ in rs)                                           # the flip where the table has no bf16x6 row
    # ---- two blocks
    r2 = _fam("rs2")
    assert {c.h for c in r2} >= {1, 2} and any(c.w <= 14 for c in r2) and any(c.w % 14 == 1 and c.w > 14 for c in r2)
    assert {D.plan(c).info["acts"] for c in r2} == {0, 1} and any(len(set(c.acts)) > 1 for c in r2)
    assert {tuple(sorted(c.env)) for c in r2} == {(), (("OAR_DSB_RS2_REGW", "0"),), (("OAR_DSB_RS2_VARIANT", "1"),)}
    # ---- wave-autonomous
    wa = [(c, D.plan(c)) for c in _fam("wa")]
    assert all(c.out_hw[0] % (4 * p.info["P"]) for c, p in wa)                                                                      # a ragged last tile row
    assert any(c.residual for c, _ in wa) and any(p.info["tiles"] > p.info["grid"] for _, p in wa)
    assert all((dict(c.env).get("OAR_DSBLOCK_WA") == "2") == (p.info["nf"] > 4) for c, p in wa)
    # ---- chunk-streamed, producer / consumer
    cs = [(c, D.plan(c)) for c in _fam("cs")]
    assert all(p.info["items"] % 4 for _, p in cs) and all(dict(c.env) == dict(D.ENV_CS) for c, _ in cs)
    assert any(p.info["iters"] >= 2 and (c.c, c.cout, c.k) == (96, 96, 3) for c, p in cs)
    assert all(c.out_hw[0] % p.info["rows"] for c, p in cs)
    pc = [(c, D.plan(c)) for c in _fam("pc")]
    assert all(not c.env for c, _ in pc) and {p.info["acts"] for _, p in pc} == {0, 1} and any(p.info["iters"] >= 2 for _, p in pc)
    # ---- dsblock.inc
    ds = [(c, D.plan(c)) for c in _fam("ds")]
    assert {p.info["TC"] for _, p in ds} == {16, 32, 64}
    for ks in (3, 5):
        for sw in (1, 2):
            assert {c.strides[0] for c, _ in ds if (c.k, c.strides[1]) == (ks, sw)} == {1, 2}
    assert any(c.residual for c, _ in ds) and any("swish" in c.acts for c, _ in ds) and any(p.info["tiles"] > p.info["grid"] for _, p in ds)
    # ---- poison: one case per family, never behind a Relu
    assert sorted(c.family for c in D.CASES if c.poison) == sorted(["rs", "rs2", "wa", "cs", "pc", "ds"])
    for c in D.CASES:
        if c.poison:
            assert all(a in (None, "hswish") for a in c.acts) and not c.residual, c.name      # fmaxf swallows a NaN
            assert c.poison != "tail" or c.c % 16, c.name
            at = D.poison_at(c)
            assert all(0 <= i < d for i, d in zip(at, (c.n, c.c, c.h, c.w))), (c.name, at)
    # ---- children: few, and every per-process switch is part of the group's key
    assert len(D.groups()) <= 12 and sum(len(v) for v in D.groups().values()) == len(D.CASES)


def _nfnch(c):
    return -(-c.c // 16) * -(-c.cout // 16)


def test_selection_thresholds_restated():
    """spot checks of plan against the native rules' edges (the GPU test holds the rest to what runs)"""
    mk = lambda **kw: D.Case("t", "rs", **{**dict(c=48, cout=48, k=3, n=2, h=7, w=19), **kw})
    assert D.plan(mk()).info["x6"] == 1 and D.plan(mk(c=32, cout=32)).info["x6"] == 0                          # nf nch >= 6
    assert D.plan(mk(c=32, cout=128)).info["x6"] == 0                                                         # 16 >= 6, no bf16x6 row: flipped
    assert D.plan(mk(residual=True, acts=(None, "relu"))).family == "wa"                                      # the row-streaming kernel takes no residual
    assert D.plan(mk(k=5, pads=None)).family == "ds" and D.plan(mk(k=5, c=192, cout=192)).family == "pc"
    assert D.plan(mk(k=5, c=192, cout=192), {"OAR_DSB_PC": "0"}).family == "cs"
    assert D.plan(mk(c=96, cout=96)).family == "rs" and D.plan(mk(c=96, cout=96), dict(D.ENV_CS)).family == "cs"
    assert D.plan(mk(acts=("swish", "swish"))).family == "ds"


@pytest.mark.parametrize("family", ["normal", "positive"])
def test_tolerance_tells_wrong_references_apart(family):
    """On a reduced copy of every case: fused_bundle's tol is finite and positive, and six wrong edits of the float64 reference lie outside it -- one depthwise
    tap dropped at one border pixel; the padding read as the clamped edge pixel; the pointwise bias left out of the cout fragments after the first; one
    strip's output row computed from the input one row later; (rs2) the intermediate tensor not zeroed outside the image; (bf16x6 pointwise) the mm slice
    product lost.  The smallest margin (error / tol) of each edit is printed; on `normal` every margin must be >= 4.  `positive` tells every edit apart as
    well (asserted: margin > 1), the lost mm product least: a coherent sum's f32 noise is larger while the lost product stays 2^-16 of it, so its smallest
    margin there is about 2 (printed, recorded in DESIGN 4.48) -- the >= 4 requirement rests on `normal`."""
    margins = {e: [] for e in D.EDITS}
    for full in D.CASES:
        c = D.reduced(full)
        inp = D.case_inputs(c, family)
        b = D.bundle(c, inp)
        assert np.isfinite(b["tol"]) and b["tol"] > 0, (c.name, b["tol"])
        for e in D.EDITS:
            if e == "mid" and c.family != "rs2":
                continue
            if e == "bias" and c.out_ch <= 16:
                continue
            if e == "clamp" and not D.reads_padding(c):
                continue
            if e == "x6" and not D.x6_pointwise(full):
                continue
            at = int(np.abs(b["f64"][0, :, 0, :]).max(0).argmax())     # 'tap': the first-row pixel of image 0 with the largest output (not one every Relu has zeroed)
            wrong = D.block_ref(c, inp, "float64", edit=e, at=at)
            margins[e].append((float(np.abs(wrong.astype(np.float64) - b["f64"]).max()) / b["tol"], c.name))
    for e, v in margins.items():
        m, name = min(v)
        print(f"\n[ds] {family} | wrong edit '{e}': {len(v)} cases, smallest error / tol = {m:.3g} ({name})")
        if family == "normal":
            assert m >= 4.0, (e, m, name)
        else:
            assert m > 1.0, (e, m, name)


def test_references_agree_with_the_plain_block():
    """block_ref against x6_cases.ds_ref where that one applies (stride 1, padding k // 2, one activation, no residual), and the fault-free bf16x6 emulation
    of the pointwise meets the tolerance; pow2 reproduces `normal`'s bits in the f32 reference"""
    from oar_ocr_amd.synth import x6_cases
    seen = 0
    for full in D.CASES:
        c = D.reduced(full)
        if c.family == "rs2" or c.strides != (1, 1) or c.pads is not None or c.residual or c.acts[0] != c.acts[1] or c.acts[0] == "swish":
            continue
        inp = D.case_inputs(c, "normal")
        old = x6_cases.DsCase(c.name, "", (), c.c, c.cout, c.k, c.n, c.h, c.w, c.acts[0])
        f64 = D.block_ref(c, inp, "float64")
        assert np.abs(x6_cases.ds_ref(old, inp["x"], *inp["blocks"][0], dtype="float64") - f64).max() <= 1e-12 * max(1.0, np.abs(f64).max()), c.name
        seen += 1
    assert seen >= 20
    for full in D.CASES:
        if "pow2" not in D.families_of(full) or full.in_bytes > 1e6:
            continue
        c = D.reduced(full)
        a, b = D.block_ref(c, D.case_inputs(c, "normal"), "float32"), D.block_ref(c, D.case_inputs(c, "pow2"), "float32")
        assert np.array_equal(b.view(np.uint32), np.ldexp(a, x6_cases.POW2_B).view(np.uint32)), c.name
    for full in D.CASES:
        if not D.x6_pointwise(full) or full.in_bytes > 1e6:
            continue
        c = D.reduced(full)
        inp = D.case_inputs(c, "normal")
        b = D.bundle(c, inp)
        assert np.abs(D.block_ref(c, inp, "float32", edit="x6:").astype(np.float64) - b["f64"]).max() <= b["tol"], c.name
