"""The tables of oar_ocr_amd/synth/row_cases.py held to their own claims, without a GPU: every launch form of the f32 reduction kernels has a
case, the fault-free emulation of every kernel lies inside the tolerance on every case and input family, every fault lies outside it on at least one, the
tolerances are f32-sized, and the restated launch arithmetic agrees with the tables.  This is the proof that tests/test_gpu_row_kernels.py can fail."""
import numpy as np
import pytest

from oar_ocr_amd.synth import attention_cases as A
from oar_ocr_amd.synth import row_cases as R
from oracle import op_cases

CAP = 2.0 ** -14
# `rising` / `falling` attention: scaled scores of +-200 (attention_cases.RAMP).  A score's f32 rounding grows with its size and exp turns it into a relative
# error of the weight, so the noise of an honest f32 evaluation -- and with it 16 noise -- is RAMP / 8 times that of N(0, 1) inputs, whose scores stay below 8
CAP_RAMP = CAP * A.RAMP / 8.0
_SEEN = {}      # family -> {(case, kind): (tol, fault-free error, {fault: error})}


def _family(family):
    if family not in _SEEN:
        out = {}
        for c in R.cases_of(family):
            for kind in c.kinds:
                if kind.startswith("nan") or kind == "neginf":
                    continue
                inp = R.inputs(c, kind)
                b = R.bundle(c, inp)
                out[(c.name, kind)] = (b["tol"], R.error(c, R.emulate(c, inp), b), {f: R.error(c, R.emulate(c, inp, f), b) for f in R.FAULTS[family]})
        _SEEN[family] = out
    return _SEEN[family]


def test_names_are_unique_and_every_form_has_a_case():
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    reached = {R.form_key(c, R.GROUPS[R.group_of(c)]) for c in R.CASES}
    assert None not in reached
    unreached = [f for f in R.ALL_FORMS if f not in reached]
    print("\nforms no case reaches:", unreached)
    assert unreached == [] and reached <= set(R.ALL_FORMS), (unreached, reached - set(R.ALL_FORMS))
    for c in R.CASES:
        assert R.group_of(c) in R.GROUPS and all(isinstance(n, str) and n for n in R.form(c, R.GROUPS[R.group_of(c)])), c.name
        for n in R.form(c, R.GROUPS[R.group_of(c)]):
            assert len(n) < 96, n      # the profiler's name buffer


def test_the_tables_hold_the_shapes_the_forms_and_edges_need():
    sm = {c.C for c in R.cases_of("softmax")}
    assert {1, 2, 63, 64, 65, 1000, 1024, 1025, 1279, 1280, 4113, 16384, 16385, 18385} <= sm and {c.rows for c in R.cases_of("softmax")} == {1, 3, 4, 5, 9}
    assert max(c.rows * c.C for c in R.cases_of("softmax")) == 9 * 18385
    ln = R.cases_of("layernorm")
    assert {c.C for c in ln} == {4, 32, 124, 128, 132, 256, 260, 384, 388, 512, 516, 1020, 1024, 1, 3, 30, 65, 1028, 1500} and {c.rows for c in ln} == {1, 7, 8, 9, 17}
    assert {R.ln_nv(c.C) for c in ln if R.LN.takes_v4(c.C)} == {1, 2, 3, 4, 8}
    for form in {R.form_key(c) for c in ln}:      # every form with and without scale and bias, at both eps, and with the NaN rows
        mine = [c for c in ln if R.form_key(c) == form]
        assert {c.affine for c in mine} == {True, False} or len(mine) < 2, form
    assert {c.eps for c in ln} == {1e-5, 1e-6} and any("nan4" in c.kinds and R.LN.takes_v4(c.C) for c in ln) and any("nan5" in c.kinds and not R.LN.takes_v4(c.C) for c in ln)
    lin = [c for c in R.cases_of("gemm") if c.route == "linear"]
    assert all(c.K % 4 != 0 or c.alpha != 1.0 for c in lin), "a Linear with 4 | K and alpha = 1 runs on the implicit-GEMM kernels"
    assert {1, 63, 64, 65, 130} <= {c.M for c in lin} and {1, 3, 64, 67} <= {c.N for c in lin} and {1, 15, 16, 17, 30, 64, 67} <= {c.K for c in lin}
    assert {c.tB for c in lin} == {0, 1} and {c.bias for c in lin} == {True, False} and {c.beta for c in lin} == {1.0, 0.25} and {c.act for c in lin} == {"none", "relu"}
    assert {c.res for c in lin} == {True, False} and all(c.spelling == "matmul" and c.act == "none" for c in lin if c.res)      # (rewrite pass 4 folds an Add behind a plain Linear)
    mm = [c for c in R.cases_of("gemm") if c.route == "matmul"]
    assert {c.batch for c in mm} == {1, 3, 7} and {c.bcast for c in mm} == {"none", "A", "B"} and {b for c in mm if "nan" in c.kinds for b in (c.bcast,)} == {"none", "A", "B"}
    gap = [c for c in R.cases_of("pool") if c.op == "gap"]
    assert {4, 48, 256, 1024, 6, 1028} <= {c.C for c in gap} and {1, 5, 21, 22, 85} <= {c.H * c.W for c in gap}
    assert {R.gap_splits(c.N, c.H * c.W, c.C) for c in gap} >= {1, 2, 5} and R.gap_splits(1, 529, 48) == 2 and R.gap_splits(2, 1300, 4) == 5
    assert tuple(c.C for c in R.cases_of("pool") if c.op == "mean") == R.RED_C == op_cases.RED_C
    mx = [c for c in R.cases_of("pool") if c.op == "max"]
    assert {(c.k, c.s, c.pad) for c in mx} == {(3, 2, 1), (2, 2, 0)} and any(c.ceil for c in mx) and all("neginf" in c.kinds for c in mx)
    at = R.cases_of("attention")
    assert {c.hd for c in at} == {4, 15, 16, 20, 32, 33, 64} and {1, 2, 31, 32, 63, 64, 65, 257, 301, 385} <= {c.T for c in at}
    for c in at:
        if not R.attn_whole(c.T, c.hd):
            assert -(-c.T // R.ATTN_BLOCK) >= 3 and c.T % R.ATTN_BLOCK and {"rising", "falling"} & set(c.kinds), c.name      # three key blocks, the last ragged


def test_se_table_states_the_launch_geometry():
    se = R.cases_of("se")
    for c in se:
        assert (c.G, c.slice, c.parts) == R.se_geometry(c.N, c.C, c.R, c.C), (c.name, R.se_geometry(c.N, c.C, c.R, c.C))
        assert (c.C + c.R + c.parts * c.slice) * 4 <= 64 * 1024
    assert len({c.G for c in se}) >= 2 and len({c.slice for c in se}) >= 2 and len({c.parts for c in se}) >= 2
    assert any(c.G == 1 and c.N >= 128 for c in se) and any(c.slice > 64 for c in se) and {1, 8} <= {c.parts for c in se}
    assert any(c.R % 4 and c.R % 8 for c in se) and any(c.C > 256 and c.C % 64 for c in se)
    # the restated arithmetic at the launcher's own edges: 127 / 128 images, a slice that has to shrink below 1024
    assert R.se_geometry(127, 192, 48, 192)[0] == 2 and R.se_geometry(128, 192, 48, 192)[0] == 1 and R.se_geometry(200, 2100, 64, 2100) == (3, 704, 1)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulation_is_inside_the_tolerance_and_every_fault_outside(family):
    seen = _family(family)
    assert seen
    worst = 0.0
    for (name, kind), (tol, err, _) in seen.items():
        exact = R.exact(R.case_by_name(name))
        cap = CAP_RAMP if family == "attention" and kind in ("rising", "falling") else CAP
        assert np.isfinite(tol) and tol < cap and (tol > 0 or exact), (name, kind, tol)
        assert err <= tol, (name, kind, "the fault-free emulation", err, tol)
        worst = max(worst, err / tol if tol else 0.0)
    print(f"\n{family}: {len(seen)} (case, input family) pairs, fault-free emulation at most {worst:.3f} tol")
    assert len(R.FAULTS[family]) >= 5
    for fault in R.FAULTS[family]:
        caught = [(k, faults[fault] / tol if tol else np.inf) for k, (tol, _, faults) in seen.items() if faults[fault] > tol]
        print(f"  {fault}: caught on {len(caught)} pairs, e.g. {caught[0][0] if caught else None}")
        assert caught, (family, fault, "no case catches it")


def test_softmax_probabilities_stay_far_from_underflow():
    """the relative rule needs no carve-out: every float64 probability of every case is at least 2^-100"""
    low = min(float(R.ref(c, R.inputs(c, kind)).min()) for c in R.cases_of("softmax") for kind in c.kinds)
    print(f"\nsmallest float64 probability: 2^{np.log2(low):.1f}")
    assert low >= 2.0 ** -100


def test_poisoned_inputs_are_what_they_say():
    for c in R.CASES:
        for kind in c.kinds:
            if kind.startswith("nan"):
                key = "a" if c.family == "gemm" else "x"
                clean, bad = R.inputs(c, "normal")[key], R.inputs(c, kind)[key]
                assert np.isnan(bad).sum() == 1 and np.array_equal(clean[~np.isnan(bad)], bad[~np.isnan(bad)]), (c.name, kind)
                if c.family == "layernorm":
                    assert np.isnan(bad[int(kind[3])]).any()
            if kind == "neginf":
                y = R.ref(c, R.inputs(c, kind))
                assert np.isneginf(y[:, :, 0, 0]).all() and np.isfinite(y[:, :, 1:, :]).all() and np.isneginf(y).sum() == c.N * c.C, c.name      # the corner window alone
