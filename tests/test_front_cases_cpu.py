"""The tables of oar_ocr_amd/synth/front_cases.py held to their own claims, without a GPU: every instantiation of the u8 stem has a case, the
fault-free emulation lies inside the float64 tolerance on every case and byte family and equals the twin's emulation bit for bit, every fault lies outside
the tolerance (or differs from the twin in bits) on at least one case, and the tolerances are f32-sized.  This is the proof that
tests/test_gpu_front_kernels.py can fail."""
import numpy as np
import pytest

from oar_ocr_amd.synth import front_cases as F

CAP = 2.0 ** -14      # the bar tests/test_gpu_f32_conv_kernels.py sets
_SEEN = {}


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _seen(name):
    """-> {family: (tol_S, fault-free err_S, equals the twin?, {fault: (err_S, equals the twin?)})} of one case, computed once"""
    if name not in _SEEN:
        c = F.case_by_name(name)
        out = {}
        for fam in F.BYTE_FAMILIES:
            inp = F.inputs(c, fam)
            b = F.bundle(c, inp)
            twin = F.emulate_twin(c, inp)
            clean = F.emulate(c, inp)
            out[fam] = (b["tol_S"], F.error(c, clean, b), _bits(clean, twin), {f: (F.error(c, y, b), _bits(y, twin)) for f in F.faults_for(c) for y in [F.emulate(c, inp, f)]})
        _SEEN[name] = out
    return _SEEN[name]


def test_every_form_has_a_case():
    have = {F.form_key(c, env) for g, env in F.GROUPS.items() for c in F.cases_of(g)}
    assert have == set(F.ALL_FORMS), (sorted(have), F.ALL_FORMS)
    assert {F.form_key(c, F.GROUPS["sw_off"]) for c in F.cases_of("sw_off")} == {"pages k3 lds", "table k3 lds"}      # the switch moves every case of its group
    assert all(F.form_key(c).endswith("sw") for c in F.cases_of("sw_off"))
    assert len({c.name for c in F.CASES}) == len(F.CASES)
    for c in F.CASES:
        assert len(F.form(c)) < 96 and len(F.twin_form(c)) < 96, c.name      # the profiler's name field


def test_the_table_holds_the_shapes_it_promises():
    page = [c for c in F.CASES if not c.table]
    assert {1, 63, 64, 65, 255, 257} <= {c.px for c in page} and any(900 <= c.px <= 1100 for c in page) and any(c.px > F.PASS_PIXELS for c in page)
    assert {16, 32, 8, 24, 3} <= {c.cout for c in page}
    assert {1, 3, 32} <= {c.n for c in page} and {1, 70} <= {c.n for c in F.CASES if c.table}
    assert {(0, 1, 2), (2, 1, 0), (1, 2, 0)} <= {c.src for c in page}
    assert {(3, 3), (1, 1), (2, 2), (3, 5), (5, 5), (6, 7)} <= {(c.kh, c.kw) for c in page}
    assert {((2, 2), (1, 1)), ((2, 1), (1, 1)), ((1, 1), (2, 2))} <= {(c.strides, c.dilations) for c in page if c.k3}
    assert any(not c.bias and not c.identity for c in page) and {"relu", "hswish"} <= {c.act for c in page}
    assert max(c.kh * c.kw * 3 for c in F.CASES) == 126
    assert any(c.n > 1 and c.px % 64 for c in page)      # dead lanes with a next image to land in
    for c in F.CASES:
        if c.table:
            assert max(c.widths) <= c.w and c.h == 8 and c.w == 40


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_fault_free_emulation_is_inside_the_tolerance_and_equals_the_twin(name):
    for fam, (tol, err, same, _) in _seen(name).items():
        print(f"\n[front] {name} | {fam} | tol_S {tol:.3g} | emulation err_S {err:.3g}")
        assert np.isfinite(tol) and tol < CAP, (name, fam, tol)
        assert err <= tol, (name, fam, err, tol)
        assert same, (name, fam, "the stem's emulation and the twin's differ in bits")


@pytest.mark.parametrize("fault", F.FAULTS)
def test_every_fault_is_caught_somewhere(fault):
    by_tol, by_bits = [], []
    for c in F.CASES:
        if fault not in F.faults_for(c):
            continue
        for fam, (tol, _, _, faults) in _seen(c.name).items():
            err, same = faults[fault]
            if err > tol:
                by_tol.append((c.name, fam))
            if not same:
                by_bits.append((c.name, fam))
    print(f"\n[front] {fault}: outside tol_S on {len(by_tol)} (case, family) pairs, e.g. {by_tol[:1]}; differs from the twin in bits on {len(by_bits)}, e.g. {by_bits[:1]}")
    assert by_tol or by_bits, (fault, "no case catches it")


def test_identity_cases_return_the_normalised_tensor():
    for c in F.CASES:
        if c.identity:
            for fam in F.BYTE_FAMILIES:
                inp = F.inputs(c, fam)
                assert _bits(F.emulate(c, inp), F.stem_tensor(c, inp)), (c.name, fam)
