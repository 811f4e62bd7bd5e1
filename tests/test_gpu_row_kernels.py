"""The engine's f32 reduction kernels (csrc/kernels.hip: soft-max, LayerNorm, gemm_batched, the pools, se_fc, the SVTR attention) against float64, held to
f32 accuracy, with the launch form that ran asserted.

The tables, the Python restatement of every launcher's selection rule and the references live in oar_ocr_amd/synth/row_cases.py.  Every case is a one- or
two-node graph through api.OrtInfer; the cases of one family run in ONE child process started with OAR_PROF_DETAIL=1 (the attention cases that reach the f32
kernels only with OAR_ATTN_X6=0 in a second one), every job twice; the child hands back the outputs, the profiler names of every job and whether the two
runs agreed byte for byte.  Per case and input family: the detail name row_cases.form predicts ran and no other launch of the family's classes did; the two
runs are byte-identical; the output is finite and within tol of float64 over the WHOLE output (tol = max(16 noise, 2^-19), soft-max relative per element;
gemm: S-normalised, tol_S = 4 noise_S; MaxPool: bit for bit).  A NaN in one row of a LayerNorm or of a MatMul's left operand comes out in exactly the rows
the float64 reference gives NaN, every other output is the clean run's bit for bit; a MaxPool window of nothing but -inf gives -inf."""
import shutil

import numpy as np
import pytest

from oar_ocr_amd.synth import row_cases as R
from oar_ocr_amd.synth.child_run import infer_many_in_child

pytestmark = pytest.mark.gpu
_RUNS = {}      # group -> {job key: ChildResult}: the group's child ran (once: a failed child is not started again)


@pytest.fixture(scope="module")
def workroot(tmp_path_factory):
    root = tmp_path_factory.mktemp("row_kernels")
    yield root
    shutil.rmtree(root, ignore_errors=True)


def _runs(group, workroot):
    if group not in _RUNS:
        assert None not in _RUNS.values(), "an earlier child failed: no further GPU work is started by this module"
        _RUNS[group] = None
        keys = []

        def gen():
            for c in R.CASES:
                if R.group_of(c) == group:
                    for key, m, feed in R.jobs(c):
                        keys.append(key)
                        yield m, feed

        # the time limit: the child's start and the library load, then an engine and two runs of a tiny graph per job (about a hundred per group)
        res = infer_many_in_child(gen(), {"OAR_PROF_DETAIL": "1", **R.GROUPS[group]}, workroot / group, timeout=240.0)
        _RUNS[group] = dict(zip(keys, res))
    assert _RUNS[group] is not None, f"the child of the group {group} failed in an earlier test"
    return _RUNS[group]


def _lg(v):
    return f"2^{np.log2(v):.1f}" if v > 0 else "0"


def _check_ran(c, kind, res, env):
    want = set(R.form(c, env))
    mine = {n for n in res.names if any(n == cls or n.startswith(cls + " ") for cls in R.CLASS_OF[c.family])}
    assert want <= res.names and mine == want, (c.name, kind, "predicted", sorted(want), "ran", sorted(mine), sorted(res.names))
    assert res.same, (c.name, kind, "two runs of the same input differ")


def _check_poison(c, kind, got, clean):
    """NaN rows: exactly where float64 has them, everything else the clean run's bits"""
    with np.errstate(invalid="ignore"):
        bad = np.isnan(R.ref(c, R.inputs(c, kind)))
    assert bad.any() and not bad.all() and got.shape == bad.shape, (c.name, kind)
    rows = bad.reshape(-1, bad.shape[-1])
    assert np.array_equal(rows.all(1), rows.any(1)), (c.name, kind)      # whole rows
    spread, lost = np.isnan(got) & ~bad, ~np.isnan(got) & bad
    assert not spread.any() and not lost.any(), (c.name, kind, int(spread.sum()), int(lost.sum()), np.argwhere(spread)[:8].tolist(), np.argwhere(lost)[:8].tolist())
    assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32)), (c.name, kind, "a row without a NaN changed")


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_row_kernel(name, workroot):
    c = R.case_by_name(name)
    group = R.group_of(c)
    env = R.GROUPS[group]
    runs = _runs(group, workroot)
    clean = None
    for kind in c.kinds:
        res = runs[(name, kind)]
        _check_ran(c, kind, res, env)
        got = res.outputs()[0]
        assert got.dtype == np.float32
        if kind.startswith("nan"):
            _check_poison(c, kind, got, clean)
            continue
        inp = R.inputs(c, kind)
        b = R.bundle(c, inp)
        assert got.shape == b["f64"].shape, (name, kind, got.shape, b["f64"].shape)
        err = R.error(c, got, b)
        form = " + ".join(R.form(c, env))
        print(f"\n[row] {c.family} | {name} {kind} | {form} | noise {_lg(b['noise'])} | tol {_lg(b['tol'])} | err {_lg(err)} | err/tol {err / b['tol'] if b['tol'] else err:.3f}")
        if kind == "neginf":      # finding 2: a window of nothing but -inf is -inf, not -FLT_MAX
            assert np.isneginf(got[:, :, 0, 0]).all() and np.isfinite(got[:, :, 1:, :]).all(), (name, got[0, 0, 0, 0])
        else:
            assert np.isfinite(got).all(), (name, kind)
        assert np.isfinite(b["tol"]) and err <= b["tol"], (name, kind, err, b["tol"])
        if kind == "normal":
            clean = got
    for key, res in runs.items():     # the case passed: its outputs are not needed again (a failed case keeps them for a look)
        if key[0] == name:
            res.discard()
