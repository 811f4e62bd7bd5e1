"""Every path of the sample-local chain kernel (csrc/chain.hip) against float64, held to f32 accuracy, with the path of every operator asserted.

The matrix, the Python restatement of Planner::fuse_chains and of the kernel's dispatch, and the references live in oar_ocr_amd/synth/chain_cases.py.  The
cases run in three child processes started with OAR_PROF_DETAIL=1: the default one, one with OAR_CHAIN_LDS=0 (every product on the general path) and the
control with OAR_FUSE_CHAIN=0 (operator by operator: it serves the poison check only).  Every job runs twice in its child; the child hands back the outputs,
the profiler names of every job and whether the two runs agreed byte for byte.  Per case and input family: exactly one launch of class `chain` ran, under
the detail name chain_cases.plan predicts -- one token per operator of its table -- and no attention, layernorm, pool2d, copy2d or conv_igemm launch;
max |y - f64| <= 4 max |f32 numpy - f64| over the WHOLE output.  Poison: one NaN at one token of sample 1 comes out at exactly the outputs the float64
reference gives non-finite (a convolution's taps, all tokens of an attention), every other output is the clean run's, bit for bit."""
import shutil

import numpy as np
import pytest

from oar_ocr_amd.synth import chain_cases as C
from oar_ocr_amd.synth.child_run import infer_many_in_child

pytestmark = pytest.mark.gpu
_RUNS = {}      # group -> {job key: ChildResult}: the group's child ran (once: a failed child is not started again)
_UNFUSED_ONLY = ("attention", "layernorm", "pool2d", "copy2d", "conv_igemm")


@pytest.fixture(scope="module")
def workroot(tmp_path_factory):
    root = tmp_path_factory.mktemp("chain")
    yield root
    shutil.rmtree(root, ignore_errors=True)


def _job(c, kind):
    inp = C.case_inputs(c, "normal" if kind == "poison" else kind)
    return C.model(c, inp), {"x": C.poisoned(c, inp["x"]) if kind == "poison" else inp["x"]}


def _runs(group, workroot):
    if group not in _RUNS:
        assert None not in _RUNS.values(), "an earlier child failed: no further GPU work is started by this module"
        _RUNS[group] = None
        keys = [(c.name, kind) for c in C.CASES for kind in C.jobs_of(c, group)]
        gen = (_job(C.case_by_name(name), kind) for name, kind in keys)
        # the time limit, sized to the group: the child's start, then an engine and two runs per job (a workgroup per sample, T <= 137 but for one case)
        res = infer_many_in_child(gen, {"OAR_PROF_DETAIL": "1", **dict(C.GROUPS[group])}, workroot / group, timeout=60.0 + 1.0 * len(keys))
        _RUNS[group] = dict(zip(keys, res))
    assert _RUNS[group] is not None, f"the child of the group {group} failed in an earlier test"
    return _RUNS[group]


def _check_ran(c, p, res):
    ran = sorted(n for n in res.names if n.startswith("chain"))
    if c.overflow:      # the planner sends tensors back to the arena: the same launch holds a general-path product and an LDS one
        assert len(ran) == 1, (c.name, sorted(res.names))
        toks = ran[0].split()[3:]
        assert any(t.startswith("gh") for t in toks) and any(t[:2] in ("gs", "g1", "g2", "g3") for t in toks), (c.name, ran)
    else:
        assert ran == [p.name], (c.name, p.name, sorted(res.names))
    assert not any(n.startswith(_UNFUSED_ONLY) for n in res.names), (c.name, sorted(res.names))
    assert res.same, (c.name, "two runs of the same input differ")


def _output(c, res):
    got = res.outputs()[0]
    assert got.dtype == np.float32 and got.shape == (c.n, c.T, C.widths(c)[len(c.ops) - 1]), (c.name, got.shape)
    return got


def _check_poison(c, got, clean, tag):
    inp = C.case_inputs(c, "normal")
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~np.isfinite(C.ref(c, inp, "float64", x=C.poisoned(c, inp["x"])))
    assert bad[1].any() and not bad[0].any() and not bad[2:].any(), (c.name, tag)          # inside its sample
    assert np.array_equal(bad.all(2), bad.any(2)), (c.name, tag)                             # whole tokens
    spread, lost = ~np.isfinite(got) & ~bad, np.isfinite(got) & bad
    assert not spread.any() and not lost.any(), (c.name, tag, int(spread.sum()), int(lost.sum()), np.argwhere(spread)[:8].tolist(), np.argwhere(lost)[:8].tolist())
    assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32)), (c.name, tag, "an output outside the poisoned tokens' reach changed")


def _check_group(c, group, workroot):
    runs = _runs(group, workroot)
    p = C.plan(c, C.GROUPS[group])
    clean = None
    for kind in C.jobs_of(c, group):
        res = runs[(c.name, kind)]
        _check_ran(c, p, res)
        got = _output(c, res)
        if kind == "poison":
            _check_poison(c, got, clean, group)
            continue
        assert np.isfinite(got).all(), (c.name, kind)
        b = C.bundle(c, C.case_inputs(c, kind))
        assert np.isfinite(b["tol"]) and b["tol"] > 0, (c.name, kind, b["tol"])
        err = float(np.abs(got.astype(np.float64) - b["f64"]).max())
        print(f"\n[chain] {c.name} | {group} | {p.name} | {kind} | scale {b['scale']:.3g} tol {b['tol']:.3g} err {err:.3g} | err / tol {err / b['tol']:.3f}")
        assert err <= b["tol"], (c.name, group, kind, err, b["tol"])
        if kind == "normal":
            clean = got
    for key, res in runs.items():     # the case passed: its outputs are not needed again (a failed case keeps them for a look)
        if key[0] == c.name:
            res.discard()


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_chain_paths(name, workroot):
    _check_group(C.case_by_name(name), "default", workroot)


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.hbm_too])
def test_chain_general_path(name, workroot):
    """OAR_CHAIN_LDS=0: every tensor of the run in the arena, every product on ch_gemm_slow, LayerNorm and attention reading and writing HBM"""
    _check_group(C.case_by_name(name), "hbm", workroot)


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.poison])
def test_poison_expectation_holds_operator_by_operator(name, workroot):
    """the control (OAR_FUSE_CHAIN=0): no chain launch, and the poisoned run differs from the clean one exactly where the float64 reference is non-finite --
    the poison assertions above state a property of the operation, not of the fused kernel"""
    c = C.case_by_name(name)
    runs = _runs("unfused", workroot)
    for kind in ("normal", "poison"):
        assert not any(n.startswith("chain") for n in runs[(name, kind)].names) and runs[(name, kind)].same, (name, kind, sorted(runs[(name, kind)].names))
    _check_poison(c, _output(c, runs[(name, "poison")]), _output(c, runs[(name, "normal")]), "unfused")
    for kind in ("normal", "poison"):
        runs[(name, kind)].discard()
