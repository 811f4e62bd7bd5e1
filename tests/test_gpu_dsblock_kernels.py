"""Every compiled instantiation of the fused depthwise-separable block against float64, held to f32 accuracy, with the instantiation that ran asserted
(DESIGN 4.48).

The matrix, the Python restatement of the host-side selection and the references live in oar_ocr_amd/synth/ds_cases.py.  All cases that share one set of
switches run in ONE child process started with OAR_PROF_DETAIL=1 plus those switches, every job twice; the child hands back the outputs, the profiler
names of every job and whether the two runs agreed byte for byte.  Per case and input family: the one dsblock name that ran is the detail name
ds_cases.plan predicts -- family, shape plan and instantiation -- and no convolution ran (the block did not fall back; a pair ran as one launch);
max |y - f64| <= 4 max |f32 numpy - f64| over the WHOLE output; pow2 reproduces `normal` bit for bit (scaling by powers of two is exact in the float64
reference and in the tolerance too, so those bits meet pow2's own bound).  Poison: one NaN in the input comes out at exactly the outputs -- all
channels -- of the pixels whose window holds it, every other output is the clean run's, bit for bit."""
import shutil

import numpy as np
import pytest

from oar_ocr_amd.synth import ds_cases as D
from oar_ocr_amd.synth import x6_cases
from oar_ocr_amd.synth.child_run import infer_many_in_child

pytestmark = pytest.mark.gpu
_RUNS = {}      # env tuple -> {job key: ChildResult}: the group's child ran (once: a failed child is not started again)


@pytest.fixture(scope="module")
def workroot(tmp_path_factory):
    root = tmp_path_factory.mktemp("dsblock")
    yield root
    shutil.rmtree(root, ignore_errors=True)


def _feed(inp, x=None):
    f = {"x": inp["x"] if x is None else x}
    if inp["r"] is not None:
        f["r"] = inp["r"]
    return f


def _jobs(c):
    """-> (key, model, feed) of one case: its input families, and the poisoned `normal` input"""
    for fam in D.families_of(c):
        inp = D.case_inputs(c, fam)
        yield (c.name, fam), D.model(c, inp), _feed(inp)
    if c.poison:
        inp = D.case_inputs(c, "normal")
        yield (c.name, "poison"), D.model(c, inp), _feed(inp, D.poisoned(c, inp["x"]))


def _runs(env, workroot):
    env = tuple(sorted(env))
    if env not in _RUNS:
        assert None not in _RUNS.values(), "an earlier child failed: no further GPU work is started by this module"
        _RUNS[env] = None
        cases = D.groups()[env]
        keys = []

        def gen():
            for c in cases:
                for key, m, feed in _jobs(c):
                    keys.append(key)
                    yield m, feed

        jobs = sum(len(D.families_of(c)) + bool(c.poison) for c in cases)
        mb = sum(c.in_bytes * (len(D.families_of(c)) + bool(c.poison)) for c in cases) / 1e6
        # the time limit, sized to the group: the child's start, an engine and two runs per job, and the files the inputs and outputs travel through
        res = infer_many_in_child(gen(), {"OAR_PROF_DETAIL": "1", **dict(env)}, workroot / f"g{len(_RUNS)}", timeout=90.0 + 1.5 * jobs + 0.5 * mb)
        _RUNS[env] = dict(zip(keys, res))
    assert _RUNS[env] is not None, f"the child of the group {env} failed in an earlier test"
    return _RUNS[env]


def _lg(v, scale):
    return f"2^{np.log2(v / scale):.1f}" if v > 0 else "0"


def _check_ran(c, p, res):
    ran = sorted(n for n in res.names if n.startswith("dsblock"))
    assert ran == [p.name], (c.name, p.name, sorted(res.names))                 # the predicted instantiation, and nothing else of the block's (rs2: the pair as one launch)
    assert not any(n.startswith("conv") for n in res.names), (c.name, sorted(res.names))     # no fall-back to the two convolutions
    assert res.same, (c.name, "two runs of the same input differ")


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_dsblock_instantiation(name, workroot):
    c = D.case_by_name(name)
    runs = _runs(c.env, workroot)
    p = D.plan(c)
    clean = None
    for fam in D.families_of(c):
        res = runs[(name, fam)]
        _check_ran(c, p, res)
        got = res.outputs()[0]
        assert got.shape == (c.n, c.out_ch, *c.out_hw) and got.dtype == np.float32 and np.isfinite(got).all(), (name, fam, got.shape)
        if fam == "pow2":
            assert np.array_equal(got.view(np.uint32), np.ldexp(clean, x6_cases.POW2_B).view(np.uint32)), (name, "pow2 does not reproduce normal's bits")
            print(f"\n[ds] {name} | {p.name} | pow2 | the bits of normal")
            continue
        inp = D.case_inputs(c, fam)
        b = D.bundle(c, inp)
        assert np.isfinite(b["tol"]) and b["tol"] > 0, (name, fam, b["tol"])
        err = float(np.abs(got.astype(np.float64) - b["f64"]).max())
        print(f"\n[ds] {name} | {p.name} | {fam} | noise {_lg(b['noise'], b['scale'])} | tol {_lg(b['tol'], b['scale'])} | err {_lg(err, b['scale'])}"
              f"  (of the output scale {b['scale']:.3g}; err / tol {err / b['tol']:.3f})")
        assert err <= b["tol"], (name, fam, err, b["tol"])
        if fam == "normal":
            clean = got
    if c.poison:
        res = runs[(name, "poison")]
        _check_ran(c, p, res)
        got = res.outputs()[0]
        inp = D.case_inputs(c, "normal")
        with np.errstate(invalid="ignore"):
            bad = ~np.isfinite(D.block_ref(c, inp, "float64", x=D.poisoned(c, inp["x"])))
        assert bad.any() and not bad.all() and np.array_equal(bad.all(1), bad.any(1))          # all output channels of the pixels whose window holds the element
        spread, lost = ~np.isfinite(got) & ~bad, np.isfinite(got) & bad
        assert not spread.any() and not lost.any(), (name, "poison", int(spread.sum()), int(lost.sum()), np.argwhere(spread)[:8].tolist(), np.argwhere(lost)[:8].tolist())
        assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32)), (name, "poison: an output outside the element's windows changed")
    for key, res in runs.items():     # the case passed: its outputs are not needed again (a failed case keeps them for a look)
        if key[0] == name:
            res.discard()
