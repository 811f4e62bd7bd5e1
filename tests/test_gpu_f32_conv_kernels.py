"""Every compiled variant of the f32 convolution kernels against float64, held to f32 accuracy, with the variant that ran asserted.

The matrix, the Python restatement of the selection rules and the references live in oar_ocr_amd/synth/f32_cases.py.  All cases of one kernel family run
in ONE child process started with OAR_PROF_DETAIL=1 (the switch is read once per process), every case twice; the child hands back the outputs, the
profiler names of every job and whether the two runs agreed byte for byte.  Per case and input family: the detail name that ran is the one
f32_cases.plan predicts; max |y - f64| / S <= tol_S over the WHOLE output (S = the operation on absolute values, tol_S = 4 noise_S from the case's own
sample); a HardSwish layer is compared in front of its activation.  Poison: three NaNs in the input come out at exactly the outputs whose receptive field
holds one, every other output is the clean run's, bit for bit."""
import shutil
from dataclasses import replace

import numpy as np
import pytest

from oar_ocr_amd.synth import f32_cases as C
from oar_ocr_amd.synth import x6_cases
from oar_ocr_amd.synth.child_run import infer_many_in_child

pytestmark = pytest.mark.gpu
_RUNS = {}      # kind -> {job key: ChildResult}: the kind's child ran (once: a failed child is not started again)


@pytest.fixture(scope="module")
def workroot(tmp_path_factory):
    root = tmp_path_factory.mktemp("f32_conv")
    yield root
    shutil.rmtree(root, ignore_errors=True)     # (gigabytes of outputs: not left to the three-session retention of the tmp factory)


def _feed(i, x=None):
    f = {"x": i["x"] if x is None else x}
    if i["r"] is not None:
        f["r"] = i["r"]
    return f


def _jobs(c):
    """-> (key, model, feed) of one case: both families (a HardSwish layer also without its activation), the poisoned input, the Concat placements"""
    lin = None if c.act == "hswish" else "case"
    for fam in C.FAMILIES:
        i = C.case_inputs(c, fam)
        yield (c.name, fam), C.model(c, i["w"], i["b"]), _feed(i)
        if c.act == "hswish":
            yield (c.name, fam, "linear"), C.model(c, i["w"], i["b"], act=None), _feed(i)
    i = C.case_inputs(c, "normal")
    if c.poison:
        yield (c.name, "poison"), C.model(c, i["w"], i["b"], act=lin), _feed(i, C.poisoned(c, i["x"]))
    if c.concat:
        s = C.sibling_of(c)
        si = C.case_inputs(s, "normal", seed=1)
        yield (c.name, "sibling"), C.model(s, si["w"], si["b"]), {"x": i["x"]}
        for first in (False, True):
            yield (c.name, "concat", first), C.model(c, i["w"], i["b"], sibling=(s, si["w"], si["b"], first)), {"x": i["x"]}


def _runs(kind, workroot):
    if kind not in _RUNS:
        assert None not in _RUNS.values(), "an earlier child failed: no further GPU work is started by this module"
        _RUNS[kind] = None
        keys = []

        def gen():
            for c in C.cases_of(kind):
                for key, m, feed in _jobs(c):
                    keys.append(key)
                    yield m, feed

        res = infer_many_in_child(gen(), {"OAR_PROF_DETAIL": "1", **C.KIND_ENV.get(kind, {})}, workroot / kind, timeout=500.0)
        _RUNS[kind] = dict(zip(keys, res))
    assert _RUNS[kind] is not None, f"the child of kind {kind} failed in an earlier test"
    return _RUNS[kind]


def _lg(v):
    return f"2^{np.log2(v):.1f}" if v > 0 else "0"


def _check_names(c, res, env):
    p = C.plan(c, env)
    assert p.f32, (c.name, p)
    assert set(p.names) <= res.names, (c.name, p.names, sorted(n for n in res.names if n.startswith("conv")))
    if c.se:
        assert C.se_fused(c, env) and not any(n.startswith("binary") for n in res.names), sorted(res.names)     # the gate rode on the convolution: no Mul launch
    return p


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_f32_conv_variant(name, workroot):
    c = C.case_by_name(name)
    env = C.KIND_ENV.get(c.kind, {})
    runs = _runs(c.kind, workroot)
    clean = None
    for fam in C.FAMILIES:
        i = C.case_inputs(c, fam)
        b = C.bundle(c, i["x"], i["w"], i["b"], i["r"])
        assert np.isfinite(b["tol_S"]) and b["tol_S"] < 2.0 ** -14, (name, fam, b["tol_S"])
        res = runs[(name, fam)]
        p = _check_names(c, res, env)
        assert res.same, (name, fam, "two runs of the same input differ")
        outs = res.outputs()
        got = outs[0]
        assert got.shape == b["f64"].shape and np.isfinite(got).all(), (name, fam, got.shape)
        if c.act == "hswish":
            # in front of the activation the bound is defined; behind it: HardSwish has slope <= 1.5 and its own three f32 roundings, each <= 2^-24 |y| <= 2^-24 S
            lin = runs[(name, fam, "linear")]
            _check_names(c, lin, env)
            assert lin.same
            act, got = got, lin.outputs()[0]
            e_act = C.err_S(act, C.act_ref(b["f64"], "hswish"), b["S"])
            assert e_act <= 1.5 * b["tol_S"] + 2.0 ** -22, (name, fam, "behind HardSwish", e_act, b["tol_S"])
        f64 = C.act_ref(b["f64"], "relu") if c.act == "relu" else b["f64"]
        err = C.err_S(got, f64, b["S"])
        print(f"\n[f32] {name} | {p.inst} | {fam} | noise_S {_lg(b['noise_S'])} (chain {_lg(b['noise_chain'])}, torch {_lg(b['noise_torch'])}) | tol_S {_lg(b['tol_S'])} | err_S {_lg(err)}")
        assert err <= b["tol_S"], (name, fam, err, b["tol_S"])
        if fam == "normal":
            clean = got
        if c.gap:
            _check_gap(c, b, outs, f64)
    i = C.case_inputs(c, "normal")
    if c.poison:
        _check_poison(c, i, runs[(name, "poison")], clean, env)
    if c.concat:
        s = C.sibling_of(c)
        own = runs[(name, "sibling")].outputs()[0]
        for first in (False, True):
            both = runs[(name, "concat", first)]
            _check_names(c, both, env)
            y = both.outputs()[0]
            a, z = (y[:, s.cout:], y[:, :s.cout]) if first else (y[:, :c.cout], y[:, c.cout:])
            assert np.array_equal(a.view(np.uint32), clean.view(np.uint32)) and np.array_equal(z.view(np.uint32), own.view(np.uint32)), (name, "concat", first)
    for key, res in runs.items():     # the case passed: its outputs are not needed again (a failed case keeps them for a look)
        if key[0] == name:
            res.discard()


def _check_poison(c, i, res, clean, env):
    _check_names(c, res, env)
    assert res.same
    got = res.outputs()[0]
    with np.errstate(invalid="ignore"):
        bad = np.isnan(C.conv_ref(c, C.poisoned(c, i["x"]), i["w"], i["b"], "float64", i["r"]))
    assert bad.any() and not bad.all()
    spread, lost = np.isnan(got) & ~bad, ~np.isnan(got) & bad
    assert not spread.any() and not lost.any(), (c.name, "poison", int(spread.sum()), int(lost.sum()), np.argwhere(spread)[:8].tolist(), np.argwhere(lost)[:8].tolist())
    assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32)), (c.name, "poison: an output outside the receptive fields changed")


def _check_gap(c, b, outs, f64):
    """the pooled branch.  'mean': [n, c, 1, 1] means of the layer's output -- against the float64 mean of the float64 layer, within tol_S mean(S) (every
    summand's own bound) plus 4 x the larger error of two honest f32 sums of the GPU's own values (in order; numpy's pairwise).  'gate': the layer times
    the gate, which is 1, 0.5 or 0.25 by channel: exact."""
    y = outs[0]
    if c.gap == "gate":
        gate = x6_cases.se_gate(replace(c, cin=c.cout))[4]
        assert np.array_equal((y * gate[None, :, None, None]).view(np.uint32), outs[1].view(np.uint32)), c.name
        return
    pooled = outs[1].reshape(c.n, c.cout).astype(np.float64)
    flat = y.reshape(c.n, c.cout, -1)
    exact = flat.astype(np.float64).mean(-1)
    in_order = np.cumsum(flat, axis=-1, dtype=np.float32)[..., -1] / np.float32(flat.shape[-1])
    pairwise = flat.mean(-1, dtype=np.float32)
    scale = np.abs(f64).reshape(c.n, c.cout, -1).mean(-1)
    scale = np.where(scale > 0, scale, 1.0)
    noise = max(float((np.abs(in_order - exact) / scale).max()), float((np.abs(pairwise - exact) / scale).max()))
    bound = b["tol_S"] * b["S"].reshape(c.n, c.cout, -1).mean(-1) + 4.0 * noise * scale
    err = np.abs(pooled - f64.reshape(c.n, c.cout, -1).mean(-1))
    print(f"\n[f32] {c.name} | pooled | sum noise {_lg(noise)} | err / mean|y| {_lg(float((err / scale).max()))} | err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (c.name, "pooled", float((err / bound).max()))
