"""The references, input families and layouts that tests/test_gpu_flash_attention_kernels.py runs the two flash-attention kernels against (synth/attention_cases.py;
DESIGN 4.37), checked without a GPU:
  * mha_core is torch's einsum + softmax in f64, relpos_core is the core of vit_reference._attention (identity projection, so the block's output minus
    its residual IS the attention);
  * the inputs can tell a wrong key loop from the right one: flash_emulate is the kernels' loop in f32 numpy (32-key blocks, running maximum and sum);
    without a fault it is within tol of f64 on every family, and each fault moves the output by more than 100 tol (or makes it non-finite) on the family
    built for it;
  * the entry points' argument checks, which come in front of the device query and so answer here as they do on the GPU."""
import numpy as np
import pytest

from oar_ocr_amd import api, build
from oar_ocr_amd.synth import attention_cases as ac
from oar_ocr_amd.synth import vit_reference

#          N  Tq  Tk nh  dh
SHAPES = [(1, 5, 33, 1, 8), (2, 70, 97, 3, 20), (1, 64, 65, 2, 48), (1, 17, 64, 1, 64), (2, 65, 32, 2, 36), (1, 3, 31, 1, 4)]
IDS = ["N%d_Tq%d_Tk%d_nh%d_dh%d" % s for s in SHAPES]

_cache = {}


def _case(shape, family, pre):
    """inputs and the reference bundle: computed once, never modified"""
    key = (shape, family, pre)
    if key not in _cache:
        q, k, v = ac.mha_inputs(family, *shape, seed=5)
        _cache[key] = (q, k, v, ac.reference_bundle(ac.mha_core, q, k, v, ac.scale_of(shape[4]), pre))
    return _cache[key]


def _emulate(shape, q, k, v, pre, layout, fault=None):
    N, Tq, Tk, nh, dh = shape
    L = ac.mha_layout(layout, q, k, v)
    return ac.flash_emulate(L["buf"], L["q_off"], L["k_off"], L["v_off"], L["ldq"], L["ldk"], L["ldv"], N, Tq, Tk, nh, dh, ac.scale_of(dh), pre, fault)


def _err(o, ref):
    return float(np.abs(o.astype(np.float64) - ref["f64"]).max()) if np.isfinite(o).all() else float("inf")


@pytest.mark.parametrize("shape,family,pre", [((2, 7, 37, 3, 12), "normal", False), ((1, 9, 70, 2, 20), "rising", True)], ids=["normal_post", "rising_pre"])
def test_mha_core_is_torch_einsum_and_softmax(shape, family, pre):
    import torch
    q, k, v = ac.mha_inputs(family, *shape, seed=1)
    tq, tk, tv = (torch.from_numpy(a).double() for a in (q, k, v))
    c = torch.tensor(ac.scale_of(shape[4])).double()
    s = torch.einsum("nthd,nshd->nhts", tq * c, tk) if pre else torch.einsum("nthd,nshd->nhts", tq, tk) * c
    want = torch.einsum("nhts,nshd->nthd", torch.softmax(s, -1), tv).reshape(shape[0], shape[1], -1).numpy()
    got = ac.mha_core(q, k, v, ac.scale_of(shape[4]), pre)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.abs(got - want).max() < 1e-13
    assert ac.mha_core(q, k, v, ac.scale_of(shape[4]), pre, dtype="float32").dtype == np.float32


@pytest.mark.parametrize("B,H,W,nh,dh,ws,scale", [(2, 5, 7, 2, 12, 4, "pre"), (1, 3, 6, 3, 8, 0, "post")], ids=["windows_padded_on_both_axes", "global"])
def test_relpos_core_is_the_core_of_the_vit_reference(B, H, W, nh, dh, ws, scale):
    """vit_reference._attention with ln1 = (1, 0) and an identity output projection: its result minus x is the attention of qkv = LN(x) Wqkv^T + bqkv,
    padding tokens entering as bqkv (the graph pads zeros in front of the Linear)"""
    import torch
    rng = np.random.default_rng(7)
    C = nh * dh
    gh, gw = (ws, ws) if ws else (H, W)
    x = rng.standard_normal((B, H * W, C))
    w = {"ln1_g": np.ones(C), "ln1_b": np.zeros(C), "wqkv": rng.standard_normal((3 * C, C)) / np.sqrt(C), "bqkv": rng.standard_normal(3 * C),
         "rh": rng.standard_normal((gh, gh, dh)) / np.sqrt(dh), "rw": rng.standard_normal((gw, gw, dh)) / np.sqrt(dh), "wp": np.eye(C), "bp": np.zeros(C)}
    t = {k: torch.from_numpy(v) for k, v in w.items()}
    with torch.no_grad():
        want = (vit_reference._attention(t, "", torch.from_numpy(x), H, W, nh, ws, scale) - torch.from_numpy(x)).numpy().reshape(B * H * W, C)
    y = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + 1e-5)
    qkv = (y @ w["wqkv"].T + w["bqkv"]).reshape(B * H * W, 3, nh, dh)
    # the reference's tables are [query, key, component], the kernel's [query, component, key]
    got = ac.relpos_core(qkv, w["rh"].transpose(0, 2, 1), w["rw"].transpose(0, 2, 1), w["bqkv"], B, H, W, ws, nh, dh, ac.scale_of(dh), scale == "pre")
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-12
    if ws:                                  # the padding keys matter: without their k / v rows the result is another one
        other = ac.relpos_core(qkv, w["rh"].transpose(0, 2, 1), w["rw"].transpose(0, 2, 1), None, B, H, W, ws, nh, dh, ac.scale_of(dh), scale == "pre")
        assert np.abs(other - want).max() > 1e-3


def test_layouts_hold_the_same_views_and_the_padded_gaps_are_nan():
    shape = (2, 6, 6, 2, 12)
    q, k, v = ac.mha_inputs("normal", *shape, seed=2)
    N, T, _, nh, dh = shape
    D = nh * dh
    for layout in ac.LAYOUTS:
        L = ac.mha_layout(layout, q, k, v)
        buf, seen = L["buf"], np.zeros(L["buf"].size, bool)
        assert buf.dtype == np.float32 and buf.ndim == 1
        for a, off, ld in ((q, L["q_off"], L["ldq"]), (k, L["k_off"], L["ldk"]), (v, L["v_off"], L["ldv"])):
            assert off % 4 == 0 and ld % 4 == 0 and ld >= D and off + (N * T - 1) * ld + D <= buf.size
            at = off + np.arange(N * T)[:, None] * ld + np.arange(D)[None, :]
            assert not seen[at].any(), layout              # the views do not overlap
            seen[at] = True
            assert np.array_equal(buf[at], a.reshape(N * T, D)), layout
        if layout == "padded":
            assert (L["ldq"], L["ldk"], L["ldv"]) == (D + 4, D + 8, D + 12) and min(L["q_off"], L["k_off"], L["v_off"]) > 0
            assert (~seen).sum() > 0 and np.isnan(buf[~seen]).all() and np.isfinite(buf[seen]).all()
        else:
            assert seen.all()


@pytest.mark.parametrize("pre", [False, True], ids=["post", "pre"])
@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_right_loop_is_within_tol_on_every_family(shape, family, pre):
    if family in ("rising", "falling") and shape[2] < 64:
        shape = shape[:2] + (shape[2] + 64,) + shape[3:]          # these two families need at least two full blocks
    q, k, v, ref = _case(shape, family, pre)
    outs = [_emulate(shape, q, k, v, pre, layout) for layout in ("dense", "padded")]
    err = _err(outs[0], ref)
    print(f"{shape} {family} {'pre' if pre else 'post'}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    assert outs[0].tobytes() == outs[1].tobytes()                 # the loop's arithmetic does not depend on addresses
    assert err <= ref["tol"], (err, ref["tol"])
    if family == "equal":                                          # the mean of v over exactly Tk keys
        N, Tq, Tk, nh, dh = shape
        mean = v.astype(np.float64).mean(1).reshape(N, 1, nh * dh)
        assert np.abs(ref["f64"] - mean).max() < 1e-12


#           fault                    family     N  Tq  Tk nh  dh   layout
FAULT_CASES = [("no tail mask", "normal", (1, 5, 33, 1, 8), "dense"),
               ("no tail mask", "equal", (1, 5, 33, 1, 8), "dense"),
               ("no tail mask", "normal", (2, 70, 97, 3, 20), "dense"),
               ("no tail mask", "equal", (1, 3, 31, 1, 4), "dense"),
               ("sum not rescaled", "normal", (2, 70, 97, 3, 20), "dense"),
               ("sum not rescaled", "normal", (1, 64, 65, 2, 48), "dense"),
               ("maximum frozen", "rising", (1, 17, 64, 1, 64), "dense"),
               ("maximum frozen", "rising", (2, 70, 97, 3, 20), "dense"),
               ("row stride ignored", "normal", (1, 5, 33, 1, 8), "padded"),
               ("row stride ignored", "normal", (2, 65, 32, 2, 36), "padded"),
               ("image stride ignored", "normal", (2, 65, 32, 2, 36), "padded"),
               ("image stride ignored", "equal", (2, 70, 97, 3, 20), "padded")]


@pytest.mark.parametrize("pre", [False, True], ids=["post", "pre"])
@pytest.mark.parametrize("fault,family,shape,layout", FAULT_CASES, ids=["%s-%s-N%d_Tq%d_Tk%d_nh%d_dh%d-%s" % ((f, fam) + s + (lay,)) for f, fam, s, lay in FAULT_CASES])
def test_each_fault_shows_on_the_family_built_for_it(fault, family, shape, layout, pre):
    q, k, v, ref = _case(shape, family, pre)
    good, bad = _err(_emulate(shape, q, k, v, pre, layout), ref), _err(_emulate(shape, q, k, v, pre, layout, fault), ref)
    print(f"{fault} | {family} {shape} {layout} {'pre' if pre else 'post'}: tol {ref['tol']:.2e} right loop {good / ref['tol']:.3f} tol, faulted {bad / ref['tol']:.3g} tol")
    assert good <= ref["tol"]
    assert bad > 100 * ref["tol"], (bad, ref["tol"])


def test_every_fault_has_a_case():
    assert {f for f, *_ in FAULT_CASES} == set(ac.FAULTS)


def test_a_frozen_maximum_is_invisible_on_normal_inputs():
    """why `rising` exists: soft-max is shift-invariant until expf overflows, so on O(1) logits the frozen maximum computes the same thing"""
    shape = (2, 70, 97, 3, 20)
    q, k, v, ref = _case(shape, "normal", False)
    assert _err(_emulate(shape, q, k, v, False, "dense", "maximum frozen"), ref) <= ref["tol"]


# ------------------------------------------------------------------------------------------------ the entry points' argument checks (no launch, no device)
@pytest.fixture(scope="module")
def L():
    build.build_lib()
    return api.lib()


def _mha_code(L, **kw):
    a = dict(buf_floats=3 * 40, q_off=0, k_off=40, v_off=80, ldq=8, ldk=8, ldv=8, n=1, tq=5, tk=5, heads=2, head_dim=4, o_floats=40, o_off=0, buf=True, o=True)
    a.update(kw)
    buf, o = np.zeros(max(a["buf_floats"], 1), np.float32), np.zeros(max(a["o_floats"], 1), np.float32)
    return L.oar_k_mha_attention(api._p(buf) if a["buf"] else None, a["buf_floats"], a["q_off"], a["k_off"], a["v_off"], a["ldq"], a["ldk"], a["ldv"], a["n"], a["tq"],
                                 a["tk"], a["heads"], a["head_dim"], 0.5, 0, api._p(o) if a["o"] else None, a["o_floats"], a["o_off"])


def test_mha_entry_point_rejects_bad_arguments_in_front_of_the_device(L):
    ok = (api.OAR_OK,) if api.device_count() > 0 else (api.OAR_DEVICE,)
    assert _mha_code(L) in ok                                              # the base call is a good one: only the device can be missing
    assert _mha_code(L, buf_floats=3 * 40 + 8, q_off=8, k_off=48, v_off=88) in ok
    bad = api.OAR_INVALID_INPUT
    assert _mha_code(L, buf=False) == bad and _mha_code(L, o=False) == bad
    for dh in (6, 68, 0, -4):
        assert _mha_code(L, head_dim=dh) == api.OAR_UNSUPPORTED_OP, dh
    for name in ("n", "tq", "tk", "heads"):
        assert _mha_code(L, **{name: 0}) == api.OAR_UNSUPPORTED_OP, name
    for name in ("q_off", "k_off", "v_off", "o_off"):
        assert _mha_code(L, **{name: 2}) == bad, name                       # an offset that is no multiple of 4 floats
    for name in ("ldq", "ldk", "ldv"):
        assert _mha_code(L, **{name: 4}) == bad and _mha_code(L, **{name: 10}) == bad and _mha_code(L, **{name: -8}) == bad, name
    assert _mha_code(L, v_off=84) == bad                                    # the v view ends 4 floats past the buffer
    assert _mha_code(L, buf_floats=119) == bad and _mha_code(L, ldv=12) == bad and _mha_code(L, q_off=2 ** 63) == bad
    assert _mha_code(L, q_off=2 ** 64 - 4) == bad                           # off + need would wrap
    assert _mha_code(L, tk=6) == bad and _mha_code(L, n=2) == bad           # more rows than the buffer holds
    assert _mha_code(L, o_floats=39) == bad and _mha_code(L, o_off=4) == bad and _mha_code(L, o_floats=44, o_off=8) == bad
    assert _mha_code(L, o_floats=44, o_off=4) in ok
    with pytest.raises(api.OCRError) as e:
        api.k_mha_attention(np.zeros(120, np.float32), 0, 40, 84, 8, 8, 8, 1, 5, 5, 2, 4, 0.5, False, np.zeros(40, np.float32), 0)
    assert e.value.code == bad and "does not fit" in str(e.value)


def test_relpos_entry_point_rejects_bad_arguments_in_front_of_the_device(L):
    ok = (api.OAR_OK,) if api.device_count() > 0 else (api.OAR_DEVICE,)

    def code(B=1, H=3, W=5, ws=0, nh=2, dh=4, rh=True, rw=True, qkv=True, o=True, o_floats=None, o_off=0, bias=True):
        gh, gw = (ws, ws) if ws > 0 else (H, W)
        z = lambda n: np.zeros(max(int(n), 1), np.float32)
        a_qkv, a_rh, a_rw, a_b = z(B * H * W * 3 * nh * max(dh, 1)), z(gh * max(dh, 1) * gh), z(gw * max(dh, 1) * gw), z(3 * nh * max(dh, 1))
        o_floats = B * H * W * nh * dh if o_floats is None else o_floats
        out = z(o_floats)
        p = lambda a, on: api._p(a) if on else None
        return L.oar_k_relpos_attention(p(a_qkv, qkv), B, H, W, ws, nh, dh, p(a_rh, rh), p(a_rw, rw), p(a_b, bias), 0.5, 1, p(out, o), o_floats, o_off)
    assert code() in ok and code(bias=False) in ok and code(ws=4) in ok and code(ws=64, dh=4, nh=1) in ok
    bad = api.OAR_INVALID_INPUT
    assert code(rh=False) == bad and code(rw=False) == bad and code(qkv=False) == bad and code(o=False) == bad
    for kw in (dict(dh=6), dict(dh=68), dict(ws=65), dict(H=65, W=3), dict(H=3, W=65), dict(ws=-1), dict(B=0)):
        assert code(**kw) == api.OAR_UNSUPPORTED_OP, kw
    assert code(o_off=2) == bad and code(o_floats=119) == bad and code(o_off=4) == bad and code(o_floats=128, o_off=12) == bad
    assert code(o_floats=128, o_off=8) in ok
    with pytest.raises(ValueError):
        api.k_relpos_attention(np.zeros(10, np.float32), 1, 3, 5, 0, 2, 4, np.zeros(36, np.float32), np.zeros(100, np.float32), None, 0.5, True, np.zeros(120, np.float32), 0)
    with pytest.raises(api.OCRError) as e:
        api.k_relpos_attention(np.zeros(360, np.float32), 1, 3, 5, 0, 2, 4, None, np.zeros(100, np.float32), None, 0.5, True, np.zeros(120, np.float32), 0)
    assert e.value.code == bad
