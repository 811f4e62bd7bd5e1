"""oar_ocr_amd/synth/f32_cases.py on the CPU: the matrix names every compiled f32 convolution variant, its tolerance is sane, and the tolerance tells
three wrong references from the right one.  tests/test_gpu_f32_conv_kernels.py runs the same matrix on the GPU."""
import numpy as np
import pytest

from oar_ocr_amd.synth import f32_cases as C

# Every instantiation the f32 convolution sources compile (igemm.hip, igemm_ws.inc, igemm_ws3.hip, kernels.hip), as f32_cases.plan names them.  A new
# template argument or kernel must be added here, and gets a case or a line in NOT_RUN.
IGEMM = ([f"tile<{nt},{pf},{kk}>" for nt in (1, 2, 3, 4) for pf in (1, 2, 4) for kk in ("1x1", "kxk")] +
         [f"small<{nt},{kk}>" for nt in (1, 2, 3, 4) for kk in ("1x1", "kxk", "1x1 SE")] +
         [f"ws_{kk}<{nt},{pf}>" for kk in ("1x1", "gen") for nt, pf in ((8, 1), (6, 1), (4, 2), (3, 2), (2, 2), (1, 2))] +
         ["ws3<1,2>", "ws3<2,2>"])
DW = ([f"dw_tiled<{k},{sh},{sw},{th}>" for k in (3, 5) for sh in (1, 2) for sw in (1, 2) for th in (1, 2)] +
      [f"dw_tiled<5,{sh},{sw},{th},gap>" for sh in (1, 2) for sw in (1, 2) for th in (1, 2)] + ["dw_generic"])
DIRECT = ["smallcin", "direct", "convt_direct"]
# compiled, and run by no case: a two-row depthwise tile needs 262144 threads, which at stride 2 x 2 is 134 MB of input
NOT_RUN = {"dw_tiled<3,2,2,2>", "dw_tiled<5,2,2,2>", "dw_tiled<5,2,2,2,gap>"}


def _plan(c):
    return C.plan(c, C.KIND_ENV.get(c.kind, {}))


def test_matrix_names_every_instantiation():
    ran = {_plan(c).inst.replace(" lds96", "") for c in C.CASES}
    listed = set(IGEMM + DW + DIRECT)
    assert ran <= listed, sorted(ran - listed)
    assert listed - ran == NOT_RUN, (sorted(listed - ran - NOT_RUN), sorted(NOT_RUN - (listed - ran)))
    assert any(_plan(c).inst.endswith("lds96") for c in C.CASES)                 # the 96 KB opt-in of the tiled depthwise kernel
    assert all(_plan(c).f32 for c in C.CASES)                                      # no case has drifted onto a bf16x6 kernel
    assert len({c.name for c in C.CASES}) == len(C.CASES) and {c.kind for c in C.CASES} == set(C.KINDS)


def test_matrix_shapes():
    """what the matrix promises about its shapes: weight-stationary cases cross tile boundaries, pixel counts are no multiple of a tile, sizes stay small"""
    for c in C.CASES:
        assert c.n * c.cin * c.h * c.w * 4 <= 100e6 and c.M * c.cout * 4 <= 120e6, c.name
        if c.kind.startswith(("ws_", "ws3", "tile")):
            assert c.M % 16 != 0, c.name
    # every weight-stationary instantiation, on its own: cases with >= 3 wave tiles per wave of the busiest workgroup at KC % 3 = 0, 1 and 2 (the stage rotation at a
    # tile boundary is compiled per instantiation) and with a zero-padded K tail; the 1x1 kernels at all five K of the issue
    ws = [c for c in C.CASES if c.kind.startswith(("ws_1x1", "ws_gen"))]
    per = {}
    for c in ws:
        if C.ws_tiles_per_wave(c) >= 3.0 and not c.residual and not c.concat:
            per.setdefault(_plan(c).inst, []).append(c)
    assert set(per) == {f"ws_{kk}<{nt},{pf}>" for kk in ("1x1", "gen") for nt, pf in ((8, 1), (6, 1), (4, 2), (3, 2), (2, 2), (1, 2))}, sorted(per)
    for inst, cs in per.items():
        ks = {c.kh * c.kw * c.cin for c in cs}
        assert {-(-k // 16) % 3 for k in ks} == {0, 1, 2}, (inst, sorted(ks))
        assert any(k % 16 for k in ks), (inst, sorted(ks))
        if inst.startswith("ws_1x1"):
            assert {32, 48, 64, 40, 80} <= ks, (inst, sorted(ks))
    assert any(c.kind.startswith("ws_1x1") and C.ws_tiles_per_wave(c) < 1.0 for c in C.CASES)     # ... and a launch where some waves get no tile
    assert all(c.h * c.w % 16 != 0 for c in ws if c.kind.startswith("ws_gen") and c.n > 1)           # a pixel fragment straddles two images
    # one HardSwish case per kind of epilogue: the implicit-GEMM kernels' (ws, ws3, tile, small), the depthwise kernel's and each direct kernel's own
    hs = {_plan(c).inst.split("<")[0] for c in C.CASES if c.act == "hswish"}
    assert {"ws_1x1", "ws_gen", "ws3", "tile", "small", "dw_tiled", "smallcin", "direct", "convt_direct"} <= hs, sorted(hs)


def test_expected_variant_is_the_plans_suffix():
    for c in C.CASES:
        p = _plan(c)
        assert C.expected_variant(c, C.KIND_ENV.get(c.kind, {})) == p.variant
        assert all(len(n) < 96 for n in p.names), p.names                          # the native buffer
        if p.variant:
            assert p.names[0].endswith(" " + p.variant), p.names


def _largest_product(c, x, w):
    """(index of the middle output pixel's first channel, the largest of the products that sum to it)"""
    ho, wo = c.out_hw
    row = (c.n - 1) * ho * wo + (ho // 2) * wo + wo // 2
    T, wsel, chan, co = C.gemm_view(c, x, w, np.array([row]), cols=1)
    terms = [float(T[0, tap, chan(ci)[0]]) * float(wsel(tap, ci)[0]) for tap in range(c.kh * c.kw) for ci in range(c.cin // c.group)]
    return (c.n - 1, 0, ho // 2, wo // 2), max(terms, key=abs)


@pytest.mark.parametrize("family", C.FAMILIES)
def test_tolerance_tells_wrong_references_apart(family):
    """On a reduced copy of every case (one or two small images, the same node): tol_S is finite, positive where anything is rounded, and under 2^-14; and
    three wrong edits of the float64 reference lie outside it -- one product removed from one output, the padding read as the clamped edge pixel instead of
    zero, the bias left out of the cout fragments after the first.  The smallest margin (error / tol_S) of each edit is printed."""
    margins = {"product": [], "clamp": [], "bias": []}
    for full in C.CASES:
        c = C.reduced(full)
        i = C.case_inputs(c, family)
        b = C.bundle(c, i["x"], i["w"], i["b"], i["r"])
        assert np.isfinite(b["tol_S"]) and 0 <= b["tol_S"] < 2.0 ** -14, (c.name, b["tol_S"])
        assert C.err_S(b["f64"], b["f64"], b["S"]) == 0.0
        at, term = _largest_product(c, i["x"], i["w"])
        wrong = b["f64"].copy()
        wrong[at] -= term
        e = C.err_S(wrong, b["f64"], b["S"])
        assert e > b["tol_S"], (c.name, "product", e, b["tol_S"])
        margins["product"].append((e / max(b["tol_S"], 2.0 ** -30), c.name))
        if any(c.pads) and not c.transpose:
            e = C.err_S(C.conv_ref(c, i["x"], i["w"], i["b"], "float64", i["r"], edit="clamp"), b["f64"], b["S"])
            assert e > b["tol_S"], (c.name, "clamp", e, b["tol_S"])
            margins["clamp"].append((e / max(b["tol_S"], 2.0 ** -30), c.name))
        if c.bias and c.cout > 16:
            e = C.err_S(C.conv_ref(c, i["x"], i["w"], i["b"], "float64", i["r"], edit="bias"), b["f64"], b["S"])
            assert e > b["tol_S"], (c.name, "bias", e, b["tol_S"])
            margins["bias"].append((e / max(b["tol_S"], 2.0 ** -30), c.name))
    for k, v in margins.items():
        m, name = min(v)
        print(f"\n[f32] {family} | wrong edit '{k}': {len(v)} cases, smallest error / tol_S = 2^{np.log2(m):.1f} ({name})")
        assert m > 1.0


def test_references_agree_with_the_plain_convolution():
    """conv_ref against an independent evaluation: x6_cases.conv_ref (numpy, per-tap matrix products) where that one applies (stride 1, padding k // 2),
    and the sample chain against the float64 reference everywhere -- transposed, grouped, dilated, strided and asymmetric cases included"""
    from oar_ocr_amd.synth import x6_cases
    for full in C.CASES:
        c = C.reduced(full)
        i = C.case_inputs(c, "normal")
        f64 = C.conv_ref(c, i["x"], i["w"], i["b"], "float64", i["r"])
        rows = C.sample_rows(c)
        chain, co = C.f32_chain(c, i["x"], i["w"], i["b"], i["r"], rows)
        assert np.abs(chain - C.pick(c, f64, rows, co)).max() <= 1e-4 * max(1.0, np.abs(f64).max()), c.name     # (the chain is an independent im2col: a wrong tap or group would be off by O(1))
        if not c.transpose and c.kh == c.kw and c.strides == (1, 1) and c.dilations == (1, 1) and c.pads == (c.kh // 2,) * 4 and not c.residual and c.bias:
            ref = x6_cases.conv_ref(C.gated(c, i["x"]), i["w"], i["b"], c.group, "float64")
            assert np.abs(ref - f64).max() <= 1e-12 * max(1.0, np.abs(f64).max()), c.name
