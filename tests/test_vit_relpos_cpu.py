"""ViT encoder attention with the decomposed relative-position bias, host side: the exported spelling of synth.models.build_vit_block /
build_vary_vit through the ONNX oracles against the torch f64 reference written from the formulas (synth/vit_reference.py), inputs that tell the wrong
readings of the block from the right one, the builders' default bytes, and the kernel's resources.

Tolerance, as elsewhere in the project: noise = max |torch f32 - f64|, tol = max(16 noise, 2^-19)."""
import hashlib
import re
import subprocess

import numpy as np
import pytest

from oar_ocr_amd import build
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.vit_reference import VARIANTS, reference_bundle, vary_vit_reference, vit_block_reference

#          B   H   W nh  dh  ws          (the shapes of tests/test_gpu_vit_relpos.py)
SHAPES = [(1, 5, 7, 2, 8, 0),          # global; H != W
          (2, 9, 15, 1, 64, 0),        # 135 tokens, B = 2, full head size
          (1, 10, 13, 3, 16, 7),       # padded on both axes, 4 windows
          (1, 8, 8, 2, 16, 4),         # aligned windows, no pad
          (1, 16, 16, 1, 64, 14),      # the -L window: N = 196, pad 16 -> 28
          (1, 48, 48, 1, 64, 0)]       # the -L token count, 2304 keys, one head
IDS = ["B%d_H%d_W%d_nh%d_dh%d_ws%d" % s for s in SHAPES]

_cache = {}


def _case(shape, scale="pre"):
    """model, info, input, reference bundle: computed once, never modified"""
    if (shape, scale) not in _cache:
        B, H, W, nh, dh, ws = shape
        model, info = models.build_vit_block(H, W, nh * dh, nh, ws, seed=3, scale=scale)
        x = np.random.default_rng(11).standard_normal((B, H * W, nh * dh)).astype(np.float32)
        _cache[(shape, scale)] = (model, info, x, reference_bundle(vit_block_reference, info, x))
    return _cache[(shape, scale)]


def _oracle(model, feeds):
    """oracle/onnx_np.py (numpy f64) evaluates the graph; it has no Pad, so a graph that pads goes through oracle/onnx_ref.py, the same interpreter over
    torch f32, which has one"""
    from oracle import onnx_np, onnx_ref
    parsed = onnx_ref.parse_model(model)
    padded = any(nd["op"] == "Pad" for nd in parsed["nodes"])
    return np.asarray((onnx_ref if padded else onnx_np).run(parsed, feeds)[0], np.float64), padded


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exported_spelling_computes_what_the_reference_computes(shape):
    for scale in ("pre", "post"):
        model, info, x, ref = _case(shape, scale)
        got, padded = _oracle(model, {"x": x})
        err = float(np.abs(got - ref["f64"]).max())
        print(f"{shape} {scale}: oracle ({'torch f32' if padded else 'numpy f64'}) err {err:.2e} | noise {ref['noise']:.2e} tol {ref['tol']:.2e}")
        assert bool(padded) == bool(shape[5] and (shape[1] % shape[5] or shape[2] % shape[5]))
        assert got.shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])


def test_near_miss_spellings_compute_what_the_reference_computes():
    """the knobs tests/test_gpu_vit_relpos.py uses for its fall-backs: RhT as a graph input, the rel term from the scaled q (which the reference models and
    which is not what the plain block computes), a whole block, and a head size of 80"""
    B, H, W, nh, dh, ws = SHAPES[2]
    x = np.random.default_rng(11).standard_normal((B, H * W, nh * dh)).astype(np.float32)
    plain = _case(SHAPES[2])[3]
    for kw in (dict(rh_input=True), dict(rel_from="scaled"), dict(whole=True)):
        model, info = models.build_vit_block(H, W, nh * dh, nh, ws, seed=3, **kw)
        ref = reference_bundle(vit_block_reference, info, x)
        got, _ = _oracle(model, {"x": x, **({"rhT": info["rhT"]} if "rhT" in info else {})})
        assert float(np.abs(got - ref["f64"]).max()) <= ref["tol"], kw
        if "rh_input" in kw:
            assert np.array_equal(ref["f64"], plain["f64"])
        else:
            assert float(np.abs(ref["f64"] - plain["f64"]).max()) > 100 * ref["tol"]
    model, info = models.build_vit_block(6, 6, 80, 1, 0, seed=3)
    x = np.random.default_rng(11).standard_normal((1, 36, 80)).astype(np.float32)
    ref = reference_bundle(vit_block_reference, info, x)
    assert float(np.abs(_oracle(model, {"x": x})[0] - ref["f64"]).max()) <= ref["tol"]
    with pytest.raises(ValueError):
        models.build_vit_block(6, 6, 16, 1, 0, scale="post", rel_from="scaled")                   # there is no scaled q in that spelling


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_inputs_can_tell_wrong_readings_apart(shape):
    """Every wrong reading that applies to the shape -- the rw term dropped, Rh and Rw swapped (square key grids: otherwise the tables do not even fit), the
    rel term taken from the scaled q, pad keys masked out, pad keys zero instead of the bias row (padded shapes) -- moves the reference output by more than
    100 tol.  Rh and Rw are 0.5 N(0, 1) so that this holds."""
    B, H, W, nh, dh, ws = shape
    model, info, x, ref = _case(shape)
    padded = bool(ws and (H % ws or W % ws))
    applies = {"no rw": True, "swapped": bool(ws) or H == W, "rel from scaled q": True, "pad keys masked": padded, "zero pad keys": padded}
    assert set(applies) == set(VARIANTS)
    assert np.array_equal(vit_block_reference(info, x), ref["f64"])
    for variant, on in applies.items():
        if on:
            d = float(np.abs(vit_block_reference(info, x, variant=variant) - ref["f64"]).max())
            print(f"{shape} {variant}: moves the output by {d:.2e} | 100 tol {100 * ref['tol']:.2e}")
            assert d > 100 * ref["tol"], (variant, d, ref["tol"])


def test_vary_vit_graph_and_reference_agree_and_the_bias_matters():
    """build_vary_vit at a 64 x 48 image (4 x 3 tokens, ws = 2: the width pads to 4; one global block) through the oracle against the f64 encoder; every wrong
    reading moves `memory` by more than 100 tol"""
    model, info = models.build_vary_vit(image_shape=(64, 48), seed=1)
    we = info["encoder"]
    assert info["S"] == 4 and we["global_blocks"] == (1,) and we["ws"] == 2 and we["b0_rh"].shape == (2, 2, 16) and we["b1_rh"].shape == (4, 4, 16) and we["b1_rw"].shape == (3, 3, 16)
    x = np.random.default_rng(5).standard_normal((2, 1, 64, 48)).astype(np.float32)
    enc = reference_bundle(vary_vit_reference, we, x)
    got, padded = _oracle(model, {"x": x})
    err = float(np.abs(got - enc["f64"]).max())
    print(f"vary vit: oracle err {err:.2e} | noise {enc['noise']:.2e} tol {enc['tol']:.2e} | max |ref| {np.abs(enc['f64']).max():.2f}")
    assert padded and got.shape == (2, 4, 64) and err <= enc["tol"], (err, enc["tol"])
    for variant in ("no rw", "rel from scaled q", "pad keys masked", "zero pad keys"):            # ("swapped": the global block's grid is 4 x 3)
        d = float(np.abs(vary_vit_reference(we, x, variant=variant) - enc["f64"]).max())
        print(f"vary vit {variant}: {d:.2e}")
        assert d > 100 * enc["tol"], (variant, d, enc["tol"])
    with pytest.raises(ValueError):
        models.build_vary_vit(image_shape=(60, 48))


def test_default_bytes_are_those_of_the_parent():
    """encoder=None writes what build_formulanet wrote before the keyword existed (SHA-256 as computed on the parent); encoder="vit" writes the ViT encoder
    in front of the same head"""
    sha = lambda m: hashlib.sha256(m[0]).hexdigest()
    assert sha(models.build_formulanet()) == "c79b3c1ba185ffffaa5a3249b7eb826b2ee09a538baa8a71107c41165b8170d8"
    assert models.build_formulanet(encoder=None)[0] == models.build_formulanet()[0]
    model, info = models.build_formulanet(encoder="vit", image_shape=(64, 48), seed=1)
    assert model != models.build_formulanet(image_shape=(64, 48), seed=1)[0] and info["encoder"]["D"] == info["D"] == 64 and "bb_w1" not in info["weights"]
    with pytest.raises(ValueError):
        models.build_formulanet(encoder="swin")
    with pytest.raises(ValueError):
        models.build_formulanet(encoder="vit", head_only=True)


# ------------------------------------------------------------------------------------------------ the kernel's resources
VGPRS = {1: 59, 2: 77, 3: 102, 4: 119}                                                             # per DH16 = ceil(head_dim / 16), as DESIGN 4.35 records them


def test_relpos_attention_kernel_resources(tmp_path):
    """relpos_attention.hip: one kernel template, four instantiations; no scratch, no spills, no static LDS, the VGPR counts DESIGN 4.35 records; the dynamic LDS
    from the host-compiled k::relpos_attention_lds_bytes is at most 160 KB (in fact 68,352 bytes: two workgroups per CU) over the supported range"""
    src = build.CSRC / "relpos_attention.hip"
    assert "relpos_attention.hip" in build.SOURCES
    r = subprocess.run([build.HIPCC] + build.FLAGS + ["-c", str(src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    print(kernels)
    assert len(kernels) == 4 and all("relpos_attention_kernel" in k for k in kernels), sorted(kernels)
    for k, v in kernels.items():
        dh16 = int(re.search(r"relpos_attention_kernelILi(\d)E", k).group(1))
        assert v["spill"] == 0 and v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] == VGPRS[dh16], (k, v)
    prog = tmp_path / "rp_lds.cpp"
    prog.write_text('#include <cstdio>\n#include "kernels.h"\nint main() { using namespace oar::k; size_t m = 0; for (int h = 1; h <= kRpMaxGrid; ++h) for (int w = 1; w <= kRpMaxGrid; ++w) '
                    '{ size_t b = relpos_attention_lds_bytes(h, w); if (b > m) m = b; } '
                    'std::printf("%zu %zu %zu %zu\\n", m, relpos_attention_lds_bytes(48, 48), relpos_attention_lds_bytes(14, 14), relpos_attention_lds_bytes(1, 1)); return 0; }\n')
    exe = tmp_path / "rp_lds"
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O0", "-I", str(build.CSRC), "-I", str(build.CSRC.parent.parent / "include"), str(prog), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["68352", "60160", "42752", "35584"], (out.stdout, out.stderr)
    assert int(out.stdout.split()[0]) <= 160 * 1024
