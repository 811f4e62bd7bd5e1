"""Multi-head attention with separate q / k / v sources, host side: the exported spellings of synth.models.build_mha / build_aifi_layer /
build_table_cell_det(encoder_layers=1) through the ONNX oracles against the torch f64 reference written from the formulas (synth/mha_reference.py), inputs
that tell the wrong readings of the block from the right one, the existing builders' default bytes, and the kernel's resources.

Tolerance, as elsewhere in the project: noise = max |torch f32 - f64|, tol = max(16 noise, 2^-19)."""
import hashlib
import re
import subprocess

import numpy as np
import pytest

from oar_ocr_amd import build
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.mha_reference import VARIANTS, aifi_layer_reference, aifi_stack_reference, mha_reference, reference_bundle

#        N  Tq  Tk nh  dh   (small relatives of the shapes of tests/test_gpu_mha_attention.py)
SELF = (2, 20, 20, 4, 8)
CROSS = (1, 70, 33, 1, 64)
RTDETR_DECODER_SHA = "9ac9b45cecd0edf943ca6d3ad2f753a90d1c2d9aeda6c1c74046e6ba6a3aea37"                   # build_rtdetr_decoder(), on the parent commit


def _inputs(N, Tq, Tk, nh, dh, cross):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, Tq, nh * dh)).astype(np.float32)
    return {"x": x, **({"mem": rng.standard_normal((N, Tk, nh * dh)).astype(np.float32)} if cross else {})}


def _oracle(model, feeds, want=None):
    """oracle/onnx_np.py (numpy f64) evaluates a whole graph; `want` names intermediate tensors of a graph with a TopK behind them, which goes through
    oracle/onnx_ref.py (the same interpreter over torch f32) up to the first TopK"""
    from oracle import onnx_np, onnx_ref
    parsed = onnx_ref.parse_model(model)
    if want is None:
        return np.asarray(onnx_np.run(parsed, feeds)[0], np.float64)
    nodes = []
    for nd in parsed["nodes"]:
        if nd["op"] == "TopK":
            break
        nodes.append(nd)
    return [np.asarray(v) for v in onnx_ref.run({"nodes": nodes, "inits": parsed["inits"], "inputs": [], "outputs": list(want)}, feeds, want=list(want))]


@pytest.mark.parametrize("scale", ["post", "pre"])
@pytest.mark.parametrize("shape,cross", [(SELF, False), (CROSS, True), ((1, 12, 12, 2, 8), True)], ids=["self", "cross", "cross_Tq_eq_Tk"])
def test_exported_spelling_computes_what_the_reference_computes(shape, cross, scale):
    model, info = models.build_mha(*shape, seed=3, scale=scale, shared_qk=not cross)
    assert info["self"] == (not cross)
    feeds = _inputs(*shape, cross)
    ref = reference_bundle(mha_reference, info, feeds["x"], feeds.get("mem"))
    got = _oracle(model, feeds)
    err = float(np.abs(got - ref["f64"]).max())
    print(f"{shape} {scale} {'cross' if cross else 'self'}: oracle err {err:.2e} | noise {ref['noise']:.2e} tol {ref['tol']:.2e}")
    assert got.shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])


def test_near_miss_spellings_compute_what_the_reference_computes():
    """the knobs tests/test_gpu_mha_attention.py uses for its fall-backs: an additive mask, the scores as a graph output, no position constant"""
    feeds = _inputs(*SELF, False)
    plain = reference_bundle(mha_reference, models.build_mha(*SELF, seed=3)[1], feeds["x"])
    for kw in (dict(mask=True), dict(scores_output=True), dict(pos=False)):
        model, info = models.build_mha(*SELF, seed=3, **kw)
        ref = reference_bundle(mha_reference, info, feeds["x"])
        err = float(np.abs(_oracle(model, feeds) - ref["f64"]).max())
        assert err <= ref["tol"], (kw, err, ref["tol"])
        if "scores_output" in kw:
            assert np.array_equal(ref["f64"], plain["f64"])
        else:
            assert float(np.abs(ref["f64"] - plain["f64"]).max()) > 100 * ref["tol"], kw
    with pytest.raises(ValueError):
        models.build_mha(*SELF, scale="div")


def test_aifi_layer_and_the_detectors_encoder_compute_what_the_reference_computes():
    H, W, D, nh, F = 5, 7, 32, 4, 64
    model, info = models.build_aifi_layer(H, W, D, nh, F, seed=2)
    src = np.random.default_rng(5).standard_normal((2, H * W, D)).astype(np.float32)
    ref = reference_bundle(aifi_layer_reference, info, src)
    err = float(np.abs(_oracle(model, {"src": src}) - ref["f64"]).max())
    print(f"aifi layer: oracle err {err:.2e} | noise {ref['noise']:.2e} tol {ref['tol']:.2e}")
    assert err <= ref["tol"], (err, ref["tol"])
    pos = models.sincos_2d(2, 3, 8)                                                                # token (y, x) = (1, 2) is row 5; omega = (1, 0.01)
    assert pos.shape == (1, 6, 8) and np.allclose(pos[0, 5], [np.sin(2.0), np.sin(0.02), np.cos(2.0), np.cos(0.02), np.sin(1.0), np.sin(0.01), np.cos(1.0), np.cos(0.01)], atol=1e-7)
    # the detector: the AIFI stack between its two named tensors
    model, info = models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24, decoder_layers=2, encoder_layers=1)
    a = info["aifi"]
    assert info["encoder_layers"] == 1 and (a["H"], a["W"], a["D"], len(a["layers"])) == (4, 4, 64, 1)
    x = np.random.default_rng(6).random((2, 3, 128, 128)).astype(np.float32)
    t_in, t_out = _oracle(model, {"image": x}, want=[a["in"], a["out"]])
    ref = reference_bundle(aifi_stack_reference, a, t_in)
    err = float(np.abs(t_out.astype(np.float64) - ref["f64"]).max())
    print(f"detector encoder: oracle (torch f32) err {err:.2e} | noise {ref['noise']:.2e} tol {ref['tol']:.2e}")
    assert t_in.shape == (2, 16, 64) and t_out.shape == (2, 16, 64) and err <= ref["tol"], (err, ref["tol"])
    with pytest.raises(ValueError):
        models.build_aifi_layer(4, 4, 30, 2, 64)                                                   # D must be a multiple of 4


def test_the_inputs_can_tell_wrong_readings_apart():
    """Every wrong reading -- v read from x + pos, k without pos, the scale dropped, heads merged in the wrong order, softmax over the query axis -- moves
    the reference output by more than 100 tol, for the block on its own and inside the AIFI layer.  The position constant is N(0, 1) and the q / k Linears
    have gain 2 so that this holds."""
    model, info = models.build_mha(*SELF, seed=3)
    x = _inputs(*SELF, False)["x"]
    ref = reference_bundle(mha_reference, info, x)
    assert np.array_equal(mha_reference(info, x), ref["f64"])
    H, W, D, nh, F = 5, 7, 32, 4, 64
    ainfo = models.build_aifi_layer(H, W, D, nh, F, seed=2)[1]
    src = np.random.default_rng(5).standard_normal((2, H * W, D)).astype(np.float32)
    aref = reference_bundle(aifi_layer_reference, ainfo, src)
    for variant in VARIANTS:
        d = float(np.abs(mha_reference(info, x, variant=variant) - ref["f64"]).max())
        da = float(np.abs(aifi_layer_reference(ainfo, src, variant=variant) - aref["f64"]).max())
        print(f"{variant}: block moves by {d / ref['tol']:.0f} tol, AIFI layer by {da / aref['tol']:.0f} tol")
        assert d > 100 * ref["tol"] and da > 100 * aref["tol"], (variant, d, ref["tol"], da, aref["tol"])


def test_default_bytes_are_those_of_the_parent():
    """encoder_layers=0 writes what the builders wrote before the keyword existed: the SHA-256 values the existing tests hold, restated, and
    build_rtdetr_decoder's defaults as computed on the parent commit"""
    sha = lambda m: hashlib.sha256(m[0]).hexdigest()
    det = models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24)
    assert len(det[0]) == 287396 and sha(det) == "fc70273f09319c31308ac88f6dfb320868e7f64794c03c912506f210f95603fe"
    assert models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24, encoder_layers=0)[0] == det[0] and "aifi" not in det[1]
    assert sha(models.build_formulanet()) == "c79b3c1ba185ffffaa5a3249b7eb826b2ee09a538baa8a71107c41165b8170d8"
    assert sha(models.build_swin_block(14, 21, 24, 3, 7, seed=3)) == "8846212ecc6f31f685bc0af9ed7e676f8955265dd9204d6e8ba97a39b9c79734"
    assert sha(models.build_swin_block(14, 21, 24, 3, 7, seed=3, whole=True)) == "15c2f4cbf550bda5a21516b70345b6b8f266fb97b943050583acba3e3fb1e4a1"
    assert sha(models.build_unimernet()) == "04f5d76c4d2e6253280b7d5104ef61ca594befa9df553d0b2271943c1e2379b7"
    assert sha(models.build_rtdetr_decoder()) == RTDETR_DECODER_SHA
    with_dec = models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24, decoder_layers=2)
    with_enc = models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24, decoder_layers=2, encoder_layers=1)
    assert with_enc[0] != with_dec[0] and "aifi" not in with_dec[1]


# ------------------------------------------------------------------------------------------------ the kernel's resources
VGPRS = {1: 52, 2: 69, 3: 90, 4: 106}                                                              # per DH16 = ceil(head_dim / 16), as DESIGN 4.36 records them


def test_mha_attention_kernel_resources(tmp_path):
    """mha_attention.hip: one kernel template, four instantiations; no scratch, no spills, no static LDS, the VGPR counts DESIGN 4.36 records; the dynamic LDS
    from the host-compiled k::mha_attention_lds_bytes lets two workgroups share a CU's 160 KB at head sizes 16, 32 and 64 (in fact 34,816 bytes: four)"""
    src = build.CSRC / "mha_attention.hip"
    assert "mha_attention.hip" in build.SOURCES
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
    assert len(kernels) == 4 and all("mha_attention_kernel" in k for k in kernels), sorted(kernels)
    for k, v in kernels.items():
        dh16 = int(re.search(r"mha_attention_kernelILi(\d)E", k).group(1))
        assert v["spill"] == 0 and v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] == VGPRS[dh16], (k, v)
    prog = tmp_path / "mha_lds.cpp"
    prog.write_text('#include <cstdio>\n#include "kernels.h"\nint main() { using namespace oar::k; '
                    'std::printf("%zu %zu %zu %d\\n", mha_attention_lds_bytes(16), mha_attention_lds_bytes(32), mha_attention_lds_bytes(64), kMhaMaxDh); return 0; }\n')
    exe = tmp_path / "mha_lds"
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O0", "-I", str(build.CSRC), "-I", str(build.CSRC.parent.parent / "include"), str(prog), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["34816", "34816", "34816", "64"], (out.stdout, out.stderr)
    assert all(2 * int(b) <= 160 * 1024 for b in out.stdout.split()[:3])
