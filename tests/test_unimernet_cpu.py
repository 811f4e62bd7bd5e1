"""UniMERNet, host side: the preprocessor's geometry and arithmetic, worked out by hand; the synthetic graphs (squeeze-attention head, Swin
encoder) and their torch references; the conditioning the GPU decode tests rely on; and the resources of the window-attention kernel.  Line numbers cite
the reference's processors/unimernet_preprocess.rs."""
import hashlib
import inspect
import re
import subprocess

import numpy as np
import pytest

from oar_ocr_amd import api, formula
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_reference_bundle
from oar_ocr_amd.synth.unimernet_reference import swin_block_reference, unimernet_encoder_reference

f32 = np.float32


# ------------------------------------------------------------------------------------------------ preprocessor
def test_a_single_dark_pixel_crops_to_one_pixel_and_becomes_a_square_patch():
    """:89-119 the box is inclusive and has no `min_x >= max_x` fall-back: (7, 5) alone is a 1 x 1 crop.  :130-138 scale = 192 / 1, new size 192 x 192, which
    exceeds no target side: no second resize.  :168-173 left = (672 - 192) / 2 = 240, top = 0.  PP-FormulaNet's preprocessor returns such an image as it is."""
    one = np.full((20, 30, 3), 255, np.uint8)
    one[5, 7] = 0
    p = formula.UniMERNetPreprocessor()
    assert p.target_size == (672, 192) and p.crop_threshold == 200 and p.padding_multiple == 32
    assert p.crop_rect(one) == (7, 5, 1, 1) and p.crop_margin(one).shape == (1, 1, 3)
    assert p.resized_sizes(1, 1) == ((192, 192), None)
    canvas = p.preprocess_single(one)
    assert canvas.shape == (192, 672, 3)
    assert np.all(canvas[:, 240:432] == 0) and np.all(canvas[:, :240] == 255) and np.all(canvas[:, 432:] == 255)
    assert formula.FormulaPreprocessor().crop_margin(one) is one


def test_uniform_image_and_image_without_foreground_are_returned_as_they_are():
    p = formula.UniMERNetPreprocessor()
    uniform = np.full((20, 30, 3), 77, np.uint8)
    assert p.crop_rect(uniform) is None and p.crop_margin(uniform) is uniform                     # :69 min == max
    two = np.full((10, 10, 3), 100, np.uint8)
    two[0, 0] = 101                                                                                # stretched to 0 / 255: nothing is < 0
    q = formula.UniMERNetPreprocessor(crop_threshold=0)
    assert q.crop_rect(two) is None and q.crop_margin(two) is two                                  # :114 no foreground


def test_crop_threshold_uses_the_truncating_cast():
    """(v - min) / (max - min) * 255 `as u8` truncates: with min 0, max 255 a pixel of 199 is foreground (< 200), 200 is not; the box is inclusive"""
    img = np.full((10, 10, 3), 255, np.uint8)
    img[0, 0] = 0
    img[2:5, 3:8] = 199
    img[7:9, 1:9] = 200
    assert formula.UniMERNetPreprocessor().crop_rect(img) == (0, 0, 8, 5)


def test_a_wide_image_takes_the_second_resize_with_truncated_sizes():
    """1000 x 100 (w x h): the smaller side is the height, scale = 192 / 100 = 1.92 in f32 (1.9199999571); 1000 * 1.92f = 1919.99996 rounds to the f32 1920.0
    and 100 * 1.92f = 191.999996 to 192.0, so the first size is 1920 x 192.  1920 > 672: scale_w = 672 / 1920 = 0.35f (0.3499999940), scale_h = 1, the minimum
    is 0.35f; 1920 * 0.35f = 671.99999 rounds to 672.0 and 192 * 0.35f = 67.2 truncates to 67.
    100 x 1000: 192 x 1920, then min(3.5, 0.1f) = 0.1f (0.1000000015): 192 * 0.1f = 19.2 -> 19 and 1920 * 0.1f = 192.0000029 rounds to 192.0 -> 192."""
    p = formula.UniMERNetPreprocessor()
    assert p.resized_sizes(1000, 100) == ((1920, 192), (672, 67))
    assert p.resized_sizes(100, 1000) == ((192, 1920), (19, 192))
    assert p.resized_sizes(700, 192) == ((700, 192), (672, 184))            # 672 / 700 = 0.96f: 192 * 0.96f = 184.32 -> 184
    assert p.resized_sizes(672, 192) == ((672, 192), None) and p.resized_sizes(300, 192) == ((300, 192), None)
    assert p.resized_sizes(1000, 1) == ((192000, 192), (672, 0))            # 192 * 0.0035f = 0.672 -> 0: the canvas stays white (unpinned)
    assert np.all(p.add_padding(None) == 255) and p.add_padding(None).shape == (192, 672, 3)


def test_tensor_border_grey_value_and_padded_size():
    """target 100 x 50 (w x h), multiple 32: the tensor is 64 x 128.  A 50 x 80 image (h x w) with ink in two opposite corners is cropped to itself, scale =
    50 / 50 = 1 (both resizes are skipped), left = (100 - 80) / 2 = 10, top = 0.  Grey of (10, 200, 30): ((0.299 * 10 + 0.587 * 200) + 0.114 * 30) / 255 in f32,
    then (grey - 0.7931) / 0.1738; the canvas beside the image is white: ((0.299 * 255 + 0.587 * 255) + 0.114 * 255) / 255; outside the canvas (1 - mean) / std."""
    p = formula.UniMERNetPreprocessor(target_size=(100, 50))
    assert p.padded_size() == (64, 128) and formula.UniMERNetPreprocessor().padded_size() == (192, 672)
    assert formula.UniMERNetPreprocessor(target_size=(672, 193)).padded_size() == (224, 672)
    img = np.full((50, 80, 3), 255, np.uint8)
    img[0, 0] = img[49, 79] = 0
    img[20, 30] = (10, 200, 30)
    assert p.crop_rect(img) == (0, 0, 80, 50) and p.resized_sizes(80, 50) == ((80, 50), None)
    t = p.preprocess_batch([img])
    assert t.shape == (1, 1, 64, 128) and t.dtype == np.float32
    norm = lambda grey: f32(f32(grey - f32(0.7931)) / f32(0.1738))
    grey = lambda r, g, b: f32(f32(f32(f32(0.299) * f32(r)) + f32(f32(0.587) * f32(g))) + f32(f32(0.114) * f32(b))) / f32(255.0)
    border = f32(f32(f32(1.0) - f32(0.7931)) / f32(0.1738))
    assert p.border_value() == border
    assert t[0, 0, 20, 40] == norm(grey(10, 200, 30)) and t[0, 0, 0, 10] == norm(grey(0, 0, 0)) and t[0, 0, 49, 89] == norm(f32(0.0))
    assert np.all(t[0, 0, :50, :10] == norm(grey(255, 255, 255))) and np.all(t[0, 0, :50, 90:100] == norm(grey(255, 255, 255)))
    assert np.all(t[0, 0, 50:, :] == border) and np.all(t[0, 0, :, 100:] == border)
    with pytest.raises(api.OCRError):
        p.preprocess_batch([])                                                                     # :253 "Empty image batch"


def test_predictor_model_type_defaults_to_pp_formulanet_and_refuses_unknown_types():
    par = inspect.signature(formula.FormulaRecognitionPredictor.__init__).parameters
    assert par["model_type"].default == "pp_formulanet"
    assert formula.FormulaRecognitionPredictor.MODEL_TYPES == {"pp_formulanet": ("PP-FormulaNet", (384, 384)), "unimernet": ("UniMERNet", (672, 192))}
    with pytest.raises(api.OCRError) as ex:
        formula.FormulaRecognitionPredictor(b"", formula.FormulaTokenizer(models.formula_tokenizer_spec(40)), model_type="nougat")
    assert "nougat" in str(ex.value)


# ------------------------------------------------------------------------------------------------ synthetic graphs
def test_build_formulanet_default_bytes_are_those_of_the_parent():
    """qk_squeeze = 1 writes the graph it always wrote: the SHA-256 of build_formulanet() as computed on the commit before squeeze attention"""
    assert hashlib.sha256(models.build_formulanet()[0]).hexdigest() == "c79b3c1ba185ffffaa5a3249b7eb826b2ee09a538baa8a71107c41165b8170d8"
    assert models.build_formulanet(qk_squeeze=1)[0] == models.build_formulanet()[0]


def test_squeeze_graph_parses_and_records_its_scales():
    m, info = models.build_formulanet(D=24, nh=3, F=40, V=37, Ld=2, M=5, head_only=True, with_logits=True, qk_squeeze=2)
    text = api.onnx_inspect(m)
    assert "Loop.body{inputs=fd_i,fd_cond_in,fd_tok,fd_K0,fd_V0,fd_K1,fd_V1" in text and "LayerNormalization:8" in text
    w = info["weights"]
    assert w["l0_wq"].shape == (12, 24) and w["l1_wk"].shape == (12, 24) and w["l0_wv"].shape == (24, 24) and w["l0_wcq"].shape == (24, 24)
    assert w["q_scale"] == f32(4 ** -0.5) and w["cq_scale"] == f32(8 ** -0.5) and w["qk_squeeze"] == 2
    assert "cq_scale" not in models.formula_weights(24, 3, 40, 37, 2, 7)
    with pytest.raises(ValueError):
        models.formula_weights(24, 3, 40, 37, 2, 7, qk_squeeze=3)                                  # dh = 8 is no multiple of 3


def test_build_unimernet_parses():
    m, info = models.build_unimernet(image_shape=(64, 128), V=61, M=24)
    text = api.onnx_inspect(m)
    assert "input=x" in text and "outputs=2" in text and "Softmax:4" in text and "Loop:1" in text and "Conv:6" in text
    assert info["S"] == 8 * 16 and info["D"] == 64 and info["weights"]["l0_wq"].shape == (32, 64)
    enc, _ = models.build_unimernet(image_shape=(64, 128), encoder_only=True)
    assert "outputs=1" in api.onnx_inspect(enc) and "Loop" not in api.onnx_inspect(enc)
    with pytest.raises(ValueError):
        models.build_swin_block(14, 20, 24, 3, 7)                                                  # W no multiple of ws: the padded spelling is not written


@pytest.mark.parametrize("scale", ["div", "mul"])
def test_graphs_compute_what_their_torch_references_compute(scale):
    """the graphs through the numpy ONNX oracle against synth/unimernet_reference.py in f64: 64 times the f32 rounding of values up to ~5 (4 x 2^-23 x 64)"""
    from oracle import onnx_np, onnx_ref
    tol = 64 * 4 * 2.0 ** -23
    m, info = models.build_swin_block(14, 21, 24, 3, 7, seed=3, scale=scale)
    x = np.random.default_rng(11).standard_normal((2, 14 * 21, 24)).astype(np.float32)
    got = np.asarray(onnx_np.run(onnx_ref.parse_model(m), {"x": x})[0])
    assert float(np.abs(got - swin_block_reference(info, x)).max()) <= tol
    m, info = models.build_unimernet(image_shape=(32, 64), encoder_only=True, scale=scale, seed=1)
    x = np.random.default_rng(0).random((2, 1, 32, 64)).astype(np.float32)
    got = np.asarray(onnx_np.run(onnx_ref.parse_model(m), {"x": x})[0])
    assert got.shape == (2, 4 * 8, 64) and float(np.abs(got - unimernet_encoder_reference(info["encoder"], x, scale=scale)).max()) <= tol


# ------------------------------------------------------------------------------------------------ conditioning of the GPU decode shapes
GPU_SHAPES = [(24, 3, 40, 37, 1, 9, 12, 5, 2), (40, 5, 72, 61, 2, 37, 40, 3, 2), (64, 4, 128, 300, 2, 50, 70, 2, 2), (48, 2, 64, 37, 1, 9, 6, 17, 4),
              (1024, 16, 4096, 4099, 1, 144, 16, 2, 2)]


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "D%d_nh%d_F%d_V%d_Ld%d_S%d_M%d_B%d_r%d" % s)
def test_f32_and_f64_squeeze_references_agree(shape):
    """what tests/test_gpu_unimernet_decode.py relies on, checked where no GPU is needed, no step excluded: same tokens, gap >= 8 tol, a token that keeps changing"""
    D, nh, F, V, Ld, S, M, B, r = shape
    w = models.formula_weights(D, nh, F, V, Ld, M + 2, 0, qk_squeeze=r)
    b = formula_reference_bundle(w, np.random.default_rng(1000).standard_normal((B, S, D)).astype(np.float32), M)
    assert np.array_equal(b["f32"]["tokens"], b["f64"]["tokens"])
    assert b["gap"] >= 8 * b["tol"], (b["gap"], b["tol"])
    assert b["changes"] >= B * (M - 1) // 2, b["changes"]


# ------------------------------------------------------------------------------------------------ the window-attention kernel's resources
def test_window_attention_kernel_uses_no_scratch(tmp_path):
    """window_attention.hip: one kernel, 256 threads, no scratch, no spills, at most 128 registers (4 waves per SIMD with two workgroups per CU), and no static
    LDS: all of it is dynamic, N (dh | 1) + N dh + 256 + 4 N floats <= 71,680 bytes at N dh <= 8192, N <= 256"""
    from oar_ocr_amd import build
    src = build.CSRC / "window_attention.hip"
    assert "window_attention.hip" in build.SOURCES
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
    found = {k: v for k, v in kernels.items() if "window_attention_kernel" in k}
    assert len(found) == 1 and len(kernels) == 1, sorted(kernels)
    for k, v in found.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgprs"] <= 128 and v["lds"] == 0, (k, v)
    # the LDS is dynamic: its size is the library's own formula (kernels.h), compiled here for the host alone and maximised over the supported shapes
    prog = tmp_path / "wa_lds.cpp"
    prog.write_text('#include <cstdio>\n#include "kernels.h"\nint main() { size_t m = 0; for (int ws = 1; ws * ws <= oar::k::kWinMaxN; ++ws) for (int d = 1; d <= oar::k::kWinMaxDh; ++d) '
                    'if (ws * ws * d <= oar::k::kWinMaxNd) { size_t b = oar::k::window_attention_lds_bytes(ws * ws, d); if (b > m) m = b; } '
                    'std::printf("%zu %zu %zu\\n", m, oar::k::window_attention_lds_bytes(36, 32), oar::k::window_attention_lds_bytes(144, 32)); return 0; }\n')
    exe = tmp_path / "wa_lds"
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O0", "-I", str(build.CSRC), "-I", str(build.CSRC.parent.parent / "include"), str(prog), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["71680", "10960", "40768"], (out.stdout, out.stderr)
