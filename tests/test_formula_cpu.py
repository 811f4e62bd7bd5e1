"""Formula recognition, host side: the token filter, the ByteLevel tokenizer decode, normalize_latex, the preprocessor's geometry, the synthetic model and its
torch reference, and the resources of the decode kernels.  Line numbers cite the reference (processors/formula_preprocess.rs, models/recognition/
pp_formulanet.rs, domain/adapters/formula_recognition_adapter.rs)."""
import re
import subprocess

import numpy as np
import pytest

from oar_ocr_amd import api, formula
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_reference_bundle


# ------------------------------------------------------------------------------------------------ filter_tokens (pp_formulanet.rs:364-390, verbatim)
def test_filter_tokens_stops_at_vocab_sentinel():
    assert formula.filter_tokens(np.array([[0, 42, 49_999, 4_096_990_134, 77, 2]], np.int64), 0, 2, 50_000) == [[42, 49_999]]


def test_filter_tokens_still_stops_at_eos():
    assert formula.filter_tokens(np.array([[0, 42, 2, 43]], np.int64), 0, 2, 50_000) == [[42]]


def test_filter_tokens_drops_negative_ids_and_sos_without_stopping():
    assert formula.filter_tokens(np.array([[0, -1, 5, 0, 6, 2, 7], [2, 1, 1, 1, 1, 1, 1]], np.int64), 0, 2, 50_000) == [[5, 6], []]


# ------------------------------------------------------------------------------------------------ tokenizer
def _tok(extra_added=(), **kw):
    spec = models.formula_tokenizer_spec(40, **kw)
    spec["added_tokens"] += list(extra_added)
    return formula.FormulaTokenizer(spec)


def test_special_token_ids_search_order_and_defaults():
    assert _tok().special_token_ids() == (0, 2)                                  # <s>, </s>
    spec = models.formula_tokenizer_spec(40)
    spec["added_tokens"] = [{"id": 7, "content": "[CLS]", "special": True}, {"id": 9, "content": "[BOS]", "special": True}, {"id": 5, "content": "[SEP]", "special": True}]
    assert formula.FormulaTokenizer(spec).special_token_ids() == (0, 2)         # "<s>" / "</s>" of the vocabulary come first in the search order
    for t in ("<s>", "</s>"):
        del spec["model"]["vocab"][t]
    assert formula.FormulaTokenizer(spec).special_token_ids() == (9, 5)         # [BOS] before [CLS]; [SEP] is the only eos candidate left
    spec["added_tokens"] = []
    assert formula.FormulaTokenizer(spec).special_token_ids() == (0, 2)         # nothing found: the adapter's defaults


def test_byte_level_decode_with_a_two_byte_character_and_a_skipped_special_token():
    t = _tok()
    ids = [t.token_to_id(s) for s in ("<s>", "\\frac", "{", "x", "}", "\u00c3\u00a9", "</s>", "\u0120\\beta")]
    assert None not in ids
    assert t.decode(ids) == "\\frac{x}\u00e9 \\beta"
    assert t.decode(ids, skip_special_tokens=False) == "<s>\\frac{x}\u00e9</s> \\beta"
    assert t.decode([t.token_to_id("\u00c3")] if t.token_to_id("\u00c3") is not None else [10 ** 6]) == ""      # an unknown id is skipped
    assert t.vocab_size(True) == 40 and t.vocab_size(False) == 40
    assert _tok([{"id": 40, "content": "<extra>", "special": False}]).vocab_size(True) == 41


def test_half_a_character_decodes_lossily():
    spec = models.formula_tokenizer_spec(40)
    spec["model"]["vocab"]["\u00c3"] = 40                                       # the first byte of a two-byte character alone
    assert formula.FormulaTokenizer(spec).decode([40]) == "\ufffd"


def test_other_decoders_are_refused_by_name():
    with pytest.raises(api.OCRError) as ex:
        _tok(decoder="WordPiece")
    assert "WordPiece" in str(ex.value) and "ByteLevel" in str(ex.value)


# ------------------------------------------------------------------------------------------------ normalize_latex, hand-derived
@pytest.mark.parametrize("raw, want, why", [
    ("\\text{\u901f\u5ea6}=v", "\u901f\u5ea6=v", ":272 a \\text{} around Chinese is unwrapped"),
    ("\\text{abc}", "\\text{abc}", ":272 \\text{} without Chinese stays"),
    ('a"b"', "ab", ":273 quotes go"),
    ("\\mathrm { a b }", "\\mathrm{ab}", ":279-295 a text command loses its spaces, inside the braces too"),
    ("x + y", "x+y", ":343 non-letter -> letter ('+ y') in the walk, then :364 letter -> non-letter ('x +')"),
    ("1 + 2", "1+2", ":339 non-letter -> non-letter"),
    ("a b", "a b", ":347 letter -> letter spaces stay"),
    ("\\alpha \\beta", "\\alpha\\beta", ":364 a letter before a backslash: the space goes ('a \\\\')"),
    ("x\\ \\ y", "x\\ \\ y", ":309-328 the thin space `\\ ` starts no match, twice in a row"),
    ("  a  ", "a", ":371 trim"),
    ("a 1 b", "a1b", ":343 the walk joins '1 b', :364 the pattern joins 'a 1': both halves of one iteration"),
])
def test_normalize_latex(raw, want, why):
    got = formula.normalize_latex(raw)
    assert got == want, why
    assert formula.normalize_latex(got) == got                                   # a fixed point


def test_normalize_latex_reaches_its_fixed_point_in_one_changing_iteration():
    """The loop (:306) runs until nothing changes, at most 10 times.  No input was found whose text changes in two successive iterations -- every string of up
    to 8 characters over {a, 1, space, backslash, tab} was tried -- so the second iteration only confirms the first: checked here on all strings of up to 6."""
    import itertools
    for n in range(1, 7):
        for t in itertools.product("a1 \\\t", repeat=n):
            once = formula.normalize_latex("".join(t))
            assert formula.normalize_latex(once) == once


# ------------------------------------------------------------------------------------------------ preprocessor
def test_uniform_image_and_image_without_foreground_are_returned_as_they_are():
    p = formula.FormulaPreprocessor()
    uniform = np.full((20, 30, 3), 77, np.uint8)
    assert p.crop_rect(uniform) is None and p.crop_margin(uniform) is uniform                     # :92 min == max
    one = np.full((20, 30, 3), 255, np.uint8)
    one[5, 7] = 0                                                                                  # a single dark pixel: min_x >= max_x (:128)
    assert p.crop_rect(one) is None and p.crop_margin(one) is one
    bright = np.full((20, 30, 3), 250, np.uint8)
    bright[0, 0] = 255                                                                             # stretched: 0 everywhere but one pixel -> the box is the whole image
    assert p.crop_rect(bright) == (0, 0, 30, 20)


def test_crop_threshold_uses_the_truncating_cast():
    """(v - min) / (max - min) * 255 `as u8` truncates: with min 0, max 255 a pixel of 200 is foreground only below the threshold 200 + 1"""
    img = np.full((10, 10, 3), 255, np.uint8)
    img[0, 0] = 0
    img[2:5, 3:8] = 199                                   # 199 < 200: foreground
    img[7:9, 1:9] = 200                                   # 200 is not < 200: background
    assert formula.FormulaPreprocessor().crop_rect(img) == (0, 0, 8, 5)


def test_grey_image_with_a_known_foreground_box():
    """target 50 x 36 (w x h): the crop is 20 x 36, scale = 36 / 36 = 1 (no resampling), centred at left = (50 - 20) / 2 = 15, top = 0; tensor padded to 64 x 48 with 1.0"""
    p = formula.FormulaPreprocessor(target_size=(50, 36))
    img = np.full((60, 70, 3), 255, np.uint8)
    img[10:46, 30:50] = 40
    img[12, 33] = 0                                       # (min = 0, so the stretch is v / 255 * 255)
    assert p.crop_rect(img) == (30, 10, 20, 36)
    assert p.resized_size(20, 36) == (20, 36) and p.padded_size() == (48, 64)
    t = p.preprocess_batch([img])
    assert t.shape == (1, 1, 48, 64) and t.dtype == np.float32
    g = lambda v: np.float32(np.float32(np.float32(v) * (np.float32(1.0) / np.float32(255.0)) - np.float32(0.7931)) / np.float32(0.1738))
    lum = lambda v: np.float32(np.float32(np.float32(0.114) * g(v) + np.float32(0.587) * g(v)) + np.float32(0.299) * g(v))
    assert np.all(t[0, 0, :36, 15:35][np.arange(36) != 2] == lum(40)) and t[0, 0, 2, 18] == lum(0)
    assert np.all(t[0, 0, :36, :15] == lum(0)) and np.all(t[0, 0, :36, 35:50] == lum(0))          # black beside the image, normalised
    assert np.all(t[0, 0, 36:, :] == 1.0) and np.all(t[0, 0, :, 50:] == 1.0)                       # the 1.0 border outside the target rectangle


def test_resized_size_truncates():
    p = formula.FormulaPreprocessor()                     # 384 x 384
    assert p.resized_size(100, 33) == (384, 126)          # 33 * 3.84 = 126.72: `as u32` gives 126 where rounding gives 127
    assert p.resized_size(33, 100) == (126, 384)
    assert p.resized_size(1000, 3) == (384, 1) and p.resized_size(1000, 2) == (384, 0)
    assert np.all(p.resize_and_pad(np.zeros((2, 1000, 3), np.uint8)) == 0) and p.resize_and_pad(np.zeros((0, 5, 3), np.uint8)).shape == (384, 384, 3)


# ------------------------------------------------------------------------------------------------ synthetic model and reference
GPU_SHAPES = [(24, 3, 40, 37, 1, 9, 12, 5), (40, 5, 72, 61, 2, 37, 40, 3), (64, 4, 128, 300, 2, 50, 70, 2), (24, 3, 40, 37, 1, 9, 6, 17), (24, 3, 40, 37, 1, 9, 1, 1),
              (384, 16, 1536, 4099, 2, 144, 48, 2)]


def test_build_formulanet_parses():
    m, info = models.build_formulanet(D=24, nh=3, F=40, V=37, Ld=2, M=5, head_only=True, with_logits=True)
    text = api.onnx_inspect(m)
    assert "Loop.body{inputs=fd_i,fd_cond_in,fd_tok,fd_K0,fd_V0,fd_K1,fd_V1 outputs=fd_cond_out,fd_tok_new,fd_K0_new,fd_V0_new,fd_K1_new,fd_V1_new,fd_tok_new,fd_logits" in text
    assert "LayerNormalization:8" in text and "Gelu:2" in text
    full, _ = models.build_formulanet(D=24, nh=3, F=40, V=37, Ld=1, M=5, spelling="matmul", q_scale="before")
    assert "input=x" in api.onnx_inspect(full) and "Conv:2" in api.onnx_inspect(full)
    assert info["weights"]["q_scale"] == np.float32(8 ** -0.5) and info["weights"]["c_pos"] == 2


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "D%d_nh%d_F%d_V%d_Ld%d_S%d_M%d_B%d" % s)
def test_f32_and_f64_references_agree(shape):
    """the conditioning the GPU test relies on, checked where no GPU is needed: same tokens, gap >= 8 tol, and (M > 1) a token that keeps changing"""
    D, nh, F, V, Ld, S, M, B = shape
    w = models.formula_weights(D, nh, F, V, Ld, M + 2, 0)
    r = formula_reference_bundle(w, np.random.default_rng(1000).standard_normal((B, S, D)).astype(np.float32), M)
    assert np.array_equal(r["f32"]["tokens"], r["f64"]["tokens"])
    assert r["gap"] >= 8 * r["tol"], (r["gap"], r["tol"])
    assert M == 1 or r["changes"] >= B * (M - 1) // 2, r["changes"]


# ------------------------------------------------------------------------------------------------ the decode kernels' resources
def test_formula_decode_kernels_use_no_scratch():
    """formula_decode.hip: every step launches these kernels 8 Ld + 2 times; a spill would be paid on each"""
    from oar_ocr_amd import build
    src = build.CSRC / "formula_decode.hip"
    r = subprocess.run([build.HIPCC] + build.FLAGS + ["-c", str(src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    for family, count in (("fd_rows_kernel", 5), ("fd_qkv_rows_kernel", 5), ("fd_lm_head_kernel", 5), ("fd_self_attn_kernel", 1), ("fd_cross_attn_kernel", 1), ("fd_combine_kernel", 1)):
        found = {k: v for k, v in kernels.items() if family in k}
        assert len(found) == count, (family, sorted(kernels))
        for k, v in found.items():
            assert v["spill"] == 0 and v["scratch"] == 0 and v["vgprs"] <= 128 and v["lds"] <= 64 * 1024, (k, v)     # 256 threads: 128 registers keep 4 waves per SIMD
