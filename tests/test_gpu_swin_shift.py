"""Shifted, masked and padded Swin windows on the GPU (csrc/window_attention.hip): the block whose grid is padded at the bottom / right to a
multiple of the window, rolled by the shift and given a per-window mask still is ONE WindowAttention launch -- the pad, both rolls, the mask's 5-D Reshapes
and Add, and the crop are address arithmetic in the kernel, and no copy of the token tensor is made for them.  Graphs: synth.models.build_swin_block with
shift / mask / pad_value, and build_unimernet(ws=7, shifted=True) whose stages pad and shift.

Reference: the same block in torch on the CPU, in f64 and f32 (synth/unimernet_reference.py: F.pad, torch.roll, the mask per window, the crop); noise =
max |f32 - f64|, tol = max(16 noise, 2^-19).  tests/test_swin_shift_cpu.py shows that a dropped or wrongly indexed mask, a missing or one-axis shift and a
wrong pad-key rule each move these outputs by more than 100 tol.
Per case: exactly one launch of class window_attention with the pass on, none with OAR_FUSE_WINDOW_ATTENTION=0, both outputs within tol of f64, as many
launches in all as the aligned, unshifted, unmasked block takes, and two fused runs byte-identical."""
import json

import numpy as np
import pytest

from oar_ocr_amd import api, formula
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_reference_bundle
from oar_ocr_amd.synth.unimernet_reference import reference_bundle, swin_block_reference, unimernet_encoder_reference

pytestmark = pytest.mark.gpu

#          B   H   W   C nh  ws  s  mask
SHAPES = [(2, 10, 13, 24, 3, 7, 3, "swin"),      # padded on both axes, shifted, 4 windows
          (1, 8, 8, 16, 2, 4, 2, "swin"),        # aligned, shifted
          (1, 8, 12, 16, 2, 4, 2, "random"),     # mask indexing, 6 windows, hb != wb
          (1, 9, 6, 32, 1, 4, 0, None),          # padded only: pad keys carry the k / v biases
          (2, 6, 12, 16, 2, 6, 3, "swin"),       # one window row, the roll wraps inside it
          (1, 16, 32, 32, 1, 16, 8, "swin"),     # N = 256, more than 64 KB of LDS, with a mask
          (1, 8, 8, 16, 2, 4, 0, "random")]      # a mask without a roll
IDS = ["B%d_H%d_W%d_C%d_nh%d_ws%d_s%d_%s" % s for s in SHAPES]

_cache = {}


def _random_mask(H, W, ws):
    """U(-4, 0) per (window, i, j)"""
    nW = -(-H // ws) * -(-W // ws)
    return (-4.0 * np.random.default_rng(5).random((nW, ws * ws, ws * ws))).astype(np.float32)


def _case(shape, scale, **kw):
    """model, input, reference bundle: computed once, never modified"""
    key = (shape, scale, tuple(sorted(kw.items())))
    if key not in _cache:
        B, H, W, C, nh, ws, s, mask = shape
        args = dict(seed=3, scale=scale, shift=s, mask=_random_mask(H, W, ws) if mask == "random" else mask, pad_value=0.0)
        args.update(kw)
        model, info = models.build_swin_block(H, W, C, nh, ws, **args)
        x = np.random.default_rng(11).standard_normal((B, H * W, C)).astype(np.float32)
        _cache[key] = (model, x, reference_bundle(swin_block_reference, info, x))
    return _cache[key]


def _run(model, x, monkeypatch, fuse):
    """-> (y, launches of class window_attention in one infer, the profile)"""
    if fuse is None:
        monkeypatch.delenv("OAR_FUSE_WINDOW_ATTENTION", raising=False)
    else:
        monkeypatch.setenv("OAR_FUSE_WINDOW_ATTENTION", fuse)      # (read when the graph is loaded)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        y = dict(eng.infer(x))["y"]
        snap = {e["name"]: e for e in api.prof_snapshot()}
        return y, snap.get("window_attention", {}).get("launches", 0), snap
    finally:
        api.prof_enable(False)
        eng.close()


def _launches(snap):
    return sum(e["launches"] for e in snap.values())


@pytest.mark.parametrize("scale", ["div", "mul"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_launch_no_extra_launch_and_both_routes_match_f64(shape, scale, monkeypatch):
    B, H, W, C, nh, ws, s, mask = shape
    model, x, ref = _case(shape, scale)
    fused, n_fused, snap = _run(model, x, monkeypatch, None)
    again, _, _ = _run(model, x, monkeypatch, None)
    plain, n_plain, snap0 = _run(model, x, monkeypatch, "0")
    base_model, _ = models.build_swin_block(2 * ws, 2 * ws, C, nh, ws, seed=3, scale=scale)       # aligned, unshifted, unmasked: the 4.33 spelling
    _, n_base, snap_base = _run(base_model, np.zeros((1, 4 * ws * ws, C), np.float32), monkeypatch, None)
    e1 = float(np.abs(fused.astype(np.float64) - ref["f64"]).max())
    e0 = float(np.abs(plain.astype(np.float64) - ref["f64"]).max())
    print(f"{shape} {scale}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} | fused err {e1:.2e} ({_launches(snap)} launches; the plain block {_launches(snap_base)}) | "
          f"op-by-op err {e0:.2e} ({_launches(snap0)} launches)")
    assert n_fused == 1, sorted((k, v["launches"]) for k, v in snap.items())
    assert n_plain == 0, sorted((k, v["launches"]) for k, v in snap0.items())
    assert fused.shape == ref["f64"].shape and e1 <= ref["tol"], (e1, ref["tol"])
    assert e0 <= ref["tol"], (e0, ref["tol"])
    assert n_base == 1 and _launches(snap) == _launches(snap_base), (sorted((k, v["launches"]) for k, v in snap.items()), sorted((k, v["launches"]) for k, v in snap_base.items()))
    assert np.array_equal(fused, again)


@pytest.mark.parametrize("kw", [dict(pad_value=1.0), dict(unroll=2)], ids=["pad_value_1", "reverse_roll_2_of_3"])
def test_spellings_that_are_not_swin_keep_the_op_by_op_route(kw, monkeypatch):
    """a Pad with a non-zero value, and a reverse roll that is not the inverse of the forward one: not matched, and the op-by-op route gives the reference's numbers"""
    model, x, ref = _case(SHAPES[0], "div", **kw)
    y, n, snap = _run(model, x, monkeypatch, None)
    y0, n0, _ = _run(model, x, monkeypatch, "0")
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max())
    print(f"fall-back {kw}: err {err:.2e} tol {ref['tol']:.2e} ({_launches(snap)} launches)")
    assert n == 0 and n0 == 0, sorted((k, v["launches"]) for k, v in snap.items())
    assert np.array_equal(y, y0) and err <= ref["tol"], (err, ref["tol"])


def test_whole_block_fuses_too(monkeypatch):
    """the whole block (conv enhance and MLP behind the attention) on the first case: one launch, within tol"""
    model, x, ref = _case(SHAPES[0], "div", whole=True)
    y, n, snap = _run(model, x, monkeypatch, None)
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max())
    print(f"whole block: err {err:.2e} tol {ref['tol']:.2e} noise {ref['noise']:.2e}")
    assert n == 1 and err <= ref["tol"], (n, err, ref["tol"])


# ------------------------------------------------------------------------------------------------ the encoder that pads and shifts, and the predictor on it
ENC = dict(image_shape=(64, 96), ws=7, shifted=True, depths=(2, 2), V=61, M=24, seed=1)            # (tests/test_swin_shift_cpu.py checks this seed's conditioning)
BLOCKS = 4


def _crop(seed):
    """a 96 x 64 crop with ink in two opposite corners: the margin crop keeps it whole and both resizes are the identity"""
    rng = np.random.default_rng(seed)
    img = np.full((64, 96, 3), 245, np.uint8)
    img[0, 0] = img[63, 95] = 0
    for _ in range(10):
        y, x = int(rng.integers(4, 52)), int(rng.integers(4, 78))
        img[y:y + int(rng.integers(2, 6)), x:x + int(rng.integers(4, 14))] = (int(rng.integers(0, 90)), int(rng.integers(0, 90)), int(rng.integers(0, 90)))
    return img


@pytest.fixture(scope="module")
def encoder():
    model, info = models.build_unimernet(**ENC)
    crops = [_crop(1), _crop(2)]
    t = formula.UniMERNetPreprocessor(target_size=(96, 64)).preprocess_batch(crops)
    assert t.shape == (2, 1, 64, 96)
    return model, info, crops, t, reference_bundle(unimernet_encoder_reference, info["encoder"], t)


def test_encoder_that_pads_and_shifts(encoder):
    """token grids 16 x 24 (padded to 21 x 28) and 8 x 12 (to 14 x 14), the odd blocks shifted by 3 with the "swin" mask, B = 2: `memory` within tol of the f64
    encoder, one WindowAttention launch per block"""
    model, info, crops, t, enc = encoder
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        outs = dict(eng.infer(t))
        snap = {e["name"]: e for e in api.prof_snapshot()}
    finally:
        api.prof_enable(False)
        eng.close()
    mem = outs["memory"]
    err = float(np.abs(mem.astype(np.float64) - enc["f64"]).max())
    print(f"memory: max |gpu - f64| {err:.2e} | tol {enc['tol']:.2e} | torch f32 noise {enc['noise']:.2e} | max |ref| {np.abs(enc['f64']).max():.2f} | {_launches(snap)} launches")
    assert snap.get("window_attention", {}).get("launches") == BLOCKS, sorted((k, v["launches"]) for k, v in snap.items())
    assert mem.shape == (2, info["S"], info["D"]) and err <= enc["tol"], (err, enc["tol"])


def test_predictor_on_the_encoder_that_pads_and_shifts(encoder, tmp_path):
    """FormulaRecognitionPredictor(model_type="unimernet") returns the strings the f64 reference yields on the preprocessor's own tensor (f64 encoder, f64
    head, the shared decode), under the gap rule of tests/test_gpu_unimernet.py"""
    model, info, crops, t, enc = encoder
    ref = formula_reference_bundle(info["weights"], enc["f64"], ENC["M"])
    print(f"head from the f64 memory: tol {ref['tol']:.2e} | gap {ref['gap']:.2e}")
    assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for these crops", ref["gap"], ref["tol"])
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(models.formula_tokenizer_spec(ENC["V"])), encoding="utf-8")
    p = formula.FormulaRecognitionPredictor(model, path, formula.FormulaRecognitionConfig(batch_size=2), model_type="unimernet", target_size=(96, 64))
    try:
        assert isinstance(p.preprocessor, formula.UniMERNetPreprocessor) and p.preprocessor.target_size == (96, 64)
        assert np.array_equal(p.preprocessor.preprocess_batch(crops), t)
        want = p.decode(ref["tokens"])
        out = p.predict(crops)
        print(out.formulas)
        assert out.formulas == want and all(want), (out.formulas, want)
    finally:
        p.close()
