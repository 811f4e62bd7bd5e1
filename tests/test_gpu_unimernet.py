"""UniMERNet end to end on the GPU: synth.models.build_unimernet at target (128, 64) -- stem, two stages of two Swin blocks (ws = 4) with patch
merging, final LayerNorm, a two-layer squeeze-attention decode Loop -- through the engine (one WindowAttention launch per block, the Loop as FormulaDecode)
and through `formula.FormulaRecognitionPredictor(model_type="unimernet")`.

  (a) `memory` against the f64 encoder (synth/unimernet_reference.py) within the network budget 1e-3 max(1, max |ref|); the error is printed
  (b) token_ids equal the f64 head (synth/formula_reference.py) run from the GPU's own `memory`, under the gap rule of test_gpu_formula_decode.py
  (c) the predictor's strings from RGB images equal those of the reference path -- UniMERNetPreprocessor's tensor -> f64 encoder -> f64 head -> the shared
      decode --, with and without stop_at_eos.  The crops are 128 x 64 with ink in two opposite corners, so the margin crop keeps them whole and both resizes
      are the identity; eos is chosen from the reference as in test_gpu_formula_stop_predictor.py."""
import json

import numpy as np
import pytest

from oar_ocr_amd import api, formula
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_reference_bundle
from oar_ocr_amd.synth.unimernet_reference import reference_bundle, unimernet_encoder_reference

pytestmark = pytest.mark.gpu

V, M, SEED = 61, 24, 1
BLOCKS = 4


def _crop(seed):
    rng = np.random.default_rng(seed)
    img = np.full((64, 128, 3), 245, np.uint8)
    img[0, 0] = img[63, 127] = 0
    for _ in range(10):
        y, x = int(rng.integers(4, 52)), int(rng.integers(4, 110))
        img[y:y + int(rng.integers(2, 6)), x:x + int(rng.integers(4, 14))] = (int(rng.integers(0, 90)), int(rng.integers(0, 90)), int(rng.integers(0, 90)))
    return img


def _tokenizer_with_eos(eos):
    """models.formula_tokenizer_spec with `</s>` moved from id 2 to `eos`"""
    spec = models.formula_tokenizer_spec(V)
    vocab = spec["model"]["vocab"]
    old = next(k for k, v in vocab.items() if v == eos)
    del vocab[old], vocab["</s>"]
    vocab["</s>"], vocab["t2"] = eos, 2
    spec["added_tokens"] = [a for a in spec["added_tokens"] if a["content"] != "</s>"] + [{"id": eos, "content": "</s>", "special": True}]
    return spec


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    model, info = models.build_unimernet(image_shape=(64, 128), V=V, M=M, seed=SEED)
    crops = [_crop(1), _crop(2), _crop(3)]
    t = formula.UniMERNetPreprocessor(target_size=(128, 64)).preprocess_batch(crops)
    assert t.shape == (3, 1, 64, 128)
    enc = reference_bundle(unimernet_encoder_reference, info["encoder"], t)
    ref = formula_reference_bundle(info["weights"], enc["f64"], M)
    assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for these crops", ref["gap"], ref["tol"])
    tok = ref["tokens"]
    firsts = {e: [int(np.nonzero(r == e)[0][0]) for r in tok] for e in range(4, V) if all(np.any(r[:M - 1] == e) for r in tok)}
    assert firsts, "no token occurs in every row of the reference before the last step: choose other crops"
    eos = min(firsts, key=lambda e: (-min(firsts[e]), e))
    assert eos == 13 and firsts[eos] == [11, 6, 9]            # (what seed 1 and these crops give)
    path = tmp_path_factory.mktemp("unimernet") / "tokenizer.json"
    path.write_text(json.dumps(_tokenizer_with_eos(eos)), encoding="utf-8")
    return model, info, path, crops, t, enc, tok, eos


def test_encoder_memory_and_tokens(setup):
    model, info, path, crops, t, enc, ref_tokens, eos = setup
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        outs = eng.infer(t)
        snap = {e["name"]: e for e in api.prof_snapshot()}
    finally:
        api.prof_enable(False)
        eng.close()
    assert outs[0][0] == "token_ids"                         # the first output: what unimernet.rs reads
    outs = dict(outs)
    mem = outs["memory"]
    assert mem.shape == (3, info["S"], info["D"]) and outs["token_ids"].shape == (3, M) and outs["token_ids"].dtype == np.int64
    err = float(np.abs(mem.astype(np.float64) - enc["f64"]).max())
    budget = 1e-3 * max(1.0, float(np.abs(enc["f64"]).max()))
    print(f"(a) memory: max |gpu - f64| {err:.2e} | budget {budget:.2e} | torch f32 noise {enc['noise']:.2e} | max |ref| {np.abs(enc['f64']).max():.2f}")
    assert snap.get("window_attention", {}).get("launches") == BLOCKS, sorted((k, v["launches"]) for k, v in snap.items())
    assert err <= budget, (err, budget)
    ref = formula_reference_bundle(info["weights"], mem, M)
    print(f"(b) head from the GPU's memory: noise {ref['noise']:.2e} | tol {ref['tol']:.2e} | gap {ref['gap']:.2e} token changes {ref['changes']}")
    assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for this memory", ref["gap"], ref["tol"])
    assert np.array_equal(outs["token_ids"], ref["tokens"]), ("tokens differ at (image, step)", np.argwhere(outs["token_ids"] != ref["tokens"])[:4])


def test_predictor_strings_with_and_without_the_stop(setup):
    model, info, path, crops, t, enc, ref_tokens, eos = setup
    got = {}
    for stop in (True, False):
        p = formula.FormulaRecognitionPredictor(model, path, formula.FormulaRecognitionConfig(batch_size=2), stop_at_eos=stop, model_type="unimernet")
        try:
            assert isinstance(p.preprocessor, formula.UniMERNetPreprocessor) and p.preprocessor.target_size == (128, 64) and p.preprocessor.padding_multiple == 32
            assert p.eos_token_id == eos and p.model_name == "UniMERNet"
            want = p.decode(ref_tokens)
            out = p.predict(crops)                            # batch_size 2: two infers, the last with one image (first eos at step 9)
            st = p.decode_stats()
            print(f"stop_at_eos = {stop}: {out.formulas} | {st}")
            assert out.formulas == want and all(want), (out.formulas, want)
            if stop:
                assert st.steps_executed == 10 and st.steps_limit == M, st
            else:
                assert st.steps_executed == st.steps_limit == st.steps_enqueued == M, st
            got[stop] = out.formulas
        finally:
            p.close()
    assert got[True] == got[False]


def _wide_crop(seed, h=90, w=400):
    """a crop that is no multiple of the target: a white margin (cropped away), bars of many sizes and colours: both the first and the second resize run"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 250, np.uint8)
    for _ in range(40):
        y, x = int(rng.integers(8, h - 16)), int(rng.integers(12, w - 40))
        img[y:y + int(rng.integers(2, 9)), x:x + int(rng.integers(3, 30))] = (int(rng.integers(0, 120)), int(rng.integers(0, 120)), int(rng.integers(0, 120)))
    return img


def test_predictor_on_crops_that_really_resize(setup):
    """RGB crops of 90 x 400 and 300 x 120: the margin crop cuts the white border, the first Triangle resize (`k_resize_triangle`) brings the smaller side to 64, the
    400-wide one exceeds 128 and takes the second resize, the 300-high one exceeds 64 and takes it too; both land centred on white.  The reference path runs on the
    predictor's own tensor (f64 encoder, f64 head, the shared decode), with and without stop_at_eos; the tensor's geometry is asserted from the sizes the CPU tests pin."""
    model, info, path, crops, t, enc, ref_tokens, eos = setup
    imgs = [_wide_crop(5), np.ascontiguousarray(_wide_crop(6, 120, 300).transpose(1, 0, 2))]
    got = {}
    for stop in (False, True):
        p = formula.FormulaRecognitionPredictor(model, path, formula.FormulaRecognitionConfig(batch_size=2), stop_at_eos=stop, model_type="unimernet")
        try:
            pre = p.preprocessor
            x = pre.preprocess_batch(imgs)
            assert x.shape == (2, 1, 64, 128)
            border = pre.border_value()
            for i, img in enumerate(imgs):
                cx, cy, cw, ch = pre.crop_rect(img)
                assert (cw, ch) != (img.shape[1], img.shape[0])                            # the margin crop did cut
                first, second = pre.resized_sizes(cw, ch)
                assert second is not None and first != (cw, ch)                            # both resizes run
                fw, fh = second
                left, top = (128 - fw) // 2, (64 - fh) // 2
                inside = x[i, 0, top:top + fh, left:left + fw]
                white = np.float32((np.float32(np.float32(0.299 * 255) + np.float32(0.587 * 255)) + np.float32(0.114 * 255)) / np.float32(255.0))
                outside = np.ones((64, 128), bool)
                outside[top:top + fh, left:left + fw] = False
                assert np.all(x[i, 0][outside] == (white - pre.mean[0]) / pre.std[0]) and float(inside.min()) < 0.0 and np.unique(inside).size > 8, (i, fw, fh)
            mem = unimernet_encoder_reference(info["encoder"], x, "float64")
            ref = formula_reference_bundle(info["weights"], mem, M)
            print(f"resizing crops: gap {ref['gap']:.2e} tol {ref['tol']:.2e} tokens {ref['tokens'].tolist()}")
            assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for these crops", ref["gap"], ref["tol"])
            want = p.decode(ref["tokens"])
            out = p.predict(imgs)
            print(f"stop_at_eos = {stop}: {out.formulas}")
            assert out.formulas == want, (out.formulas, want)
            got[stop] = out.formulas
        finally:
            p.close()
    assert got[True] == got[False]
