"""Formula recognition end to end on the GPU: `formula.FormulaRecognitionPredictor` (preprocessor -> the synthetic PP-FormulaNet-shaped graph through the engine,
its decode Loop as the FormulaDecode operator -> token filter -> ByteLevel decode -> normalize_latex) against the torch reference of the same graph run on the
preprocessor's own tensor, and `structure.OverallOCR.recognize_formulas` on a synthetic page."""
import json

import numpy as np
import pytest

from oar_ocr_amd import formula, structure
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_memory_reference, formula_reference_bundle

pytestmark = pytest.mark.gpu

D, NH, F, V, LD, M = 40, 5, 72, 61, 2, 24


def _crop(h, w, seed):
    """dark strokes on a light page, with a margin for crop_margin to remove"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w, 3), 245, np.uint8)
    for _ in range(6):
        y, x = int(rng.integers(4, h - 8)), int(rng.integers(4, w - 12))
        img[y:y + int(rng.integers(2, 5)), x:x + int(rng.integers(4, 10))] = int(rng.integers(0, 90))
    return img


@pytest.fixture(scope="module")
def predictor(tmp_path_factory):
    model, info = models.build_formulanet(D=D, nh=NH, F=F, V=V, Ld=LD, M=M, seed=0, image_shape=(64, 64))
    path = tmp_path_factory.mktemp("formula") / "tokenizer.json"
    path.write_text(json.dumps(models.formula_tokenizer_spec(V)), encoding="utf-8")
    p = formula.FormulaRecognitionPredictor(model, path, formula.FormulaRecognitionConfig(batch_size=2))
    yield p, info["weights"]
    p.close()


def _reference_strings(p, w, crops):
    """the torch reference (backbone and head, f64) on the preprocessor's tensor, decoded on the host; the gap rule of test_gpu_formula_decode.py holds for it"""
    t = p.preprocessor.preprocess_batch(crops)
    ref = formula_reference_bundle(w, formula_memory_reference(w, t, "float64"), M)
    assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for these crops", ref["gap"], ref["tol"])
    return p.decode(ref["tokens"])


def test_predictor_matches_the_reference_strings(predictor):
    p, w = predictor
    assert p.preprocessor.target_size == (64, 64) and (p.sos_token_id, p.eos_token_id) == (0, 2)      # the model's static input size; <s> / </s>
    crops = [_crop(40, 90, 1), _crop(70, 50, 2), _crop(64, 64, 3)]                                     # batch_size 2: the last batch has one image
    out = p.predict(crops)
    assert len(out.formulas) == 3 and out.scores == [None, None, None]
    want = _reference_strings(p, w, crops)
    print("formulas:", out.formulas)
    assert out.formulas == want
    assert any(out.formulas), "every formula decoded to nothing: the test shows nothing"


def test_recognize_formulas_on_a_page(predictor):
    p, w = predictor
    page = np.full((200, 300, 3), 250, np.uint8)
    page[20:60, 30:120] = _crop(40, 90, 4)
    page[100:170, 180:230] = _crop(70, 50, 5)
    E = structure.LayoutElement
    elements = [E(structure.from_coords(30, 20, 120, 60), "formula"), E(structure.from_coords(10, 10, 290, 190), "text"),
                E(structure.from_coords(50, 80, 50, 120), "formula"),                                 # degenerate: no width
                E(structure.from_coords(180, 100, 230, 170), "formula_number")]
    s = structure.OverallOCR(None, None, formula_recognizer=p)
    assert s.formula_recognition                                                                     # a recognizer turns the masking on
    got = s.recognize_formulas(page, elements)
    assert [tuple(structure.aabb(r.bbox)) for r in got] == [(30, 20, 120, 60), (180, 100, 230, 170)]
    assert [r.latex for r in got] == _reference_strings(p, w, [page[20:60, 30:120], page[100:170, 180:230]])
    assert all(r.confidence == 0.0 for r in got)
    assert structure.OverallOCR(None, None).recognize_formulas(page, elements) == []                # no recognizer: nothing, as before
