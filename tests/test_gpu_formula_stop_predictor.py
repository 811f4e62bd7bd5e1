"""`FormulaRecognitionPredictor(stop_at_eos=True)`: the decode ends at eos on the device, and `predict` gives the strings it gives without it -- those of the torch
reference (backbone and head, f64) on the preprocessor's own tensor.

The synthetic tokenizer's eos is chosen from the reference: among the ordinary tokens (id >= 4) that every row emits before the last step, the one whose earliest
first occurrence is latest (lowest id among equals), so that every row stops early and no string is empty.  The crops are 64 x 64 with ink in two opposite
corners: the margin crop keeps them whole and the resize is the identity, so the preprocessor's tensor -- and with it the choice -- needs no GPU."""
import json

import numpy as np
import pytest

from oar_ocr_amd import formula
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_memory_reference, formula_reference_bundle

pytestmark = pytest.mark.gpu

D, NH, F, V, LD, M = 40, 5, 72, 61, 2, 24


def _crop(seed):
    rng = np.random.default_rng(seed)
    img = np.full((64, 64, 3), 245, np.uint8)
    img[0, 0] = img[63, 63] = 0
    for _ in range(6):
        y, x = int(rng.integers(4, 52)), int(rng.integers(4, 50))
        img[y:y + int(rng.integers(2, 5)), x:x + int(rng.integers(4, 10))] = int(rng.integers(0, 90))
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
    model, info = models.build_formulanet(D=D, nh=NH, F=F, V=V, Ld=LD, M=M, seed=0, image_shape=(64, 64))
    crops = [_crop(1), _crop(2), _crop(3)]
    t = formula.FormulaPreprocessor(target_size=(64, 64)).preprocess_batch(crops)
    ref = formula_reference_bundle(info["weights"], formula_memory_reference(info["weights"], t, "float64"), M)
    assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for these crops", ref["gap"], ref["tol"])
    tok = ref["tokens"]
    firsts = {e: [int(np.nonzero(r == e)[0][0]) for r in tok] for e in range(4, V) if all(np.any(r[:M - 1] == e) for r in tok)}
    assert firsts, "no token occurs in every row of the reference before the last step: choose other crops"
    eos = min(firsts, key=lambda e: (-min(firsts[e]), e))
    assert eos == 21 and firsts[eos] == [4, 5, 14]            # (what seed 0 and these crops give)
    path = tmp_path_factory.mktemp("formula_stop") / "tokenizer.json"
    path.write_text(json.dumps(_tokenizer_with_eos(eos)), encoding="utf-8")
    return model, path, crops, tok, eos


def test_predict_gives_the_same_strings_with_and_without_the_stop(setup):
    model, path, crops, ref_tokens, eos = setup
    got = {}
    for stop in (True, False):
        p = formula.FormulaRecognitionPredictor(model, path, formula.FormulaRecognitionConfig(batch_size=2), stop_at_eos=stop)
        try:
            assert p.eos_token_id == eos and p.preprocessor.target_size == (64, 64) and p.stop_at_eos is stop
            want = p.decode(ref_tokens)
            out = p.predict(crops)                            # batch_size 2: two infers, the last with one image (first eos at step 14)
            st = p.decode_stats()
            print(f"stop_at_eos = {stop}: {out.formulas} | {st}")
            assert out.formulas == want and all(want), (out.formulas, want)
            assert st.steps_limit == M
            if stop:
                assert st.steps_executed == 15 and st.steps_executed < st.steps_limit, st
            else:
                assert st.steps_executed == st.steps_limit == st.steps_enqueued, st
            got[stop] = out.formulas
        finally:
            p.close()
    assert got[True] == got[False]
