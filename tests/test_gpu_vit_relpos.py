"""ViT encoder attention with the decomposed relative-position bias on the GPU (csrc/relpos_attention.hip): the attention of a SAM / Vary ViT
block -- global or in padded windows, with the query-dependent bias q . Rh[qy, ky] + q . Rw[qx, kx] -- is ONE RelPosAttention launch; the pad, partition,
reverse, crop and the whole score / bias subgraph leave the graph.  Graphs: synth.models.build_vit_block, build_vary_vit and build_formulanet(encoder="vit").

Reference: the same block in torch on the CPU, in f64 and f32 (synth/vit_reference.py, written from the formulas); noise = max |f32 - f64|, tol =
max(16 noise, 2^-19).  tests/test_vit_relpos_cpu.py shows that a dropped rw term, swapped tables, a rel term from the scaled q, masked pad keys and zero
pad keys each move these outputs by more than 100 tol.
Per case: exactly one launch of class relpos_attention with the pass on, none with OAR_FUSE_RELPOS_ATTENTION=0, both outputs within tol of f64, fewer
launches in all than op by op, and two fused runs byte-identical."""
import json

import numpy as np
import pytest

from oar_ocr_amd import api, formula
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_reference_bundle
from oar_ocr_amd.synth.vit_reference import reference_bundle, vary_vit_reference, vit_block_reference

pytestmark = pytest.mark.gpu

#          B   H   W nh  dh  ws
SHAPES = [(1, 5, 7, 2, 8, 0),          # global; key tail inside the first block; H != W
          (2, 9, 15, 1, 64, 0),        # 135 tokens: more than one query tile and more than one key block, batch stride, full head size
          (1, 10, 13, 3, 16, 7),       # padded on both axes, 4 windows
          (1, 8, 8, 2, 16, 4),         # aligned windows, no pad
          (1, 16, 16, 1, 64, 14),      # the -L window: N = 196, pad 16 -> 28
          (1, 48, 48, 1, 64, 0)]       # the -L token count, 2304 keys, one head
IDS = ["B%d_H%d_W%d_nh%d_dh%d_ws%d" % s for s in SHAPES]

_cache = {}


def _case(shape, scale, **kw):
    """model, feeds, reference bundle: computed once, never modified"""
    key = (shape, scale, tuple(sorted(kw.items())))
    if key not in _cache:
        B, H, W, nh, dh, ws = shape
        model, info = models.build_vit_block(H, W, nh * dh, nh, ws, seed=3, scale=scale, **kw)
        x = np.random.default_rng(11).standard_normal((B, H * W, nh * dh)).astype(np.float32)
        feeds = [("x", x), ("rhT", info["rhT"])] if "rhT" in info else x                              # (a list of (name, array) pairs binds by name)
        _cache[key] = (model, feeds, reference_bundle(vit_block_reference, info, x))
    return _cache[key]


def _run(model, feeds, monkeypatch, fuse):
    """-> (y, launches of class relpos_attention in one infer, the profile)"""
    monkeypatch.setenv("OAR_FUSE_RELPOS_ATTENTION", fuse)          # (read when the graph is loaded; set either way, so the test does not depend on the default)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        y = dict(eng.infer(feeds))["y"]
        snap = {e["name"]: e for e in api.prof_snapshot()}
        return y, snap.get("relpos_attention", {}).get("launches", 0), snap
    finally:
        api.prof_enable(False)
        eng.close()


def _launches(snap):
    return sum(e["launches"] for e in snap.values())


@pytest.mark.parametrize("scale", ["pre", "post"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_launch_fewer_launches_and_both_routes_match_f64(shape, scale, monkeypatch):
    model, feeds, ref = _case(shape, scale)
    fused, n_fused, snap = _run(model, feeds, monkeypatch, "1")
    again, _, _ = _run(model, feeds, monkeypatch, "1")
    plain, n_plain, snap0 = _run(model, feeds, monkeypatch, "0")
    e1 = float(np.abs(fused.astype(np.float64) - ref["f64"]).max())
    e0 = float(np.abs(plain.astype(np.float64) - ref["f64"]).max())
    print(f"{shape} {scale}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} | fused err {e1:.2e} ({_launches(snap)} launches) | op-by-op err {e0:.2e} ({_launches(snap0)} launches)")
    assert n_fused == 1, sorted((k, v["launches"]) for k, v in snap.items())
    assert n_plain == 0, sorted((k, v["launches"]) for k, v in snap0.items())
    assert fused.shape == ref["f64"].shape and e1 <= ref["tol"], (e1, ref["tol"])
    assert e0 <= ref["tol"], (e0, ref["tol"])
    assert _launches(snap) < _launches(snap0), (_launches(snap), _launches(snap0))
    assert np.array_equal(fused, again)


FALLBACKS = {"dh_80": ((1, 6, 6, 1, 80, 0), {}),                                       # a head size the kernel does not take
             "rhT_as_input": ((1, 10, 13, 3, 16, 7), dict(rh_input=True)),             # a table that is no constant
             "rel_from_scaled_q": ((1, 10, 13, 3, 16, 7), dict(rel_from="scaled"))}    # the rel term taken from another tensor


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_near_misses_are_never_fused_wrongly(name, monkeypatch):
    """with the pass on: within tol of the f64 reference of what the graph says; the first two show no relpos_attention launch, the third is either fused with
    the right values or left op by op"""
    shape, kw = FALLBACKS[name]
    model, feeds, ref = _case(shape, "pre", **kw)
    y, n, snap = _run(model, feeds, monkeypatch, "1")
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max())
    print(f"fall-back {name}: err {err:.2e} tol {ref['tol']:.2e} ({_launches(snap)} launches, {n} of relpos_attention)")
    if name != "rel_from_scaled_q":
        assert n == 0, sorted((k, v["launches"]) for k, v in snap.items())
    assert y.shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])


def test_whole_block_fuses_too(monkeypatch):
    """the whole block (LN2 and the MLP behind the attention) on the padded case: one launch, within tol"""
    model, feeds, ref = _case(SHAPES[2], "pre", whole=True)
    y, n, snap = _run(model, feeds, monkeypatch, "1")
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max())
    print(f"whole block: err {err:.2e} tol {ref['tol']:.2e} noise {ref['noise']:.2e}")
    assert n == 1 and err <= ref["tol"], (n, err, ref["tol"])


# ------------------------------------------------------------------------------------------------ the encoder, and the predictor on it
ENC = dict(image_shape=(64, 48), V=61, M=24, seed=1, encoder="vit")                                # 4 x 3 tokens, ws = 2 (W padded to 4), one global block
BLOCKS = 2


def _crop(seed):
    """a 48 x 64 crop (width x height) with ink in two opposite corners"""
    rng = np.random.default_rng(seed)
    img = np.full((64, 48, 3), 245, np.uint8)
    img[0, 0] = img[63, 47] = 0
    for _ in range(10):
        y, x = int(rng.integers(4, 52)), int(rng.integers(4, 34))
        img[y:y + int(rng.integers(2, 6)), x:x + int(rng.integers(4, 10))] = (int(rng.integers(0, 90)), int(rng.integers(0, 90)), int(rng.integers(0, 90)))
    return img


def test_vary_vit_encoder_memory(monkeypatch):
    """build_vary_vit at a 64 x 48 image, B = 2: `memory` against the f64 encoder within the network budget 1e-3 max(1, max |ref|) (as
    tests/test_gpu_unimernet.py uses it for build_unimernet); one RelPosAttention launch per block"""
    monkeypatch.setenv("OAR_FUSE_RELPOS_ATTENTION", "1")
    model, info = models.build_vary_vit(image_shape=(64, 48), seed=1)
    x = np.random.default_rng(5).standard_normal((2, 1, 64, 48)).astype(np.float32)
    enc = reference_bundle(vary_vit_reference, info["encoder"], x)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        mem = dict(eng.infer(x))["memory"]
        snap = {e["name"]: e for e in api.prof_snapshot()}
    finally:
        api.prof_enable(False)
        eng.close()
    err = float(np.abs(mem.astype(np.float64) - enc["f64"]).max())
    budget = 1e-3 * max(1.0, float(np.abs(enc["f64"]).max()))
    print(f"memory: max |gpu - f64| {err:.2e} | budget {budget:.2e} | torch f32 noise {enc['noise']:.2e} tol {enc['tol']:.2e} | max |ref| {np.abs(enc['f64']).max():.2f} | {_launches(snap)} launches")
    assert snap.get("relpos_attention", {}).get("launches") == BLOCKS, sorted((k, v["launches"]) for k, v in snap.items())
    assert mem.shape == (2, info["S"], info["D"]) and err <= budget, (err, budget)


def test_predictor_on_the_vit_encoder(tmp_path, monkeypatch):
    """FormulaRecognitionPredictor on build_formulanet(encoder="vit") returns the strings the f64 path yields on the preprocessor's own tensor (f64 encoder,
    f64 head, the shared decode), under the gap rule of tests/test_gpu_unimernet.py"""
    monkeypatch.setenv("OAR_FUSE_RELPOS_ATTENTION", "1")
    model, info = models.build_formulanet(**ENC)
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(models.formula_tokenizer_spec(ENC["V"])), encoding="utf-8")
    crops = [_crop(1), _crop(2), _crop(3)]
    p = formula.FormulaRecognitionPredictor(model, path, formula.FormulaRecognitionConfig(batch_size=2))
    try:
        t = p.preprocessor.preprocess_batch(crops)
        assert t.shape == (3, 1, 64, 48), t.shape                                                  # the target size comes from the model's static input shape
        mem = vary_vit_reference(info["encoder"], t, "float64")
        ref = formula_reference_bundle(info["weights"], mem, ENC["M"])
        print(f"head from the f64 memory: tol {ref['tol']:.2e} | gap {ref['gap']:.2e} | tokens {ref['tokens'].tolist()}")
        assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for these crops", ref["gap"], ref["tol"])
        want = p.decode(ref["tokens"])
        out = p.predict(crops)
        print(out.formulas)
        assert out.formulas == want and all(want), (out.formulas, want)
    finally:
        p.close()
