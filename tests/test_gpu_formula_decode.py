"""The PP-FormulaNet-style decode head on the GPU: an ONNX Loop of M greedy steps of a pre-norm transformer decoder with a key / value cache, which the
engine replaces by ONE FormulaDecode operator -- per step and chunk of 16 images a fixed chain of 8 Ld + 2 short launches (csrc/formula_decode.hip).

Reference: the same recurrence in torch on the CPU, in f64 and in f32 (synth/formula_reference.py).  The weights follow synth.models.formula_weights.
Each case measures the f32-against-f64 `noise` of the logits itself and asserts, in this order:
  1. on the reference alone: every step's top-1 / top-2 logit gap >= 8 tol, tol = max(16 noise, 2^-19) -- the greedy path never comes close enough
     to a fork for an error of size tol to change it (the seeds are chosen so that this holds; no step is excluded)
  2. the GPU's token_ids equal the f64 tokens at every position
  3. max |logits - f64| <= tol
The measured figures are printed (pytest -s) and recorded in DESIGN 4.32."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_head_reference, formula_reference_bundle

pytestmark = pytest.mark.gpu

#          D   nh    F     V  Ld   S   M   B
SHAPES = [(24, 3, 40, 37, 1, 9, 12, 5),              # nothing a multiple of 16, dh = 8
          (40, 5, 72, 61, 2, 37, 40, 3),             # two layers, odd S
          (64, 4, 128, 300, 2, 50, 70, 2),           # the cache passes 64 entries; V spans several workgroups of the arg max
          (24, 3, 40, 37, 1, 9, 6, 17),              # 17 images: two chunks, the second with one row
          (24, 3, 40, 37, 1, 9, 1, 1),               # a single step
          (384, 16, 1536, 4099, 2, 144, 48, 2)]      # a PP-FormulaNet-S-shaped layer; V is prime
SEED = 0
LAUNCHES_PER_LAYER, LAUNCHES_PER_STEP = 8, 2         # 8 Ld + 2 launches per step and chunk


def _memory(shape, seed=SEED):
    D, nh, F, V, Ld, S, M, B = shape
    return np.random.default_rng(1000 + seed).standard_normal((B, S, D)).astype(np.float32)


def _run(model, x):
    eng = api.OrtInfer(model)
    try:
        return dict(eng.infer(x))
    finally:
        eng.close()


def _build(shape, **kw):
    D, nh, F, V, Ld, S, M, B = shape
    return models.build_formulanet(D=D, nh=nh, F=F, V=V, Ld=Ld, M=M, seed=SEED, head_only=True, with_logits=True, **kw)


_cache = {}


def _case(shape):
    """reference bundle and GPU outputs of one shape: computed once, never modified"""
    if shape not in _cache:
        model, info = _build(shape)
        mem = _memory(shape)
        _cache[shape] = (formula_reference_bundle(info["weights"], mem, shape[6]), _run(model, mem))
    return _cache[shape]


def _check_against(ref, outs, shape, label):
    D, nh, F, V, Ld, S, M, B = shape
    assert outs["token_ids"].shape == (B, M) and outs["token_ids"].dtype == np.int64 and outs["logits"].shape == (B, M, V)
    tol = ref["tol"]
    err = float(np.abs(outs["logits"].astype(np.float64) - ref["logits"]).max())
    print(f"{label}: noise {ref['noise']:.2e} | tol {tol:.2e} | gap {ref['gap']:.2e} token changes {ref['changes']} | gpu err logits {err:.2e}")
    assert ref["gap"] >= 8 * tol, ("the reference itself is ill conditioned for this seed", ref["gap"], tol)
    assert np.array_equal(outs["token_ids"], ref["tokens"]), ("tokens differ at (image, step)", np.argwhere(outs["token_ids"] != ref["tokens"])[:4])
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d_nh%d_F%d_V%d_Ld%d_S%d_M%d_B%d" % s)
def test_decode_matches_the_f64_recurrence(shape):
    ref, outs = _case(shape)
    _check_against(ref, outs, shape, str(shape))


def test_equal_logits_go_to_the_lowest_index():
    """two identical rows of W_lm / b_lm, scaled so that they win most steps, in different workgroups of the arg max (8 rows each at V = 300): the higher index is
    never emitted (ONNX ArgMax, select_last_index = 0)"""
    shape = SHAPES[2]
    D, nh, F, V, Ld, S, M, B = shape
    w = models.formula_weights(D, nh, F, V, Ld, M + 2, SEED)
    lo, hi = 2, V - 1
    w["w_lm"][lo] *= np.float32(3.0)
    w["b_lm"][lo] = np.float32(10.0)
    w["w_lm"][hi], w["b_lm"][hi] = w["w_lm"][lo], w["b_lm"][lo]
    model, _ = _build(shape, weights=w)
    mem = _memory(shape)
    ref = formula_head_reference(w, mem, M, "float64")
    assert np.array_equal(ref["logits"][..., lo], ref["logits"][..., hi]) and (ref["tokens"] == lo).sum() >= M     # the tie really decides steps (71 of 140)
    outs = _run(model, mem)
    assert np.array_equal(outs["logits"][..., lo], outs["logits"][..., hi])
    assert not np.any(outs["token_ids"] == hi)
    assert np.array_equal(outs["token_ids"], ref["tokens"])


@pytest.mark.parametrize("q_scale", ["after", "before"])
def test_matmul_spelling_with_outer_weights_fuses_too(q_scale):
    """MatMul + Add with the weights in the outer scope, commuted operands, Reshape targets with -1, and the query scale on either side of the bias Add"""
    shape = SHAPES[1]
    model, info = _build(shape, spelling="matmul", q_scale=q_scale)
    # (x W^T) * s + b is other math than (x W^T + b) * s: the reference follows the weights record of the graph that was written
    ref = _case(shape)[0] if q_scale == "after" else formula_reference_bundle(info["weights"], _memory(shape), shape[6])
    _check_against(ref, _run(model, _memory(shape)), shape, f"matmul+add, scale {q_scale} the bias " + str(shape))


def test_folded_query_scale():
    """no Mul at all: Wq / bq arrive scaled, and the reference runs on the weights the graph holds"""
    shape = SHAPES[0]
    model, info = _build(shape, q_scale="folded")
    assert info["weights"]["q_scale"] == 1.0
    mem = _memory(shape)
    _check_against(formula_reference_bundle(info["weights"], mem, shape[6]), _run(model, mem), shape, "folded scale " + str(shape))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=["one_chunk", "two_chunks"])
def test_launch_count_and_cost(shape):
    D, nh, F, V, Ld, S, M, B = shape
    model, _ = _build(shape)
    eng = api.OrtInfer(model, profile=True)
    try:
        mem = _memory(shape)
        eng.infer(mem)                       # plan
        per_infer = M * ((B + 15) // 16) * (LAUNCHES_PER_LAYER * Ld + LAUNCHES_PER_STEP)
        for runs in (1, 2):                  # (the second infer of a plan may replay it as a captured graph: the same launches)
            api.prof_reset()
            api.prof_enable(True)
            for _ in range(runs):
                eng.infer(mem)
            snap = {e["name"]: e for e in api.prof_snapshot()}
            assert "formula_decode" in snap and snap["formula_decode"]["launches"] == runs * per_infer, (snap.get("formula_decode"), per_infer)
        fl, by, nk = eng.cost(list(mem.shape))
        step_macs = Ld * (6 * D * D + 2 * F * D + 2 * S * D) + V * D                     # per image; the self attention comes on top
        step_weights = Ld * (6 * D * D + 2 * F * D) + V * D                              # floats every step streams, per chunk
        assert fl >= 2.0 * step_macs * M * B and by >= 4.0 * step_weights * M * ((B + 15) // 16)
    finally:
        api.prof_enable(False)
        eng.close()


def _refused(model):
    with pytest.raises(api.OCRError) as ex:
        api.OrtInfer(model)
    assert ex.value.code == api.OAR_UNSUPPORTED_OP and "Loop" in str(ex.value), str(ex.value)
    return str(ex.value)


def test_other_bodies_are_refused_by_name():
    small = dict(D=24, nh=3, F=40, V=37, Ld=1, M=4, head_only=True)
    assert "Relu" in _refused(models.build_formulanet(act="Relu", **small)[0])
    assert "initial cache" in _refused(models.build_formulanet(initial_cache="one", **small)[0])
    assert "M = 5000" in _refused(models.build_formulanet(**dict(small, M=5000))[0])
    assert "final cache" in _refused(models.build_formulanet(read_final_cache=True, **small)[0])


def test_backbone_and_head():
    """the whole graph on a 64 x 64 image: the GPU's tokens equal the f64 head run on the GPU's own `memory` (a declared output), under the same gap rule"""
    D, nh, F, V, Ld, M, B = 40, 5, 72, 61, 2, 24, 3
    model, info = models.build_formulanet(D=D, nh=nh, F=F, V=V, Ld=Ld, M=M, seed=SEED, image_shape=(64, 64))
    x = np.random.default_rng(7).random((B, 1, 64, 64)).astype(np.float32)
    outs = _run(model, x)
    assert outs["memory"].shape == (B, 64, D) and outs["token_ids"].shape == (B, M) and outs["token_ids"].dtype == np.int64
    ref = formula_reference_bundle(info["weights"], outs["memory"], M)
    print(f"backbone + head: noise {ref['noise']:.2e} | tol {ref['tol']:.2e} | gap {ref['gap']:.2e} token changes {ref['changes']}")
    assert ref["gap"] >= 8 * ref["tol"], ("the reference itself is ill conditioned for this seed", ref["gap"], ref["tol"])
    assert np.array_equal(outs["token_ids"], ref["tokens"]), ("tokens differ at (image, step)", np.argwhere(outs["token_ids"] != ref["tokens"])[:4])
