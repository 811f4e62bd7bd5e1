"""The vision reference (synth/vision_reference.py) against an outside implementation: `transformers`' PaddleOCR-VL vision tower and projector
(models/paddleocr_vl: PaddleOCRVisionTransformer, apply_rotary_pos_emb_vision, PaddleOCRProjector), loaded with the cases' weights under the checkpoint's own names
and run in f64 on the CPU.  Skipped where the package is not importable.

Bound: that implementation forms its rotary angles from an f32 `inv_freq` and rotates q and k in f32 whatever the model's dtype (`q.float()`), so its features carry f32
rounding: the bound is the case's own tol = max(16 noise, 2^-19), noise = max |f32 - f64| of the reference.  The projector has no such step: 1e-12.

One disagreement is pinned, not hidden: that implementation resamples the position table with align_corners = True, the reference implementation this project follows
(and this library) with align_corners = False.  With its switch set to False it agrees with `vision_forward`; as it ships it agrees with the reference's
"align_corners=True" fault variant."""
import warnings

import numpy as np
import pytest
import torch

from oar_ocr_amd.synth import vision_reference as vr

pytest.importorskip("transformers")
M = pytest.importorskip("transformers.models.paddleocr_vl.modeling_paddleocr_vl")
Cf = pytest.importorskip("transformers.models.paddleocr_vl.configuration_paddleocr_vl")

CASES = ("P", "Q", "R", "S", "K")
_cache = {}


def _setup(name):
    if name not in _cache:
        case = vr.ENCODER_CASES[name]
        w, px = vr.make_vision(case), vr.make_pixels(case)
        vcfg = Cf.PaddleOCRVisionConfig(hidden_size=case.D, intermediate_size=case.F, num_hidden_layers=case.L, num_attention_heads=case.heads, num_channels=3,
                                        image_size=case.G * case.patch, patch_size=case.patch, hidden_act=case.act, layer_norm_eps=case.eps, spatial_merge_size=case.merge,
                                        attention_dropout=0.0)
        vcfg._attn_implementation = "eager"
        _cache[name] = (case, w, px, vcfg, vr.vision_bundle(case, w, px))
    return _cache[name]


def _f64(w, prefix):
    return {k[len(prefix):]: torch.from_numpy(v).double() for k, v in w.items() if k.startswith(prefix)}


def test_rotation_is_theirs():
    """apply_rotary_pos_emb_vision with cos / sin = the reference's tables repeated over both halves (their `repeat(1, 2)`) against vr.rotate: rotate_half, not interleaved,
    rows in the first quarter of the head and columns in the second"""
    rng = np.random.default_rng(3)
    for dh, grid in ((8, (3, 5)), (40, (2, 7)), (72, (6, 10))):
        T = grid[0] * grid[1]
        cos, sin = vr.rotary_tables([grid], dh, dtype="float32")
        q, k = rng.standard_normal((T, 2, dh)).astype(np.float32), rng.standard_normal((T, 2, dh)).astype(np.float32)
        tq, tk = M.apply_rotary_pos_emb_vision(torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(np.tile(cos, 2)), torch.from_numpy(np.tile(sin, 2)))
        for mine, theirs in ((vr.rotate(q, cos, sin), tq), (vr.rotate(k, cos, sin), tk)):
            assert np.abs(mine - theirs.numpy()).max() <= 4 * 2.0 ** -23 * np.abs(mine).max(), dh      # the same three f32 operations, perhaps fused differently
    # and their angles: (row, col) positions times 1 / theta^(2 j / (dh / 2)), j < dh / 4
    rot = M.PaddleOCRVisionRotaryEmbedding(72 // 2)
    pos = torch.tensor([[r, c] for r in range(6) for c in range(10)])
    ang = rot(pos).numpy()
    c64, s64 = vr.rotary_tables([(6, 10)], 72, dtype="float64")
    assert ang.shape == (60, 36) and np.abs(np.cos(ang) - c64).max() <= 1e-5 and np.abs(np.sin(ang) - s64).max() <= 1e-5


@pytest.mark.parametrize("name", CASES)
def test_vision_tower_and_projector_are_theirs(name):
    case, w, px, vcfg, ref = _setup(name)
    model = M.PaddleOCRVisionTransformer(vcfg).double().eval()
    res = model.load_state_dict(_f64(w, "visual.vision_model."), strict=False)
    assert not res.missing_keys and not res.unexpected_keys, res                     # the checkpoint's names are the module's names
    grid = torch.tensor([[1, h, wd] for h, wd in case.grids])
    pv = torch.from_numpy(px).double().reshape(1, case.tokens, 3, case.patch, case.patch)
    wrong, _ = vr.vision_forward(case, w, px, "float64", fault="align_corners=True")
    out = {}
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert model.embeddings.interpolation_align_corners is True                  # as shipped
        for ac in (True, False):
            model.embeddings.interpolation_align_corners = ac
            out[ac] = model(pixel_values=pv, grid_thw=grid).last_hidden_state.reshape(case.tokens, case.D).numpy()
    r = ref["feat"]
    err, err_shipped = float(np.abs(out[False] - r["f64"]).max()), float(np.abs(out[True] - wrong).max())
    print(f"case {name}: transformers (align_corners False) differs from the reference by {err:.2e}, as shipped from the align_corners=True variant by {err_shipped:.2e} | tol {r['tol']:.2e}")
    assert err <= r["tol"] and err_shipped <= r["tol"], (err, err_shipped, r["tol"])
    if any((h, wd) != (case.G, case.G) for h, wd in case.grids):
        assert float(np.abs(out[True] - r["f64"]).max()) > 100 * r["tol"]            # the two resamplings are far apart on these cases
    cfg = Cf.PaddleOCRVLConfig(vision_config=vcfg.to_dict(), text_config=dict(hidden_size=case.text_hidden))
    proj = M.PaddleOCRProjector(cfg).double().eval()
    proj.load_state_dict(_f64(w, "mlp_AR."))                                         # strict
    with torch.no_grad():
        emb = proj(torch.from_numpy(r["f64"]), grid).numpy()
    perr = float(np.abs(emb - ref["emb"]["f64"]).max())
    print(f"case {name}: projector differs by {perr:.2e}")
    assert emb.shape == ref["emb"]["f64"].shape and perr <= 1e-12
