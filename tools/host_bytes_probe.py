"""One SHA-256 per line over what the host entries return, for comparing two builds of the library byte for byte.

Run it once per tree, one process each, and diff the two lists: the kernels are deterministic, so a line that differs is a changed launch or a changed copy,
not noise.  It uses only public names of oar_ocr_amd: the two vision encoders on the seeded tiny towers of the GPU tests (both kinds of the Qwen tower), one
images-to-tokens call of each composite model with logits, and every direct kernel wrapper once at a small ragged shape."""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api, vl  # noqa: E402
from oar_ocr_amd.synth import qwen_vision_reference as qr  # noqa: E402
from oar_ocr_amd.synth import vision_reference as vr  # noqa: E402


def show(label, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f"{h.hexdigest()}  {label}", flush=True)


def towers():
    for name in ("R", "P"):
        case = vr.ENCODER_CASES[name]
        cfg = vl.VisionConfig(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, intermediate_size=case.F, patch_size=case.patch,
                              text_hidden=case.text_hidden, pos_grid=case.G, spatial_merge_size=case.merge, layer_norm_eps=case.eps, hidden_act=case.act,
                              max_tokens=case.tokens, max_images=len(case.grids))
        with vl.VisionEncoder.from_state_dict(cfg, vr.make_vision(case)) as enc:
            emb, feat = enc.encode(vr.make_pixels(case), case.grids, return_features=True)
            show(f"VisionEncoder {name} embeds", emb)
            show(f"VisionEncoder {name} features", feat)
            show(f"VisionEncoder {name} cost", np.asarray(enc.cost(case.grids), np.float64))
    for name in ("B2", "X5", "W5"):
        case = qr.QVIS_CASES[name]
        cfg = vl.QwenVisionConfig(kind=case.kind, embed_dim=case.D, depth=case.L, num_heads=case.heads, intermediate_size=case.F, patch_size=case.patch,
                                  out_hidden_size=case.out_hidden, temporal_patch_size=case.temporal, in_channels=case.channels, spatial_merge_size=case.merge,
                                  hidden_act=case.act, window_size=case.window_size, fullatt_block_indexes=list(case.fullatt), max_tokens=case.tokens,
                                  max_images=len(case.grids))
        with vl.QwenVisionEncoder.from_state_dict(cfg, qr.make_qvision(case)) as enc:
            emb, feat = enc.encode(qr.make_qpixels(case), case.grids, return_features=True)
            show(f"QwenVisionEncoder {name} embeds", emb)
            show(f"QwenVisionEncoder {name} features", feat)
            show(f"QwenVisionEncoder {name} cost", np.asarray(enc.cost(case.grids), np.float64))


def _lm_json(lc, image, start):
    return dict(hidden_size=lc.D, num_hidden_layers=lc.L, num_attention_heads=lc.heads, num_key_value_heads=lc.kv_heads, head_dim=lc.head_dim, intermediate_size=lc.F,
                vocab_size=lc.vocab, rms_norm_eps=lc.eps, rope_theta=lc.theta, rope_scaling=dict(mrope_section=list(lc.mrope_section)), tie_word_embeddings=lc.tie,
                image_token_id=image, vision_start_token_id=start)


def composites():
    r = vr.composite_reference()
    vc = r["vis_case"]
    cfg = _lm_json(r["lm_case"], vr.PA_IDS["image"], vr.PA_IDS["start"])
    cfg["vision_config"] = dict(hidden_size=vc.D, num_hidden_layers=vc.L, num_attention_heads=vc.heads, intermediate_size=vc.F, patch_size=vc.patch, image_size=vc.G * vc.patch,
                                spatial_merge_size=vc.merge, layer_norm_eps=vc.eps, hidden_act=vc.act)
    preproc = dict(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096, rescale_factor=1.0 / 255.0, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
    with vl.PaddleOCRVL.from_state_dict(cfg, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=2), vision_overrides=dict(max_tokens=64, max_images=2)) as m:
        out = m.generate_tokens(r["images"], vr.PA_IDS["prefix"], vr.PA_IDS["suffix"], max_new_tokens=vr.PA_STEPS, return_logits=True)
        show("PaddleOCRVL tokens", out.tokens)
        show("PaddleOCRVL logits", out.logits)
    for name in qr.COMPOSITES:
        r = qr.composite_reference(name)
        vc, ids = r["vis_case"], qr.COMPOSITE_IDS
        vision = dict(depth=vc.L, num_heads=vc.heads, in_chans=vc.channels, patch_size=vc.patch, spatial_merge_size=vc.merge, temporal_patch_size=vc.temporal, hidden_act=vc.act)
        if vc.kind == "qwen2_5":
            vision.update(hidden_size=vc.D, out_hidden_size=vc.out_hidden, intermediate_size=vc.F, window_size=vc.window_size, fullatt_block_indexes=list(vc.fullatt))
        else:
            vision.update(embed_dim=vc.D, hidden_size=vc.out_hidden, mlp_ratio=vc.F / vc.D)
        cfg = _lm_json(r["lm_case"], ids["image"], ids["start"])
        cfg["vision_config"] = vision
        preproc = dict(patch_size=vc.patch, merge_size=vc.merge, temporal_patch_size=vc.temporal, min_pixels=16, max_pixels=4096, rescale_factor=1.0 / 255.0,
                       image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
        with vl.QwenVL.from_state_dict(cfg, preproc, r["weights"], lm_overrides=dict(max_positions=64, max_sequences=3), vision_overrides=dict(max_tokens=160, max_images=3)) as m:
            out = m.generate_tokens(r["images"], ids["prefix"], ids["suffix"], max_new_tokens=qr.COMPOSITE_STEPS, return_logits=True)
            show(f"QwenVL {name} tokens", out.tokens)
            show(f"QwenVL {name} logits", out.logits)


def kernels():
    g = np.random.default_rng(52)
    f = lambda *shape: g.standard_normal(shape).astype(np.float32)   # noqa: E731
    heads, dh, lens = 2, 8, (33, 5)
    D, T = heads * dh, sum(lens)
    pad = np.full(T * D + 8, 7.0, np.float32)          # the output starts 4 floats in: what lies around it must come back untouched
    buf = f(3 * 40 * 24)                               # q, k, v views of stride 24 in one buffer
    show("k_mha_attention", api.k_mha_attention(buf, 0, 960, 1920, 24, 24, 24, 1, 33, 38, heads, dh, dh ** -0.5, False, pad[:33 * D + 8], 4))
    ang = f(T, dh // 2)
    show("k_vis_attention", api.k_vis_attention(f(T * 52), 4, 52, lens, heads, dh, np.cos(ang), np.sin(ang), pad, 4))
    show("k_vis_pos_embed", api.k_vis_pos_embed(f(16, 8), 4, [(2, 3), (5, 1)], np.full(11 * 8 + 8, 7.0, np.float32), 4))
    show("k_add_layernorm", api.k_add_layernorm(f(3, 8), f(3, 8), f(8), f(8), 1e-5, True, np.full(60, 7.0, np.float32), 5, 31))
    show("k_add_layernorm no affine", api.k_add_layernorm(f(6, 8), f(3, 8), None, None, 1e-5, False, np.full(56, 7.0, np.float32), 4))
    show("k_relpos_attention", api.k_relpos_attention(f(15 * 3 * D), 1, 3, 5, 0, heads, dh, f(3 * dh * 3), f(5 * dh * 5), f(3 * D), dh ** -0.5, True, np.full(15 * D + 8, 7.0, np.float32), 4))
    show("k_lm_gemm f32", api.k_lm_gemm(f(3, 8), f(5, 8), np.full(23, 7.0, np.float32), 4))
    show("k_lm_gemm bf16", api.k_lm_gemm(f(3, 8), (f(5, 8).view(np.uint32) >> 16).astype(np.uint16), np.full(23, 7.0, np.float32), 4))
    kc, vc = f(2, 1, 40, dh), f(2, 1, 40, dh)
    show("k_lm_prefill_attention", api.k_lm_prefill_attention(f(T, D), kc, vc, [0, 2], lens, heads, pad, 4))
    for split in (0, 64):
        show(f"k_lm_decode_attention split_keys {split}", api.k_lm_decode_attention(f(3, D), kc, vc, [0, 1, 0], [32, 4, 0], heads, np.full(3 * D + 8, 7.0, np.float32), 4, split_keys=split))
    show("k_qvis_rmsnorm", vl.k_qvis_rmsnorm(f(3, 8), f(8), 1e-6, np.full(32, 7.0, np.float32), 4))
    show("k_qvis_row_gather", vl.k_qvis_row_gather(f(5, 8), [4, 0, 4], np.full(32, 7.0, np.float32), 4))
    img = g.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    show("k_normalize", api.k_normalize(img, [0.5, 0.25, 2.0], [0.1, -0.2, 0.3]))
    show("k_resize_triangle", api.k_resize_triangle(img, 5, 11))
    show("k_resize_filter", api.k_resize_filter(img, 5, 11, "catmullrom"))
    show("k_rotate_rgb", api.k_rotate_rgb(img, 1))
    show("k_bgr_planes_to_rgb", api.k_bgr_planes_to_rgb(g.random((3, 7, 9), dtype=np.float32)))
    pred = g.random((9, 13), dtype=np.float32)
    show("k_threshold", api.k_threshold(pred, 0.4))
    show("k_dilate", api.k_dilate((pred > 0.7).astype(np.uint8)))
    boxes = np.asarray([[1, 1, 7, 1, 7, 5, 1, 5], [3, 2, 11, 3, 10, 8, 2, 7]], np.float32)
    show("k_box_scores", api.k_box_scores(pred, boxes))
    show("k_unclip", *api.k_unclip(boxes, 1.5))
    show("k_ctc_argmax", *api.k_ctc_argmax(g.random((5, 11), dtype=np.float32)))


if __name__ == "__main__":
    print(api.version(), flush=True)
    kernels()
    towers()
    composites()
