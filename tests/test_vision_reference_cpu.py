"""The reference of the vision encoder's attention (synth/vision_reference.py), host side: it agrees with a second, independent spelling
(complex multiplication for the rotation, torch's scaled_dot_product_attention under a block-diagonal mask) within f64 rounding, its rotary tables give a
hand-worked answer, every wrong reading in its fault list moves the output of at least one case by more than 100 tol, and oar_k_vis_attention answers
every bad argument with its status without a GPU.

Tolerance, as elsewhere in the project: noise = max |f32 - f64| of the reference on the same inputs, tol = max(16 noise, 2^-19)."""
import numpy as np
import pytest
import torch

from oar_ocr_amd import api, build
from oar_ocr_amd.synth import vision_reference as vr

# (dh, lens): the real head size over three images of different shape; a full DH16 = 5; the smallest head; a row / column boundary inside a float4 (dh / 4 = 10)
CASES = [(72, (4, 60, 140)), (80, (64, 68)), (8, (32, 36, 16)), (40, (68, 64))]


def _bundle(case, fault=None):
    return vr.reference_bundle(vr.vis_attention_core, case["qkv"], case["cos"], case["sin"], case["lens"], case["nh"], case["dh"], fault=fault)


def test_rotary_tables_known_answer():
    """dh = 8: dh / 4 = 2 frequencies, 10000^(-0/4) = 1 and 10000^(-2/4) = 0.01.  Grid 2 x 3, patch 5 = (row 1, col 2): angles (1, 0.01, 2, 0.02);
    a second image starts again at (0, 0)"""
    cos, sin = vr.rotary_tables([(2, 3), (1, 2)], 8, dtype="float64")
    assert cos.shape == (8, 4) and sin.shape == (8, 4)
    assert np.allclose(cos[5], np.cos([1.0, 0.01, 2.0, 0.02]), atol=1e-15) and np.allclose(sin[5], np.sin([1.0, 0.01, 2.0, 0.02]), atol=1e-15)
    assert np.array_equal(cos[6], np.ones(4)) and np.array_equal(sin[6], np.zeros(4))
    assert np.allclose(sin[7], np.sin([0.0, 0.0, 1.0, 0.01]), atol=1e-15)
    c32, _ = vr.rotary_tables([(2, 3)], 8)
    assert c32.dtype == np.float32 and np.array_equal(c32[5], np.cos((np.float32([1, 1, 2, 2]) * np.float32([1.0, 0.01, 1.0, 0.01])).astype(np.float32)))
    assert vr.grid_of(140) == (10, 14) and vr.grid_of(31) == (1, 31) and vr.grid_of(64) == (8, 8) and vr.grid_of(1) == (1, 1)


@pytest.mark.parametrize("dh,lens", CASES)
def test_reference_agrees_with_a_second_spelling(dh, lens):
    case = vr.attention_case(dh, lens, seed=3)
    ref = _bundle(case)
    T, nh = sum(lens), case["nh"]
    qkv = torch.from_numpy(case["qkv"].astype(np.float64))
    ang = torch.complex(torch.from_numpy(case["cos"].astype(np.float64)), torch.from_numpy(case["sin"].astype(np.float64)))[:, None, :]   # e^(i angle)

    def rot(x):                                                               # (x[c] + i x[c + dh/2]) e^(i angle)
        z = torch.complex(x[..., :dh // 2], x[..., dh // 2:]) * ang
        return torch.cat([z.real, z.imag], -1)
    q, k, v = rot(qkv[:, 0]).transpose(0, 1), rot(qkv[:, 1]).transpose(0, 1), qkv[:, 2].transpose(0, 1)      # [nh, T, dh]
    owner = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    mask = owner[:, None] == owner[None, :]
    o = torch.nn.functional.scaled_dot_product_attention(q[None], k[None], v[None], attn_mask=mask, scale=float(np.float32(dh ** -0.5)))[0]
    o = o.transpose(0, 1).reshape(T, nh * dh).numpy()
    err = float(np.abs(o - ref["f64"]).max())
    print(f"dh {dh} lens {lens}: second spelling differs by {err:.2e} | noise {ref['noise']:.2e} tol {ref['tol']:.2e}")
    assert err <= 1e-12 and ref["noise"] > 0 and np.isfinite(ref["f64"]).all()


def test_the_cases_can_tell_wrong_readings_apart():
    """each fault moves the f64 output of at least one case by more than 100 tol of that case"""
    for fault in vr.FAULTS:
        moves = []
        for dh, lens in CASES:
            case = vr.attention_case(dh, lens, seed=3)
            ref = _bundle(case)
            table_fault = fault in ("row and column swapped", "frequencies over dh", "1-D rotary")
            wrong = vr.attention_case(dh, lens, seed=3, fault=fault) if table_fault else case
            assert np.array_equal(wrong["qkv"], case["qkv"])
            out = vr.vis_attention_core(wrong["qkv"], wrong["cos"], wrong["sin"], lens, case["nh"], dh, fault=None if table_fault else fault)
            moves.append(float(np.abs(out - ref["f64"]).max()) / ref["tol"])
        print(f"{fault}: moves the cases by {', '.join('%.0f' % m for m in moves)} tol")
        assert max(moves) > 100, (fault, moves)


def test_packed_layout_places_rows_and_poisons_gaps():
    case = vr.attention_case(8, (3, 2), seed=1)
    buf, off, ld = vr.packed_layout(case, pad=8, off=12)
    assert (off, ld) == (12, 56) and np.isnan(buf[:12]).all() and np.isnan(buf[12 + 48:12 + 56]).all()
    assert np.array_equal(buf[12 + 56 * 4:12 + 56 * 4 + 48], case["qkv"][4].ravel())
    dense, off0, ld0 = vr.packed_layout(case)
    assert (off0, ld0) == (0, 48) and np.array_equal(dense, case["qkv"].ravel())


# ------------------------------------------------------------------------------------------------ the entry point's argument checks (no launch, no device)
@pytest.fixture(scope="module")
def L():
    build.build_lib()
    return api.lib()


def _code(L, **kw):
    a = dict(lens=(5, 3), heads=2, head_dim=8, ld=48, qkv_off=0, buf_floats=8 * 48, o_floats=8 * 16, o_off=0, buf=True, o=True, cos=True, sin=True, segs=True, n_segs=None)
    a.update(kw)
    lens = np.asarray(a["lens"], np.int32)
    z = lambda n: np.zeros(max(int(n), 1), np.float32)
    buf, o, tab = z(a["buf_floats"]), z(a["o_floats"]), z(max(int(lens.sum()), 1) * 40)
    p = lambda arr, on: api._p(arr) if on else None
    return L.oar_k_vis_attention(p(buf, a["buf"]), a["buf_floats"], a["qkv_off"], a["ld"], p(lens, a["segs"]), lens.size if a["n_segs"] is None else a["n_segs"],
                                 a["heads"], a["head_dim"], p(tab, a["cos"]), p(tab, a["sin"]), p(o, a["o"]), a["o_floats"], a["o_off"])


def test_vis_attention_entry_point_rejects_bad_arguments_in_front_of_the_device(L):
    assert "oar_k_vis_attention" in api.EXPORTS and "vis_attention.hip" in build.SOURCES
    ok = (api.OAR_OK,) if api.device_count() > 0 else (api.OAR_DEVICE,)
    assert _code(L) in ok                                                     # the base call is a good one: only the device can be missing
    assert _code(L, ld=52, buf_floats=7 * 52 + 48) in ok and _code(L, qkv_off=8, buf_floats=8 * 48 + 8) in ok and _code(L, o_off=4, o_floats=8 * 16 + 4) in ok
    bad = api.OAR_INVALID_INPUT
    for name in ("buf", "o", "cos", "sin", "segs"):
        assert _code(L, **{name: False}) == bad, name
    for dh in (12, 88, 4, 0, -8, 84):
        assert _code(L, head_dim=dh) == api.OAR_UNSUPPORTED_OP, dh
    assert _code(L, heads=0) == bad and _code(L, heads=-2) == bad                 # a head count is an input, not a head size
    assert _code(L, lens=(5, 0, 3)) == bad and _code(L, lens=(8, -1)) == bad and _code(L, n_segs=0) == bad   # an empty segment, no segment
    assert _code(L, qkv_off=2, buf_floats=8 * 48 + 4) == bad and _code(L, o_off=2, o_floats=8 * 16 + 4) == bad   # misaligned offsets
    assert _code(L, ld=50, buf_floats=8 * 50) == bad and _code(L, ld=44) == bad and _code(L, ld=-48) == bad        # a misaligned stride, one below 3 D
    assert _code(L, buf_floats=8 * 48 - 1) == bad and _code(L, ld=52) == bad and _code(L, qkv_off=4) == bad        # views that do not fit
    assert _code(L, qkv_off=2 ** 64 - 4) == bad and _code(L, lens=(5, 4)) == bad
    assert _code(L, o_floats=8 * 16 - 1) == bad and _code(L, o_off=4) == bad
    with pytest.raises(api.OCRError) as e:
        api.k_vis_attention(np.zeros(8 * 48, np.float32), 0, 48, (5, 3), 2, 12, np.zeros((8, 6), np.float32), np.zeros((8, 6), np.float32), np.zeros(8 * 24, np.float32), 0)
    assert e.value.code == api.OAR_UNSUPPORTED_OP
    with pytest.raises(ValueError):
        api.k_vis_attention(np.zeros(8 * 48, np.float32), 0, 48, (5, 3), 2, 8, np.zeros((7, 4), np.float32), np.zeros((8, 4), np.float32), np.zeros(8 * 16, np.float32), 0)


# ================================================================================== the whole vision stage
from oar_ocr_amd import vl  # noqa: E402

_enc = {}


def _enc_case(name):
    if name not in _enc:
        case = vr.ENCODER_CASES[name]
        w, px = vr.make_vision(case), vr.make_pixels(case)
        _enc[name] = (case, w, px, vr.vision_bundle(case, w, px))
    return _enc[name]


def test_the_encoder_cases_are_the_ones_the_design_names():
    c = vr.ENCODER_CASES
    assert [(k, v.D, v.heads, v.dh, v.F, v.L, v.patch, v.G, v.text_hidden, v.grids) for k, v in c.items()] == [
        ("P", 144, 2, 72, 160, 2, 2, 5, 64, ((2, 2), (6, 10), (10, 14))), ("Q", 160, 2, 80, 96, 1, 2, 3, 48, ((8, 8), (2, 34))),
        ("R", 24, 3, 8, 40, 1, 2, 4, 40, ((4, 8), (6, 6), (4, 4))), ("S", 80, 2, 40, 96, 1, 4, 3, 48, ((2, 34), (8, 8))), ("K", 72, 1, 72, 100, 1, 14, 2, 40, ((2, 4),)), ("G", 16, 1, 16, 16, 1, 2, 2, 8, ((2, 2),))]
    assert all((3 * v.patch ** 2) % 4 == 0 and v.D % 4 == 0 and v.F % 4 == 0 for v in c.values())


def test_table_resampling_agrees_with_torch_interpolate_and_is_the_identity_at_the_table_size():
    rng = np.random.default_rng(2)
    for G, h, w in ((5, 2, 2), (5, 6, 10), (5, 10, 14), (3, 2, 34), (4, 4, 4), (2, 2, 4)):
        t = torch.from_numpy(rng.standard_normal((G * G, 6)))
        mine = vr.resample_table(t, G, h, w)
        theirs = torch.nn.functional.interpolate(t.reshape(1, G, G, 6).permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).reshape(h * w, 6)
        assert float((mine - theirs).abs().max()) <= 1e-14, (G, h, w)
        if h == w == G:
            assert torch.equal(mine, t)


def test_patch_embedding_agrees_with_conv2d():
    """the patch Linear over [T, 3 p p] rows in (c, dy, dx) order is the p x p / stride p convolution over the image"""
    case, w, px, ref = _enc_case("K")
    p, (h, wd) = case.patch, case.grids[0]
    img = torch.from_numpy(px.astype(np.float64)).reshape(h, wd, 3, p, p).permute(2, 0, 3, 1, 4).reshape(1, 3, h * p, wd * p)
    W = torch.from_numpy(w["visual.vision_model.embeddings.patch_embedding.weight"].astype(np.float64))
    b = torch.from_numpy(w["visual.vision_model.embeddings.patch_embedding.bias"].astype(np.float64))
    conv = torch.nn.functional.conv2d(img, W, b, stride=p)[0].permute(1, 2, 0).reshape(h * wd, case.D)
    lin = torch.from_numpy(px.astype(np.float64)) @ W.reshape(case.D, -1).T + b
    assert float((conv - lin).abs().max()) <= 1e-13
    assert np.array_equal(vl.patchify(img[0].permute(1, 2, 0).numpy().astype(np.float32), p), px)      # and vl.patchify is that order


def test_every_encoder_fault_moves_a_case_by_more_than_100_tol():
    least = {}
    for fault in vr.ENCODER_FAULTS:
        best = 0.0
        for name in vr.ENCODER_CASES:
            case, w, px, ref = _enc_case(name)
            f, e = vr.vision_forward(case, w, px, "float64", fault=fault)
            best = max(best, float(np.abs(f - ref["feat"]["f64"]).max()) / ref["feat"]["tol"], float(np.abs(e - ref["emb"]["f64"]).max()) / ref["emb"]["tol"])
        least[fault] = best
        print(f"{fault}: best movement {best:.0f} tol")
    assert all(v > 100 for v in least.values()), least


def test_smart_resize_known_answers():
    # (64, 64): rounds to 56 x 56 = 3136 < 101920; beta = sqrt(101920 / 4096) = 4.988..., ceil(64 beta / 28) = ceil(11.40) = 12 -> 336
    assert vl.smart_resize(64, 64, 28, 101920, 1003520) == (336, 336)
    # (2000, 1500): rounds to 1988 x 1512 = 3005856 > 1003520; beta = sqrt(3e6 / 1003520) = 1.72900; 2000 / beta / 28 = 41.31 -> 41 * 28 = 1148; 1500 / beta / 28 = 30.98 -> 30 * 28 = 840
    assert vl.smart_resize(2000, 1500, 28, 101920, 1003520) == (1148, 840) and 1148 * 840 <= 1003520
    assert vl.smart_resize(56, 84, 28, 1, 10 ** 9) == (56, 84) and vl.smart_resize(42, 41, 28, 1, 10 ** 9) == (56, 28)   # 1.5 rounds away from zero, 1.46 down
    with pytest.raises(api.OCRError):   # 201 : 1
        vl.smart_resize(10, 2010, 28, 1, 10 ** 9)
    # (100, 100), min 20000, max 20000: rounds to 112 x 112 = 12544 < min; beta = sqrt(2) -> ceil(141.4 / 28) = 6 -> 168 x 168 = 28224 > max: cannot satisfy
    with pytest.raises(api.OCRError) as e:
        vl.smart_resize(100, 100, 28, 20000, 20000)
    assert "cannot satisfy" in str(e.value)
    # (1000, 1000), min 900000, max 800000: 1008 x 1008 > max; beta = sqrt(1.25) = 1.118; floor(894.4 / 28) = 31 -> 868 x 868 = 753424 < min: cannot satisfy
    with pytest.raises(api.OCRError) as e:
        vl.smart_resize(1000, 1000, 28, 900000, 800000)
    assert "cannot satisfy" in str(e.value)
    rng = np.random.default_rng(4)
    for _ in range(200):
        h, w = int(rng.integers(20, 3000)), int(rng.integers(20, 3000))
        assert vl.smart_resize(h, w, 28, 101920, 1003520) == vr.smart_resize_ref(h, w, 28, 101920, 1003520), (h, w)
    # f64, as the reference implementation computes it, not exact arithmetic: 1845 / (beta 28) is exactly 60 (3600 x 784 x 656 = 1845 x 1003520), the f64 quotient falls just
    # below and floors to 59 -- 1652, where the exact-arithmetic spelling says 1680
    assert vl.smart_resize(1845, 656, 28, 101920, 1003520) == (1652, 588) and vr.smart_resize_ref(1845, 656, 28, 101920, 1003520) == (1680, 588)


def test_rope_index_known_answer():
    a, b, START, IMG, END = 5, 6, 90, 91, 92
    pos, delta = vl.rope_index([a, START] + [IMG] * 6 + [END, b], [(4, 6)], IMG, START, 2)
    want = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (2, 2, 3), (2, 2, 4), (2, 3, 2), (2, 3, 3), (2, 3, 4), (5, 5, 5), (6, 6, 6)]
    assert pos.shape == (3, 10) and pos.dtype == np.int32 and [tuple(c) for c in pos.T] == want and delta == -3
    pos2, delta2 = vl.rope_index([START] + [IMG] * 2 + [END, START] + [IMG] * 1 + [END], [(2, 4), (2, 2)], IMG, START, 2)
    assert [tuple(c) for c in pos2.T] == [(0, 0, 0), (1, 1, 1), (1, 1, 2), (3, 3, 3), (4, 4, 4), (5, 5, 5), (6, 6, 6)] and delta2 == 0
    with pytest.raises(api.OCRError) as e:
        vl.rope_index([a, START] + [IMG] * 6 + [END, b], [(4, 6), (2, 2)], IMG, START, 2)
    assert "count mismatch" in str(e.value)


def test_preprocess_images_is_the_naive_loop_and_resizes_to_the_expected_grid():
    cfg = vl.ImageProcessorConfig.from_json(dict(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096, rescale_factor=1 / 255, image_mean=[0.5, 0.4, 0.3], image_std=[0.5, 0.25, 0.2]))
    img = np.random.default_rng(1).integers(0, 256, (12, 20, 3), dtype=np.uint8)                     # 12 x 20: multiples of 4, 240 pixels inside the limits
    px, grids = vl.preprocess_images([img], cfg)
    assert grids.tolist() == [[6, 10]] and px.dtype == np.float32
    assert px.tobytes() == vr.patchify_ref(img, 2, cfg.rescale_factor, cfg.image_mean, cfg.image_std).tobytes()
    assert vl.smart_resize(13, 22, 4, 16, 4096) == (12, 24)
    with pytest.raises(api.OCRError) as e:
        vl.preprocess_images([img], vl.ImageProcessorConfig(patch_size=2, merge_size=2, resample=0))
    assert e.value.code == api.OAR_UNSUPPORTED_OP


# ------------------------------------------------------------------------------------------------ oar_vis_create / encode / cost: refused before the device
def _vis_create(L, case, weights, **kw):
    d = dict(hidden_size=case.D, num_hidden_layers=case.L, num_attention_heads=case.heads, intermediate_size=case.F, patch_size=case.patch, text_hidden=case.text_hidden,
             pos_grid=case.G, spatial_merge_size=case.merge, max_tokens=case.tokens, max_images=len(case.grids))
    d.update(kw)
    try:
        vl.VisionEncoder.from_state_dict(vl.VisionConfig(**d), weights).close()
        return api.OAR_OK
    except api.OCRError as e:
        return e.code


def test_vis_create_rejects_bad_configurations_and_tables_in_front_of_the_device(L):
    case, w, px, _ = _enc_case("R")
    for sym in ("oar_vis_create", "oar_vis_encode", "oar_vis_cost", "oar_vis_destroy"):
        assert sym in api.EXPORTS and hasattr(L, sym)
    assert "vis_host.cc" in build.SOURCES and "vis_misc.hip" in build.SOURCES
    ok = api.OAR_OK if api.device_count() > 0 else api.OAR_DEVICE
    assert _vis_create(L, case, w) == ok                                      # the base configuration is a good one: only the device can be missing
    bad = api.OAR_INVALID_INPUT
    for kw in (dict(num_attention_heads=5), dict(hidden_size=0), dict(num_hidden_layers=0), dict(max_images=0), dict(max_images=17), dict(max_tokens=3), dict(spatial_merge_size=0),
               dict(layer_norm_eps=0.0), dict(rope_theta=-1.0), dict(patch_size=1), dict(intermediate_size=42), dict(hidden_size=26, num_attention_heads=1)):
        assert _vis_create(L, case, w, **kw) == bad, kw
    assert _vis_create(L, case, w, num_attention_heads=2) == api.OAR_UNSUPPORTED_OP        # head size 12
    assert _vis_create(L, case, w, num_attention_heads=1, hidden_size=88) == api.OAR_UNSUPPORTED_OP
    with pytest.raises(api.OCRError) as e:
        vl.VisionConfig(hidden_size=24, num_hidden_layers=1, num_attention_heads=3, intermediate_size=40, patch_size=2, text_hidden=40, hidden_act="relu").to_c()
    assert e.value.code == api.OAR_UNSUPPORTED_OP
    for name in ("visual.vision_model.encoder.layers.0.self_attn.k_proj.bias", "mlp_AR.linear_2.weight", "visual.vision_model.embeddings.position_embedding.weight",
                 "visual.vision_model.post_layernorm.weight"):
        assert _vis_create(L, case, {k: v for k, v in w.items() if k != name}) == bad, name
        assert _vis_create(L, case, {**w, name: w[name][..., :-1]}) == bad, name              # a wrong shape
        assert _vis_create(L, case, {**w, name: w[name].astype(np.float64).view(np.uint16)}) == bad, name   # bf16 bits of four times the length
    assert _vis_create(L, case, {**w, "unrelated.weight": np.zeros(3, np.float32), "visual.other": np.zeros(3, np.float32)}) == ok
    assert _vis_create(L, case, w, pos_grid=5) == bad                          # the table is 4 x 4
    cfg = vl.VisionConfig.from_hf_json(dict(hidden_size=1152, num_hidden_layers=27, num_attention_heads=16, intermediate_size=4304, patch_size=14, image_size=384, spatial_merge_size=2,
                                            layer_norm_eps=1e-6, hidden_act="gelu_pytorch_tanh", num_channels=3), text_hidden=1024)
    assert (cfg.pos_grid, cfg.hidden_size // cfg.num_attention_heads, cfg.act_code(), cfg.text_hidden) == (27, 72, vl.OAR_VIS_GELU_TANH, 1024)


def test_composite_case_is_greedy_safe_and_its_positions_agree():
    """PA: the f64 margin between the best and the second-best logit exceeds 4 tol at each of the 24 free-running steps of both sequences (seed 0, the first tried);
    15 and 1 image tokens, prefix 2 and suffix 3 ids inside the vocabulary; vl.rope_index gives the reference's positions"""
    r = vr.composite_reference()
    assert r["margins"].shape == (2, 24) and float(r["margins"].min()) > 4 * r["tol"], (float(r["margins"].min()), r["tol"])
    print(f"PA: noise {r['noise']:.2e} tol {r['tol']:.2e} least margin {r['margins'].min() / r['tol']:.1f} tol")
    assert [len(run[2]) for run in r["runs"]] == [2 + 15 + 3, 2 + 1 + 3] and all(0 <= v < 97 for run in r["runs"] for v in run[2])
    for (t64, l64, ids, pos), grid in zip(r["runs"], vr.PA_GRIDS):
        mine, delta = vl.rope_index(ids, [grid], vr.PA_IDS["image"], vr.PA_IDS["start"], 2)
        ref_pos, ref_delta = vr.rope_index_ref(ids, [grid], vr.PA_IDS["image"], vr.PA_IDS["start"], 2)
        assert np.array_equal(mine, pos) and np.array_equal(ref_pos, pos) and delta == ref_delta
    px, grids = vl.preprocess_images(r["images"], vl.ImageProcessorConfig(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096))
    assert grids.tolist() == [list(g) for g in vr.PA_GRIDS]
    assert px[:60].tobytes() == vr.patchify_ref(r["images"][0], 2, 1.0 / 255.0, (0.5,) * 3, (0.5,) * 3).tobytes()


def test_pos_embed_entry_point_rejects_bad_arguments_in_front_of_the_device(L):
    assert "oar_k_vis_pos_embed" in api.EXPORTS
    ok = (api.OAR_OK,) if api.device_count() > 0 else (api.OAR_DEVICE,)

    def code(G=2, D=8, grids=((2, 2), (4, 6)), table=True, o=True, g=True, o_floats=None, o_off=0, n=None):
        gr = np.asarray(grids, np.int32).reshape(-1, 2)
        T = int(np.maximum(gr[:, 0], 0).astype(np.int64) @ np.maximum(gr[:, 1], 0)) if gr.size else 0
        o_floats = T * max(D, 0) if o_floats is None else o_floats
        tab, out = np.zeros(max(G * G * D, 1), np.float32), np.zeros(max(o_floats, 1), np.float32)
        p = lambda a, on: api._p(a) if on else None   # noqa: E731
        return L.oar_k_vis_pos_embed(p(tab, table), G, D, p(gr, g and gr.size), gr.shape[0] if n is None else n, p(out, o), o_floats, o_off)
    assert code() in ok and code(o_floats=28 * 8 + 4, o_off=4) in ok
    bad = api.OAR_INVALID_INPUT
    for kw in (dict(table=False), dict(o=False), dict(g=False), dict(G=0), dict(G=1025), dict(D=6), dict(D=0), dict(n=0), dict(grids=((2, 2),) * 17), dict(grids=((2, 0),)),
               dict(grids=((-1, 2),)), dict(o_floats=28 * 8 - 1), dict(o_off=4), dict(o_floats=28 * 8 + 4, o_off=2)):
        assert code(**kw) == bad, kw
    with pytest.raises(ValueError):
        api.k_vis_pos_embed(np.zeros((5, 8), np.float32), 2, [(2, 2)], np.zeros(32, np.float32), 0)
