"""The reference of the Qwen vision towers (synth/qwen_vision_reference.py) and the host routines of the library that need no device: the window
plan in both spellings against recorded results (tests/golden/qwen_window_plan.json), case W5's plan as worked out by hand, the patch positions, the
preprocessing against the naive loop, every argument check of oar_qvis_check, every fault moving its case by more than 4 tol, and the composite cases' margins."""
import json
from pathlib import Path

import numpy as np
import pytest

from oar_ocr_amd import api, build, vl
from oar_ocr_amd.synth import qwen_vision_reference as qr

GOLDEN = json.loads((Path(__file__).parent / "golden" / "qwen_window_plan.json").read_text())


def _plans(grids, merge, patch, window):
    """the plan in both spellings, as (window_index, reverse_index, cumulative segment ends)"""
    out = []
    for fn in (qr.window_plan, vl.qvis_window_plan):
        wi, ri, segs = fn([g[-2:] for g in grids], merge, patch, window)
        assert [s for s, _ in segs] == [0] + list(np.cumsum([n for _, n in segs])[:-1])
        out.append((list(map(int, wi)), list(map(int, ri)), [0] + [int(v) for v in np.cumsum([n for _, n in segs])]))
    assert out[0] == out[1]
    return out[0]


@pytest.mark.parametrize("case", GOLDEN["window_plan"], ids=lambda c: c["name"])
def test_window_plan_matches_the_recorded_results(case):
    grids, args = case["grids"], (case["merge"], case["patch"], case["window_size"])
    if case.get("rejected"):
        with pytest.raises(ValueError, match="window_size"):
            qr.window_plan([g[-2:] for g in grids], *args)
        with pytest.raises(api.OCRError) as e:
            vl.qvis_window_plan([g[-2:] for g in grids], *args)
        assert e.value.code == api.OAR_INVALID_INPUT and "window_size" in str(e.value)
        return
    wi, ri, cu = _plans(grids, *args)
    for key, got in (("window_index", wi), ("reverse_index", ri), ("cu_window_seqlens", cu)):
        if key in case:
            assert got == case[key], key
    if "window_index_head" in case:
        assert wi[:len(case["window_index_head"])] == case["window_index_head"]
    if "window_index_tail" in case:
        assert wi[case["window_index_tail_from"]:] == case["window_index_tail"]
    if "units" in case:
        assert len(wi) == case["units"] and cu[-1] == case["units"] * case["merge"] ** 2
    if case.get("mutual_inverse"):
        assert sorted(wi) == list(range(len(wi)))
        for slot, source in enumerate(wi):
            assert ri[source] == slot and wi[ri[source]] == source


def test_the_plan_of_case_w5():
    c = qr.QVIS_CASES["W5"]
    wi, ri, cu = _plans(c.grids, c.merge, c.patch, c.window_size)
    assert list(np.diff(cu)) == [64, 48, 48, 36, 64, 64, 64, 64, 16]      # (14, 14): partial edge windows; (16, 16): its empty tail windows dropped; (4, 4): one partial window
    assert [h * w for h, w in c.grids] == [196, 256, 16] and c.fullatt == (1,) and c.L == 3      # full attention: more than three query tiles, exactly four, less than one
    assert sorted(wi[:49]) == list(range(49)) and sorted(wi[49:113]) == list(range(49, 113)) and wi[113:] == [113, 114, 115, 116]   # no unit leaves its image


def test_positions_run_in_merge_grouped_order():
    p = GOLDEN["vision_position_ids"]
    hp, wp = qr.vision_position_ids(p["t"], p["h"], p["w"], p["merge"])
    assert hp == p["hpos"] and wp == p["wpos"]
    cos, _ = qr.qrotary_tables([(4, 4)], 2, 8)                                 # the tables follow them: angle = position x 1 at frequency 0
    assert np.allclose(cos[:, 0], np.cos(np.asarray(p["hpos"], np.float32))) and np.allclose(cos[:, 2], np.cos(np.asarray(p["wpos"], np.float32)))


def test_preprocess_images_qwen_against_the_loop():
    """no resize needed (sizes are multiples of the factor inside the pixel bounds): the order of the patches, of the values within a patch, and the frame repeated"""
    rng = np.random.default_rng(3)
    cfg = vl.ImageProcessorConfig(patch_size=2, merge_size=2, min_pixels=16, max_pixels=4096, image_mean=(0.4, 0.5, 0.6), image_std=(0.2, 0.3, 0.4))
    images = [rng.integers(0, 256, (12, 20, 3), dtype=np.uint8), rng.integers(0, 256, (4, 8, 3), dtype=np.uint8)]
    for temporal in (1, 2, 3):
        px, grids = vl.preprocess_images_qwen(images, cfg, temporal)
        want = np.concatenate([qr.patchify_qwen_ref(im, 2, 2, temporal, cfg.rescale_factor, cfg.image_mean, cfg.image_std) for im in images])
        assert grids.tolist() == [[6, 10], [2, 4]] and px.shape == (68, 12 * temporal) and px.tobytes() == want.tobytes()
        frames = px.reshape(68, 3, temporal, 4)
        assert all(np.array_equal(frames[:, :, 0], frames[:, :, t]) for t in range(temporal))
    first = vl.preprocess_images(images[:1], cfg)[0]                           # the raster patches of the PaddleOCR-VL path, regrouped
    order = [(hb * 2 + mi) * 10 + wb * 2 + mj for hb in range(3) for wb in range(5) for mi in range(2) for mj in range(2)]
    assert np.array_equal(vl.preprocess_images_qwen(images[:1], cfg, 1)[0], first[order])
    with pytest.raises(api.OCRError) as e:                                     # smaller than one factor: refused with do_resize on ...
        vl.preprocess_images_qwen([np.zeros((3, 8, 3), np.uint8)], cfg)
    assert e.value.code == api.OAR_INVALID_INPUT and "factor" in str(e.value)
    import dataclasses
    with pytest.raises(api.OCRError):                                          # ... and, off, for not being divisible
        vl.preprocess_images_qwen([np.zeros((3, 8, 3), np.uint8)], dataclasses.replace(cfg, do_resize=False))


def _vcfg(**kw):
    d = dict(kind="qwen2_5", embed_dim=160, depth=3, num_heads=2, intermediate_size=200, patch_size=2, out_hidden_size=48, hidden_act="silu", window_size=16,
             fullatt_block_indexes=[1], max_tokens=468, max_images=3)
    d.update(kw)
    return vl.QwenVisionConfig(**d)


def test_every_argument_check_without_a_device():
    vl.qvis_check(_vcfg(), [(14, 14), (16, 16), (4, 4)])
    vl.qvis_check(_vcfg(kind="qwen2", window_size=0, fullatt_block_indexes=[], hidden_act="quick_gelu"))
    invalid = [dict(embed_dim=0), dict(depth=0), dict(num_heads=0), dict(intermediate_size=-4), dict(patch_size=0), dict(temporal_patch_size=0), dict(in_channels=0),
               dict(spatial_merge_size=0), dict(out_hidden_size=0), dict(max_tokens=0), dict(max_images=0), dict(max_images=17), dict(num_heads=3),
               dict(window_size=0), dict(window_size=-16), dict(window_size=18), dict(fullatt_block_indexes=[3]), dict(fullatt_block_indexes=[0, -1]), dict(out_hidden_size=50)]
    for kw in invalid:
        with pytest.raises(api.OCRError) as e:
            vl.qvis_check(_vcfg(**kw))
        assert e.value.code == api.OAR_INVALID_INPUT, (kw, e.value.code)
    for kw in (dict(num_heads=1), dict(embed_dim=24, num_heads=2), dict(embed_dim=176, num_heads=2)):       # head sizes 160, 12, 88
        with pytest.raises(api.OCRError) as e:
            vl.qvis_check(_vcfg(**kw))
        assert e.value.code == api.OAR_UNSUPPORTED_OP, (kw, e.value.code)
    with pytest.raises(api.OCRError) as e:                                     # an activation code the library does not know
        vl.qvis_check(_vcfg(), act=7)
    assert e.value.code == api.OAR_UNSUPPORTED_OP
    with pytest.raises(api.OCRError) as e:                                     # a name the binding does not know
        vl.qvis_check(_vcfg(hidden_act="relu"))
    assert e.value.code == api.OAR_UNSUPPORTED_OP
    for grids in ([(3, 4)], [(4, 6), (14, 14), (16, 16)], [(2, 2)] * 4, []):   # merge, max_tokens, max_images, none
        with pytest.raises(api.OCRError) as e:
            vl.qvis_check(_vcfg(), grids if grids else np.zeros((0, 2), np.int32))
        assert e.value.code == api.OAR_INVALID_INPUT, grids


def test_config_from_hf_json_decides_the_kind_from_the_keys():
    q2 = vl.QwenVisionConfig.from_hf_json(dict(depth=32, embed_dim=1280, hidden_size=1536, mlp_ratio=4, num_heads=16, in_chans=3, patch_size=14, spatial_merge_size=2, temporal_patch_size=2), 1536)
    assert (q2.kind, q2.embed_dim, q2.intermediate_size, q2.out_hidden_size, q2.hidden_act, q2.in_channels) == ("qwen2", 1280, 5120, 1536, "quick_gelu", 3)
    q5 = vl.QwenVisionConfig.from_hf_json(dict(depth=32, hidden_size=1280, out_hidden_size=2048, intermediate_size=3420, num_heads=16, in_channels=3, patch_size=14, spatial_merge_size=2,
                                               temporal_patch_size=2, window_size=112, fullatt_block_indexes=[7, 15, 23, 31]), 2048)
    assert (q5.kind, q5.embed_dim, q5.intermediate_size, q5.out_hidden_size, q5.hidden_act, q5.window_size, list(q5.fullatt_block_indexes)) == ("qwen2_5", 1280, 3420, 2048, "silu", 112, [7, 15, 23, 31])
    with pytest.raises(api.OCRError):
        vl.QwenVisionConfig.from_hf_json(dict(depth=2, num_heads=2, patch_size=14), 64)
    assert {"oar_qvis_create", "oar_qvis_destroy", "oar_qvis_encode", "oar_qvis_cost", "oar_qvis_check", "oar_qvis_window_plan", "oar_k_qvis_rmsnorm", "oar_k_qvis_act",
            "oar_k_qvis_row_gather"} <= set(api.EXPORTS)
    assert "qvis_misc.hip" in build.SOURCES and "qvis_host.cc" in build.SOURCES


_bundles = {}


def _bundle(name):
    if name not in _bundles:
        c = qr.QVIS_CASES[name]
        w, px = qr.make_qvision(c), qr.make_qpixels(c)
        _bundles[name] = (c, w, px, qr.qvision_bundle(c, w, px))
    return _bundles[name]


@pytest.mark.parametrize("fault", list(qr.FAULTS))
def test_every_fault_bites(fault):
    """A GPU result may sit one tol from the truth, so a fault must move the f64 output of its case by more than 4 tol: a factor of two on each side."""
    c, w, px, b = _bundle(qr.FAULTS[fault])
    feat, emb = qr.qvision_forward(c, w, px, "float64", fault=fault)
    moved = {"feat": float(np.abs(feat - b["feat"]["f64"]).max()) / b["feat"]["tol"], "emb": float(np.abs(emb - b["emb"]["f64"]).max()) / b["emb"]["tol"]}
    print(f"{fault} on {c.name}: features move {moved['feat']:.0f} tol, embeddings {moved['emb']:.0f} tol")
    assert moved["emb"] > 4.0, moved                                            # (the embeddings: what the decoder sees, and what every fault must reach)
    if fault != "no reverse permutation":                                      # (that one happens behind the features)
        assert moved["feat"] > 4.0, moved


@pytest.mark.parametrize("name", ["W5", "X5"])
def test_the_eps_fault_bites_on_rows_near_eps(name):
    """eps inside the mean's divisor moves the unit-scale cases by less than tol (eps / D against eps under mean(x^2) ~ 1); with the pixels scaled by 1e-3 it moves the
    f64 output by more than 4 tol.  tests/test_gpu_qwen_vision.py::test_rows_near_eps_match_f64 runs that input."""
    c, w, px, b = _bundle(name)
    small = (px * np.float32(qr.EPS_FAULT_SCALE)).astype(np.float32)
    ref = qr.qvision_bundle(c, w, small)
    feat, emb = qr.qvision_forward(c, w, small, "float64", fault=qr.EPS_FAULT)
    moved = {"feat": float(np.abs(feat - ref["feat"]["f64"]).max()) / ref["feat"]["tol"], "emb": float(np.abs(emb - ref["emb"]["f64"]).max()) / ref["emb"]["tol"]}
    f1, e1 = qr.qvision_forward(c, w, px, "float64", fault=qr.EPS_FAULT)
    unit = {"feat": float(np.abs(f1 - b["feat"]["f64"]).max()) / b["feat"]["tol"], "emb": float(np.abs(e1 - b["emb"]["f64"]).max()) / b["emb"]["tol"]}
    print(f"{name}: at unit scale the fault moves {unit}, at 1e-3 {moved} (in tol)")
    assert moved["feat"] > 4.0 and moved["emb"] > 4.0, moved


def test_the_hidden_act_names():
    x = np.linspace(-3, 3, 25)
    assert all(np.array_equal(qr.act_fn(n, x), qr.act_fn("gelu", x)) for n in qr.ERF_NAMES)                  # all three names: the erf form
    assert np.abs(qr.act_fn("gelu", x) - qr.act_fn("quick_gelu", x)).max() > 1e-3 and np.allclose(qr.act_fn("silu", x), x / (1 + np.exp(-x)))
    assert vl.QVIS_ACTS["gelu"] == vl.QVIS_ACTS["gelu_new"] == vl.QVIS_ACTS["gelu_pytorch_tanh"] != vl.QVIS_ACTS["quick_gelu"]


@pytest.mark.parametrize("name", list(qr.COMPOSITES))
def test_the_composite_references_meet_their_margins(name):
    ref = qr.composite_reference(name)
    cond = qr.composite_conditions(ref)
    print(name, cond, f"tol {ref['tol']:.2e}")
    assert cond["margin_ratio"] > 1.0, cond                                     # the f64 run alone keeps more than 2 tol at every step
    assert ref["lm_case"].qkv_bias and len(ref["runs"]) == 3
    if name == "MA":
        assert cond["ngram_margin_ratio"] > 1.0 and cond["least_changed"] >= 1, cond


def test_qwenvl_refuses_the_refill_schedule_with_processors_without_a_device():
    m = vl.QwenVL.__new__(vl.QwenVL)                                           # (the refusal comes before anything is touched)
    for kw in (dict(no_repeat_ngram_size=3), dict(repetition_penalty=1.3)):
        with pytest.raises(api.OCRError) as e:
            vl.QwenVL.generate_tokens(m, [], (1,), (2,), schedule="refill", **kw)
        assert e.value.code == api.OAR_UNSUPPORTED_OP
