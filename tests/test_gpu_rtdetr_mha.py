"""RT-DETR graphs with the fused multi-head attention on the GPU, OAR_FUSE_MHA_ATTENTION=1 and OAR_FUSE_DEFORMABLE_ATTENTION=1 set here:
the decoder (synth.models.build_rtdetr_decoder) runs one mha_attention and one deformable_attention launch per layer and no softmax launch, every declared
output within its own tol of the f64 reference, layer by layer; the AIFI layer (build_aifi_layer) runs one mha_attention launch; the whole detector with a
hybrid-encoder layer (build_table_cell_det(decoder_layers=2, encoder_layers=1)) goes through the three checks of tests/test_gpu_rtdetr_decoder.py."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.structure import from_coords
from oar_ocr_amd.synth import models, pages
from oar_ocr_amd.synth.mha_reference import aifi_layer_reference, reference_bundle
from oar_ocr_amd.synth.rtdetr_reference import rtdetr_decoder_reference
from oracle import cpu_ref as R
from oracle import onnx_ref

pytestmark = pytest.mark.gpu

KNOBS = ("OAR_FUSE_MHA_ATTENTION", "OAR_FUSE_DEFORMABLE_ATTENTION")
DEC = dict(D=32, nh=4, levels=((8, 8), (4, 4), (2, 2)), P=4, layers=2, Q=20, n_classes=3, seed=0)      # tests/test_gpu_rtdetr_decoder.py's
N = 2
SHAPE, QUERIES, KEEP, LAYERS, ENC, SEED = (128, 128), 40, 24, 2, 1, 22
RTDETR_PRE = dict(filter="triangle", scale=1.0 / 255.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), bgr=True)


def _launches(eng, feeds, names):
    try:
        api.prof_reset()
        api.prof_enable(True)
        outs = dict(eng.infer([(k, feeds[k]) for k in names]))
        return outs, {e["name"]: e["launches"] for e in api.prof_snapshot()}
    finally:
        api.prof_enable(False)


def _load(model, monkeypatch):
    for k in KNOBS:
        monkeypatch.setenv(k, "1")
    return api.OrtInfer(model, profile=True)


def test_decoder_runs_one_attention_launch_of_each_kind_per_layer(monkeypatch):
    model, info = models.build_rtdetr_decoder(**DEC)
    rng = np.random.default_rng(3)
    Lv = sum(h * w for h, w in info["levels"])
    feeds = {"memory": rng.standard_normal((N, Lv, DEC["D"])).astype(np.float32), "tgt": rng.standard_normal((N, DEC["Q"], DEC["D"])).astype(np.float32),
             "ref_logit": rng.uniform(-1.5, 1.5, (N, DEC["Q"], 4)).astype(np.float32)}
    eng = _load(model, monkeypatch)
    try:
        outs, snap = _launches(eng, feeds, ("memory", "tgt", "ref_logit"))
    finally:
        eng.close()
    print(f"{sum(snap.values())} launches, mha_attention {snap.get('mha_attention', 0)}, deformable_attention {snap.get('deformable_attention', 0)}, softmax {snap.get('softmax', 0)}")
    assert snap.get("mha_attention", 0) == info["layers"] and snap.get("deformable_attention", 0) == info["layers"] and snap.get("softmax", 0) == 0, sorted(snap.items())
    bad = []
    for nm in info["layer_outputs"] + ["boxes", "logits"]:          # in the order of the layers: the first name printed as bad is where an error enters
        ref = reference_bundle(rtdetr_decoder_reference, info, feeds["memory"], feeds["tgt"], feeds["ref_logit"], want=nm)
        err = float(np.abs(outs[nm].astype(np.float64) - ref["f64"]).max())
        print(f"  {nm}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
        if outs[nm].shape != ref["f64"].shape or not err <= ref["tol"]:
            bad.append((nm, err, ref["tol"]))
    assert not bad, bad


def test_aifi_layer_is_one_attention_launch(monkeypatch):
    H, W, D, nh, F = 5, 7, 32, 4, 64
    model, info = models.build_aifi_layer(H, W, D, nh, F, seed=2)
    src = np.random.default_rng(5).standard_normal((N, H * W, D)).astype(np.float32)
    ref = reference_bundle(aifi_layer_reference, info, src)
    eng = _load(model, monkeypatch)
    try:
        outs, snap = _launches(eng, {"src": src}, ("src",))
    finally:
        eng.close()
    err = float(np.abs(outs["y"].astype(np.float64) - ref["f64"]).max())
    print(f"aifi layer: {sum(snap.values())} launches | noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
    assert snap.get("mha_attention", 0) == 1 and snap.get("softmax", 0) == 0, sorted(snap.items())
    assert outs["y"].shape == ref["f64"].shape and err <= ref["tol"], (err, ref["tol"])


# ------------------------------------------------------------------------------------------------ the whole detector
@pytest.fixture(scope="module")
def det():
    mp = pytest.MonkeyPatch()
    try:
        for k in KNOBS:
            mp.setenv(k, "1")
        m, info = models.build_table_cell_det(image_shape=SHAPE, queries=QUERIES, keep=KEEP, decoder_layers=LAYERS, encoder_layers=ENC, seed=SEED)
        imgs = [pages.make_page(30 + i, (200 + 60 * i, 260 - 30 * i), 6 + i) for i in range(3)]
        x = np.stack([R.layout_preprocess(im, SHAPE, **RTDETR_PRE)[0] for im in imgs])
        feeds = {"image": x,
                 "scale_factor": np.array([[np.float32(SHAPE[0]) / np.float32(im.shape[0]), np.float32(SHAPE[1]) / np.float32(im.shape[1])] for im in imgs], np.float32),
                 "im_shape": np.array([[SHAPE[0], SHAPE[1]]] * len(imgs), np.float32)}
        eng = api.OrtInfer(m, profile=True)
        try:
            outs, snap = _launches(eng, feeds, ("image", "scale_factor", "im_shape"))
        finally:
            eng.close()
        return {"model": m, "info": info, "imgs": imgs, "feeds": feeds, "outs": outs, "snap": snap}
    finally:
        mp.undo()


def _segments_with_engine_indices(model, feeds, engine_idx):
    """every float segment through onnx_ref; TopK takes the ENGINE's indices, the gathers are numpy's (as in tests/test_gpu_rtdetr_decoder.py)"""
    env = dict(feeds)
    seg = []

    def flush():
        if seg:
            outs = [o for nd in seg for o in nd["outputs"]]
            need = {i for nd in seg for i in nd["inputs"] if i in env}
            vals = onnx_ref.run({"nodes": list(seg), "inits": model["inits"], "inputs": [], "outputs": outs}, {k: env[k] for k in need}, want=outs)
            env.update(zip(outs, vals))
            seg.clear()

    for nd in model["nodes"]:
        if nd["op"] not in ("TopK", "GatherND", "GatherElements"):
            seg.append(nd)
            continue
        flush()
        a = [env[i] if i in env else model["inits"][i] for i in nd["inputs"]]
        if nd["op"] == "TopK":
            idx = engine_idx[nd["outputs"][1]]
            env[nd["outputs"][0]], env[nd["outputs"][1]] = np.take_along_axis(a[0], idx, -1), idx
        elif nd["op"] == "GatherND":
            assert nd["attrs"].get("batch_dims", 0) == 1 and a[1].shape[-1] == 1
            env[nd["outputs"][0]] = a[0][np.arange(a[0].shape[0])[:, None], a[1][..., 0]]
        else:
            env[nd["outputs"][0]] = np.take_along_axis(a[0], a[1], nd["attrs"].get("axis", 0))
    flush()
    return env


def test_detector_runs_one_attention_launch_per_encoder_and_decoder_layer(det):
    snap = det["snap"]
    assert snap.get("mha_attention", 0) == ENC + LAYERS and snap.get("deformable_attention", 0) == LAYERS and snap.get("softmax", 0) == 0, sorted(snap.items())


def test_detector_selections_are_the_stable_selections_of_their_inputs(det):
    for t in det["info"]["topk"]:
        x, idx = det["outs"][t["input"]], det["outs"][t["index"]]
        assert idx.dtype == np.int64 and idx.shape == (3, t["k"]) and x.dtype == np.float32
        assert np.array_equal(idx, np.argsort(-x, axis=-1, kind="stable")[:, :t["k"]]), t


def test_detector_float_segments_agree_with_the_reference_evaluator(det):
    info, outs = det["info"], det["outs"]
    env = _segments_with_engine_indices(onnx_ref.parse_model(det["model"]), det["feeds"], {t["index"]: outs[t["index"]] for t in info["topk"]})
    for name in [t["input"] for t in info["topk"]] + ["boxes"]:
        ref, got = env[name], outs[name]
        err, bound = np.abs(got - ref).max(), 2e-4 * max(1.0, np.abs(ref).max())
        print(name, ref.shape, "max abs err", err, "bound", bound)
        assert got.shape == ref.shape and err <= bound, (name, err, bound)
    assert outs["boxes"].shape == (3 * KEEP, 6)
    sc = outs["boxes"].reshape(3, KEEP, 6)[..., 1]
    assert np.all(sc[:, :-1] >= sc[:, 1:])


def test_predictor_equals_layout_postprocess_of_the_engines_rows(det, monkeypatch):
    for k in KNOBS:
        monkeypatch.setenv(k, "1")
    imgs, thr, max_cells = det["imgs"], 0.3, 300
    mc = api.TableCellModelConfig("synthetic_cell_det", 1, {0: "cell"}, "rtdetr", SHAPE)
    pred = api.TableCellDetectionPredictor(det["model"], mc, api.TableCellDetectionConfig(thr, max_cells))
    try:
        got = pred.predict(imgs)
    finally:
        pred.close()
    y = det["outs"]["boxes"].reshape(len(imgs), KEEP, 6)
    total = 0
    for i, im in enumerate(imgs):
        rb, rc, rs = R.layout_postprocess(y[i], im.shape[1], im.shape[0], 1, thr, 0.5, max_cells, "rtdetr")
        assert len(got[i]) == len(rb), (i, len(got[i]), len(rb))
        for cell, b, s in zip(got[i], rb, rs):
            assert cell.label == "cell" and cell.score == float(s) and np.array_equal(cell.bbox, from_coords(b[0], b[1], b[2], b[3]))
        total += len(rb)
    assert total >= 8                                               # (the comparison is not over empty lists)
