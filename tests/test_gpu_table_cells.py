"""Table cell detection on the GPU: a synthetic RT-DETR-shaped graph whose query selection (TopK, GatherND, GatherElements, tensor-indexed Gather)
runs in the engine, the TableCellDetectionPredictor over it, and TableAnalyzer's cells -> HTML branch with real predictors.

oracle.onnx_ref cannot evaluate TopK, so the graph declares every TopK's input and index output: each selection is checked EXACTLY against the
stable numpy selection applied to the engine's own TopK input, and the float segments between the selections are evaluated by onnx_ref with the
engine's indices fed through numpy gathers."""
import numpy as np
import pytest

from oar_ocr_amd import api, table
from oar_ocr_amd.structure import LayoutElement, from_coords
from oar_ocr_amd.synth import models, pages
from oracle import cpu_ref as R
from oracle import onnx_ref

pytestmark = pytest.mark.gpu

SHAPE, QUERIES, KEEP = (128, 128), 40, 24      # 336 anchors: neither selection is trivial, neither row length a power of two
RTDETR_PRE = dict(filter="triangle", scale=1.0 / 255.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), bgr=True)


@pytest.fixture(scope="module")
def ctx():
    """the graph, three pages of different sizes, the engine's declared outputs on them -- computed once, never modified"""
    m, info = models.build_table_cell_det(image_shape=SHAPE, queries=QUERIES, keep=KEEP)
    imgs = [pages.make_page(30 + i, (200 + 60 * i, 260 - 30 * i), 6 + i) for i in range(3)]
    x = np.stack([R.layout_preprocess(im, SHAPE, **RTDETR_PRE)[0] for im in imgs])
    feeds = {"image": x,
             "scale_factor": np.array([[np.float32(SHAPE[0]) / np.float32(im.shape[0]), np.float32(SHAPE[1]) / np.float32(im.shape[1])] for im in imgs], np.float32),
             "im_shape": np.array([[SHAPE[0], SHAPE[1]]] * len(imgs), np.float32)}
    eng = api.OrtInfer(m)
    outs = dict(eng.infer([(k, feeds[k]) for k in ("image", "scale_factor", "im_shape")]))
    eng.close()
    return {"model": m, "info": info, "imgs": imgs, "feeds": feeds, "outs": outs}


def _segments_with_engine_indices(model, feeds, engine_idx):
    """every float segment through onnx_ref; TopK takes the ENGINE's indices, the gathers are numpy's"""
    env = dict(feeds)
    seg = []

    def flush():
        if seg:
            outs = [nd["outputs"][0] for nd in seg]
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


def test_each_selection_is_the_stable_selection_of_its_own_input(ctx):
    for t in ctx["info"]["topk"]:
        x, idx = ctx["outs"][t["input"]], ctx["outs"][t["index"]]
        assert idx.dtype == np.int64 and idx.shape == (3, t["k"]) and x.dtype == np.float32
        assert np.array_equal(idx, np.argsort(-x, axis=-1, kind="stable")[:, :t["k"]]), t
    enc = ctx["outs"][ctx["info"]["topk"][0]["input"]]
    assert enc.shape == (3, 336)


def test_float_segments_agree_with_the_reference_evaluator(ctx):
    """2e-4 * max(1, |ref|max): the tolerance tests/test_gpu_engine.py holds the engine to"""
    info, outs = ctx["info"], ctx["outs"]
    env = _segments_with_engine_indices(onnx_ref.parse_model(ctx["model"]), ctx["feeds"], {t["index"]: outs[t["index"]] for t in info["topk"]})
    for name in [t["input"] for t in info["topk"]] + ["boxes"]:
        ref, got = env[name], outs[name]
        err, bound = np.abs(got - ref).max(), 2e-4 * max(1.0, np.abs(ref).max())
        print(name, ref.shape, "max abs err", err, "bound", bound)
        assert got.shape == ref.shape and err <= bound, (name, err, bound)
    assert outs["boxes"].shape == (3 * KEEP, 6)
    sc = outs["boxes"].reshape(3, KEEP, 6)[..., 1]
    assert np.all(sc[:, :-1] >= sc[:, 1:])                                                     # sorted by score, like the real export


def _filtered(boxes, classes, scores, thr, cap):
    """the adapter's per-call filter (table_cell_detection_adapter.rs:107-127)"""
    out = []
    for b, c, s in zip(boxes, classes, scores):
        if s < np.float32(thr):
            continue
        out.append((b, s))
        if len(out) >= cap:
            break
    return out


@pytest.mark.parametrize("max_cells,call_thr", [(300, None), (5, None), (300, 0.44)])
def test_predictor_equals_layout_postprocess_of_the_engines_rows(ctx, max_cells, call_thr):
    imgs, thr = ctx["imgs"], 0.3
    mc = api.TableCellModelConfig("synthetic_cell_det", 1, {0: "cell"}, "rtdetr", SHAPE)
    pred = api.TableCellDetectionPredictor(ctx["model"], mc, api.TableCellDetectionConfig(thr, max_cells))
    for i, im in enumerate(imgs):
        assert np.array_equal(pred.preprocess(im), ctx["feeds"]["image"][i]), i                # bit-equal to layout_preprocess with RT-DETR's settings
    call = api.TableCellDetectionConfig(call_thr, max_cells) if call_thr is not None else None
    got = pred.predict(imgs, call)
    y = ctx["outs"]["boxes"].reshape(len(imgs), KEEP, 6)
    dropped = 0
    for i, im in enumerate(imgs):
        rb, rc, rs = R.layout_postprocess(y[i], im.shape[1], im.shape[0], 1, thr, 0.5, max_cells, "rtdetr")
        want = _filtered(rb, rc, rs, call_thr if call_thr is not None else thr, max_cells)
        dropped += len(rb) - len(want)
        assert len(got[i]) == len(want), (i, len(got[i]), len(want))
        for cell, (b, s) in zip(got[i], want):
            assert cell.label == "cell" and cell.score == float(s) and np.array_equal(cell.bbox, from_coords(b[0], b[1], b[2], b[3]))
        assert len(got[i]) == 5 if max_cells == 5 else len(got[i]) >= (8 if call_thr is None else 1), (i, len(got[i]))
    if call_thr is not None:
        assert dropped > 0                                                                      # the per-call threshold really drops cells
    pred.close()


def test_table_analyzer_with_real_predictors(ctx):
    page = pages.make_page(41, (420, 360), 16)
    els = [LayoutElement(from_coords(12.5, 20.0, 300.0, 190.0), "table"), LayoutElement(from_coords(5, 5, 50, 15), "text"),
           LayoutElement(from_coords(40.0, 210.25, 330.0, 400.0), "table")]
    cls_model, _ = models.build_cls(n_classes=2, seed=9)
    classifier = api.TableClassifier(cls_model)
    det = api.TableCellDetectionPredictor(ctx["model"], api.TableCellModelConfig("synthetic_cell_det", 1, {0: "cell"}, "rtdetr", SHAPE))
    an = table.TableAnalyzer(classifier, det, use_wired_table_cells_trans_to_html=True, use_wireless_table_cells_trans_to_html=True)
    res = an.analyze_tables(page, els)
    assert len(res) == 2
    crops = [page[int(el.bbox[0, 1]):int(el.bbox[2, 1]), int(el.bbox[0, 0]):int(el.bbox[2, 0])] for el in (els[0], els[2])]
    per_crop = det.predict(crops)                                  # one batch, as the analyzer runs the tables of a page
    for r, el, crop, cells in zip(res, (els[0], els[2]), crops, per_crop):
        x0, y0 = el.bbox[0]
        assert len(cells) >= 8
        off = np.array([x0, y0], np.float32)
        # the analyzer builds the structure from the page boxes moved back by the float offset (table_analyzer.rs:644-654): the same round trip here.
        # The reference applies table_cells_to_html_structure TWICE in this mode -- once because the cells have no tokens yet (:641-674), once because
        # cells -> HTML is on (:684-717) -- and the second pass sees only the cells the first one placed, in row-major order.  Overlapping detections
        # lose cells in the first pass, so the second one clusters fewer edges and is not a repeat of the first: the test applies it twice as well.
        boxes = [((c.bbox + off).astype(np.float32) - off).astype(np.float32) for c in cells]
        _, first = table.table_cells_to_html_structure(boxes, 5.0)
        tokens, second = table.table_cells_to_html_structure([boxes[src] for src, _ in first], 5.0)
        order = [(first[src][0], g) for src, g in second]           # back to indices into the predictor's cells
        assert r.structure_tokens == tokens and len(r.cells) == len(order)
        for c, (src, g) in zip(r.cells, order):
            assert (c.row, c.col, c.row_span, c.col_span) == (g.row, g.col, g.row_span, g.col_span)
            assert np.array_equal(c.bbox, (cells[src].bbox + off).astype(np.float32)) and c.confidence == cells[src].score
        assert all(c.row is not None and c.col is not None for c in r.cells)
        assert r.html_structure.startswith("<html><body><table>") and r.html_structure.endswith("</table></body></html>")
        assert r.html_structure == table.wrap_table_html(tokens)
        assert r.table_type in ("Wired", "Wireless") and r.structure_confidence == 1.0 and r.classification_confidence is not None and not r.is_e2e
        assert r.classification_confidence == classifier.predict([crop])[0][0].score
    det.close()
    classifier.close()
