"""Table structure recognition end to end on the GPU: a SLANet-shaped graph (conv backbone -> Loop head), the TableStructureRecognitionPredictor over it and
TableAnalyzer's e2e mode.  The head is held to the f64 restatement of the recurrence, computed from the GPU's OWN `fea` output (the backbone has its own
tests), under the conditions of tests/test_gpu_sla_decode.py: the reference's top-1 / top-2 gap >= 8 tol, then equal tokens, then values within tol."""
import numpy as np
import pytest

from oar_ocr_amd import api, table
from oar_ocr_amd.structure import LayoutElement, crop_bounding_box, from_coords
from oar_ocr_amd.synth import models, pages
from oar_ocr_amd.synth.sla_reference import sla_reference_bundle
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu

DICT = "\n".join(["<tr>", "</tr>", "<td", ">", "</td>", ' colspan="2"', ' rowspan="2"', "<td></td>", "<tbody>", "</tbody>", "<thead>"]) + "\n"
C, H, L, M, T, SEED = 24, 40, 8, 40, 64, 3         # 64 x 64 input -> 8 x 8 = 64 positions; V = 13 follows from the dictionary


def _numpy_preprocess(img):
    """slanet.rs:72-170 restated: ResizeByLong (f32 round), Triangle filter, BGR with the ImageNet statistics in output order, zero padding after normalisation"""
    oh, ow = np.float32(img.shape[0]), np.float32(img.shape[1])
    scale = np.float32(np.float32(T) / max(oh, ow))
    rh, rw = int(np.floor(float(np.float32(oh * scale)) + 0.5)), int(np.floor(float(np.float32(ow * scale)) + 0.5))
    s, mean, std = np.float32(1) / np.float32(255), np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    t = R.normalize(R.resize_triangle(img, rw, rh), (s / std).astype(np.float32), (-mean / std).astype(np.float32), (2, 1, 0), "chw")
    out = np.zeros((3, T, T), np.float32)
    out[:, :rh, :rw] = t
    return out, np.array([oh, ow, scale, T - rh, T - rw, T], np.float32)


@pytest.fixture(scope="module")
def ctx():
    """the graph, two images of very different shapes, the engine's outputs on their preprocessed batch and the reference from its `fea`: computed once"""
    decoder = api.TableStructureDecode(DICT)
    V = len(decoder.character_dict)
    model, info = models.build_slanet(C=C, H=H, V=V, L=L, M=M, image_shape=(T, T), seed=SEED)
    imgs = [pages.make_page(5, (300, 600), 6), pages.make_page(6, (64, 40), 2)]
    pre = [_numpy_preprocess(im) for im in imgs]
    x, shape_info = np.stack([p[0] for p in pre]), [p[1] for p in pre]
    eng = api.OrtInfer(model)
    outs = eng.infer(x)
    eng.close()
    names = [n for n, _ in outs]
    outs = dict(outs)
    ref = sla_reference_bundle(info["weights"], outs["fea"], M)
    return {"model": model, "V": V, "decoder": decoder, "imgs": imgs, "x": x, "shape_info": shape_info, "names": names, "outs": outs, "ref": ref}


def test_backbone_and_head(ctx):
    outs, ref, r64 = ctx["outs"], ctx["ref"], ctx["ref"]["f64"]
    assert ctx["names"][:2] == ["bbox", "structure_probs"]                       # the reference's output order: boxes first
    assert outs["fea"].shape == (2, 64, C) and outs["bbox"].shape == (2, M, L) and outs["structure_probs"].shape == (2, M, ctx["V"])
    tol, tol_loc, tol_h = ref["tol"], ref["tol_loc"], 16 * ref["noise_h"]
    err_p = float(np.abs(outs["structure_probs"].astype(np.float64) - r64["probs"]).max())
    err_l = float(np.abs(outs["bbox"].astype(np.float64) - r64["loc"]).max())
    err_h = float(np.abs(outs["h_last"].astype(np.float64) - r64["h"]).max())
    print(f"slanet 64x64: fea std {outs['fea'].std():.2f} noise {ref['noise']:.2e} loc {ref['noise_loc']:.2e} h {ref['noise_h']:.2e} | tol {tol:.2e} / {tol_loc:.2e} / {tol_h:.2e} | "
          f"gap {ref['gap']:.2e} | gpu err probs {err_p:.2e} loc {err_l:.2e} h {err_h:.2e}")
    assert ref["gap"] >= 8 * tol, (ref["gap"], tol)
    assert np.array_equal(outs["structure_probs"].argmax(2), r64["tokens"])
    assert err_p <= tol and err_l <= tol_loc and err_h <= tol_h, (err_p, tol, err_l, tol_loc, err_h, tol_h)


def test_predictor(ctx):
    ref, decoder = ctx["ref"], ctx["decoder"]
    pred = api.TableStructureRecognitionPredictor(ctx["model"], DICT)
    try:
        assert pred.needs_padding and pred.target_size == T                      # the graph declares 64 x 64
        x, info = pred.preprocess(ctx["imgs"])
        assert x.dtype == np.float32 and np.array_equal(x, ctx["x"])
        assert len(info) == 2 and all(np.array_equal(a, b) for a, b in zip(info, ctx["shape_info"]))
        assert info[0].tolist() == [300.0, 600.0, np.float32(64.0) / np.float32(600.0), 32.0, 0.0, 64.0] and info[1].tolist() == [64.0, 40.0, 1.0, 0.0, 24.0, 64.0]
        got = pred.predict(ctx["imgs"])
    finally:
        pred.close()
    # the Python decode of the REFERENCE tensors
    want_tokens, want_boxes, want_scores = decoder.decode(ref["f64"]["probs"].astype(np.float32), ref["f64"]["loc"].astype(np.float32), ctx["shape_info"])
    assert ref["gap"] >= 8 * ref["tol"]
    assert sum(len(b) for b in want_boxes) > 0 and sum(len(t) for t in want_tokens) > 0       # the case decodes something
    for i, im in enumerate(ctx["imgs"]):
        longest = float(max(im.shape[:2]))
        assert got.structures[i] == want_tokens[i]
        assert len(got.bboxes[i]) == len(want_boxes[i])
        for a, b in zip(got.bboxes[i], want_boxes[i]):
            assert a.shape == (8,) and np.abs(a.astype(np.float64) - b).max() <= ref["tol_loc"] * longest, (a, b)
            assert np.all(a[0::2] <= im.shape[1]) and np.all(a[1::2] <= im.shape[0]) and np.all(a >= 0)
        assert abs(got.structure_scores[i] - float(want_scores[i])) <= ref["tol"]
    print("predictor:", [len(t) for t in got.structures], [len(b) for b in got.bboxes], got.structure_scores)


def test_analyzer_e2e_mode(ctx):
    page = pages.make_page(7, (200, 260), 6)
    el = LayoutElement(bbox=from_coords(30.0, 20.0, 230.0, 180.0), element_type="table")
    pred = api.TableStructureRecognitionPredictor(ctx["model"], DICT)
    try:
        direct = pred.predict([crop_bounding_box(page, el.bbox)])
        res = table.TableAnalyzer(table_structure_recognizer=pred, use_e2e_wireless_table_rec=True).analyze_tables(page, [el])
    finally:
        pred.close()
    assert len(res) == 1
    r = res[0]
    assert r.is_e2e and r.table_type == table.UNKNOWN and r.detected_cell_bboxes is None
    assert r.structure_tokens == direct.structures[0] and len(r.structure_tokens) > 0
    assert len(r.cells) == len(direct.bboxes[0]) and len(r.cells) >= 1
    grid = table.parse_cell_grid_info(r.structure_tokens)
    for c, g, b in zip(r.cells, grid, direct.bboxes[0]):
        assert (c.row, c.col, c.row_span, c.col_span) == (g.row, g.col, g.row_span, g.col_span) and c.confidence == 1.0
        assert np.allclose(c.bbox[:, 0].min(), b[0::2].min() + 30.0) and np.allclose(c.bbox[:, 1].min(), b[1::2].min() + 20.0)      # crop -> page coordinates
    assert r.html_structure == table.wrap_table_html(r.structure_tokens) and r.html_structure.startswith("<html><body><table>")
    assert r.structure_confidence == pytest.approx(direct.structure_scores[0])
