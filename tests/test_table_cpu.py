"""Table analysis without a GPU: cells -> HTML structure (the reference's own vectors and hand-derived cases), wrap_table_html, the mode table
of TableAnalyzer with stub predictors, config validation, and the host-side model inspection of a graph that selects on the device."""
from dataclasses import dataclass

import numpy as np
import pytest

from oar_ocr_amd import api, table
from oar_ocr_amd.structure import LayoutElement, from_coords
from oar_ocr_amd.synth import models


def _boxes(*xyxy):
    return [from_coords(*b) for b in xyxy]


def _grid(order):
    return [(src, g.row, g.col, g.row_span, g.col_span) for src, g in order]


# ---------------------------------------------------------------------------------------------- the reference's own vectors
def test_reference_vector_two_by_two():
    tokens, order = table.table_cells_to_html_structure(_boxes((0, 0, 50, 20), (50, 0, 100, 20), (0, 20, 50, 40), (50, 20, 100, 40)), 5.0)
    assert tokens[0] == "<table>" and tokens[-1] == "</table>" and tokens.count("<td></td>") == 4 and len(order) == 4
    assert [(g.row, g.col) for _, g in order] == [(0, 0), (0, 1), (1, 0), (1, 1)]


def test_reference_vector_rowspan():
    tokens, order = table.table_cells_to_html_structure(_boxes((0, 0, 50, 40), (50, 0, 100, 20), (50, 20, 100, 40)), 5.0)
    assert tokens == ["<table>", "<tbody>", "<tr>", '<td rowspan="2"></td>', "<td></td>", "</tr>", "<tr>", "<td></td>", "</tr>", "</tbody>", "</table>"]
    assert _grid(order) == [(0, 0, 0, 2, 1), (1, 0, 1, 1, 1), (2, 1, 1, 1, 1)]
    assert table.wrap_table_html(tokens) == '<html><body><table><tbody><tr><td rowspan="2"></td><td></td></tr><tr><td></td></tr></tbody></table></body></html>'


# ---------------------------------------------------------------------------------------------- hand-derived cases
def test_colspan():
    # x edges 0 0 50 50 100 100 -> positions [0, 50, 100] (2 columns); y edges 0 20 20 20 40 40 -> [0, 20, 40] (2 rows).
    # box 0 spans x index 0 .. 2: col_start 0, col_end 2, col_span 2, row 0.  Boxes 1, 2: row 1, columns 0 and 1.
    tokens, order = table.table_cells_to_html_structure(_boxes((0, 0, 100, 20), (0, 20, 50, 40), (50, 20, 100, 40)), 5.0)
    assert tokens == ["<table>", "<tbody>", "<tr>", '<td colspan="2"></td>', "</tr>", "<tr>", "<td></td>", "<td></td>", "</tr>", "</tbody>", "</table>"]
    assert _grid(order) == [(0, 0, 0, 1, 2), (1, 1, 0, 1, 1), (2, 1, 1, 1, 1)]


def test_jittered_edges_inside_the_tolerance():
    # x edges sorted: 0 1 | 49 50 50 51 | 99 100 (gaps 48 and 48 split, everything else <= 5): means 0.5, 50, 99.5
    # y edges sorted: -1 0 | 19 20 21 22 | 40 41: means -0.5, 20.5, 40.5.  Every box snaps to the clean 2 x 2 grid, given in row-major order.
    boxes = _boxes((1, 0, 49, 21), (51, -1, 100, 19), (0, 20, 50, 41), (50, 22, 99, 40))
    assert table.cluster_positions([1, 49, 51, 100, 0, 50, 50, 99], 5.0) == [0.5, 50.0, 99.5]
    tokens, order = table.table_cells_to_html_structure(boxes, 5.0)
    assert tokens.count("<td></td>") == 4 and tokens.count("<tr>") == 2
    assert _grid(order) == [(0, 0, 0, 1, 1), (1, 0, 1, 1, 1), (2, 1, 0, 1, 1), (3, 1, 1, 1, 1)]


def test_chain_of_edges_links_through_the_tolerance():
    # left edges 0 4 8 12: each within 5 of the one before, so ONE cluster (mean 6) although 12 - 0 > 5; right edges 50 54 58 62 likewise (mean 56):
    # a single column.  y edges 0 20 20 40 40 60 60 80 -> 5 positions, 4 rows.  Given bottom-up: the order comes out top-down.
    boxes = _boxes((12, 60, 62, 80), (8, 40, 58, 60), (4, 20, 54, 40), (0, 0, 50, 20))
    tokens, order = table.table_cells_to_html_structure(boxes, 5.0)
    assert tokens == ["<table>", "<tbody>"] + ["<tr>", "<td></td>", "</tr>"] * 4 + ["</tbody>", "</table>"]
    assert _grid(order) == [(3, 0, 0, 1, 1), (2, 1, 0, 1, 1), (1, 2, 0, 1, 1), (0, 3, 0, 1, 1)]
    # the link is to the cluster's LAST member: 0 5 10 is one cluster (mean 5); against its first member or its mean 10 would start a new one
    assert table.cluster_positions([10, 0, 5], 5.0) == [5.0]
    assert table.cluster_positions([0, 4, 10], 5.0) == [2.0, 10.0]          # 10 - 4 = 6 > 5
    assert table.cluster_positions([], 5.0) == []
    assert all(isinstance(v, np.float32) for v in table.cluster_positions([0.1, 0.2, 7.3], 5.0))


def test_nearest_index_first_of_equal_distances_and_degenerate_inputs():
    assert table.nearest_index([0.0, 10.0], 5.0) == 0 and table.nearest_index([0.0, 10.0], 5.5) == 1 and table.nearest_index([], 1.0) == 0
    assert table.table_cells_to_html_structure([], 5.0) is None
    assert table.table_cells_to_html_structure(_boxes((0, 0, 3, 3)), 5.0) is None          # every edge in one cluster: no grid


def test_wrap_table_html():
    assert table.wrap_table_html(["<tr>", "<td></td>", "</tr>"]) == "<html><body><table><tr><td></td></tr></table></body></html>"
    # attributes split into tokens of their own (the Paddle structure dictionaries), with content
    toks = ["<tr>", "<td", ' colspan="2"', ">", "</td>", "<td></td>", "</tr>"]
    assert table.wrap_table_html(toks, ["a", None]) == '<html><body><table><tr><td colspan="2">a</td><td></td></tr></table></body></html>'


# ---------------------------------------------------------------------------------------------- TableAnalyzer with stub predictors
@dataclass
class _Cls:
    label: str
    score: float


@dataclass
class _Cell:
    bbox: np.ndarray
    score: float


class _StubClassifier:
    def __init__(self, label):
        self.label = label

    def predict(self, images):
        return [[_Cls(self.label, 0.75)] for _ in images]


class _StubDetector:
    """a 2 x 2 grid scaled to the crop, whatever the crop shows; remembers its batch sizes"""

    def __init__(self, name, cells=True):
        self.name, self.cells, self.calls = name, cells, []

    def predict(self, images):
        self.calls.append(len(images))
        out = []
        for im in images:
            h, w = im.shape[:2]
            out.append([_Cell(from_coords(x, y, x + w / 2, y + h / 2), 0.9 - 0.1 * k) for k, (x, y) in enumerate(((0, 0), (w / 2, 0), (0, h / 2), (w / 2, h / 2)))]
                       if self.cells else [])
        return out


PAGE = np.zeros((200, 300, 3), np.uint8)
TABLE = LayoutElement(from_coords(20, 30, 220, 130), "table")


@pytest.mark.parametrize("label,kind", [("wired_table", "Wired"), ("Wireless", "Wireless"), ("chart", "Unknown"), (None, "Unknown")])
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)])          # (wired, wireless) cells -> HTML
@pytest.mark.parametrize("e2e", [(False, False), (True, True)])
def test_mode_table(label, kind, flags, e2e):
    """table_analyzer.rs:406-470: cells -> HTML is on per table type (never for Unknown) and overrides E2E; without it there is no structure adapter
    to fall back on, which is the reference's configuration error"""
    generic, wired, wireless = _StubDetector("generic"), _StubDetector("wired"), _StubDetector("wireless")
    an = table.TableAnalyzer(_StubClassifier(label) if label else None, generic, wired, wireless, e2e[0], e2e[1], flags[0], flags[1])
    enabled = {"Wired": flags[0], "Wireless": flags[1], "Unknown": False}[kind]
    if not enabled:
        with pytest.raises(api.OCRError) as e:
            an.analyze_tables(PAGE, [TABLE])
        assert e.value.message == f"configuration: table_structure_recognition: table 0 ({kind}): no structure adapter available and cells->html conversion is disabled"
        return
    (res,) = an.analyze_tables(PAGE, [LayoutElement(from_coords(0, 0, 5, 5), "text"), TABLE])
    assert (wired.calls, wireless.calls, generic.calls) == (([1], [], []) if kind == "Wired" else ([], [1], []))
    assert res.table_type == kind and res.is_e2e == {"Wired": e2e[0], "Wireless": e2e[1]}[kind]
    assert res.structure_confidence == 1.0 and res.classification_confidence == 0.75 and res.detected_cell_bboxes is None
    assert res.structure_tokens == ["<table>", "<tbody>"] + ["<tr>", "<td></td>", "<td></td>", "</tr>"] * 2 + ["</tbody>", "</table>"]
    assert res.html_structure == "<html><body><table><tbody><tr><td></td><td></td></tr><tr><td></td><td></td></tr></tbody></table></body></html>"
    assert [(c.row, c.col, c.row_span, c.col_span) for c in res.cells] == [(0, 0, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 1, 1)]
    assert np.array_equal(res.cells[3].bbox, from_coords(120, 80, 220, 130)) and res.cells[3].confidence == pytest.approx(0.6)


def test_cell_detector_fallback_order():
    """:457-470: wired -> generic -> wireless for a wired table, wireless -> generic -> wired for a wireless one"""
    for label, order in (("wired_table", ("wired", "generic", "wireless")), ("wireless_table", ("wireless", "generic", "wired"))):
        for have in (order, order[1:], order[2:]):
            dets = {n: _StubDetector(n) for n in have}
            an = table.TableAnalyzer(_StubClassifier(label), dets.get("generic"), dets.get("wired"), dets.get("wireless"),
                                     use_wired_table_cells_trans_to_html=True, use_wireless_table_cells_trans_to_html=True)
            an.analyze_tables(PAGE, [TABLE])
            assert [n for n in order if n in dets and dets[n].calls] == [have[0]], (label, have)


def test_error_cases():
    on = dict(use_wired_table_cells_trans_to_html=True, use_wireless_table_cells_trans_to_html=True)
    # a detector that finds nothing, and no detector at all: the table ends without cells (:676-682)
    for det in (_StubDetector("generic", cells=False), None):
        with pytest.raises(api.OCRError) as e:
            table.TableAnalyzer(_StubClassifier("wired_table"), det, **on).analyze_tables(PAGE, [TABLE])
        assert e.value.message == "invalid input: table 0 (Wired): structure recognition produced no cells"
    # no classifier: Unknown, for which cells -> HTML is never on (:412-416) -- the configuration error of :535-543
    with pytest.raises(api.OCRError) as e:
        table.TableAnalyzer(None, _StubDetector("generic"), **on).analyze_tables(PAGE, [TABLE])
    assert "table 0 (Unknown): no structure adapter available" in e.value.message
    # the second table fails: the error names it
    outside = LayoutElement(from_coords(50, 50, 50, 80), "table")              # no pixels: BBoxCrop refuses it
    with pytest.raises(api.OCRError) as e:
        table.TableAnalyzer(_StubClassifier("wired_table"), _StubDetector("generic"), **on).analyze_tables(PAGE, [TABLE, outside])
    assert e.value.message == "adapter execution failed: table_analyzer: table 1: failed to crop table region"
    assert table.TableAnalyzer().analyze_tables(PAGE, [LayoutElement(from_coords(0, 0, 9, 9), "text")]) == []


def test_float_offsets_of_a_table_box_with_negative_x_min():
    """:347-350: the offset is the float box corner clamped at 0, not the truncated crop origin"""
    el = LayoutElement(from_coords(-5.5, 10.25, 100, 60.25), "table")              # crop = page[10:60, 0:100]
    an = table.TableAnalyzer(_StubClassifier("wired_table"), _StubDetector("generic"), use_wired_table_cells_trans_to_html=True)
    (res,) = an.analyze_tables(PAGE, [el])
    assert np.array_equal(res.cells[0].bbox, from_coords(0, 10.25, 50, 35.25)) and np.array_equal(res.cells[3].bbox, from_coords(50, 35.25, 100, 60.25))
    assert all(c.bbox.dtype == np.float32 for c in res.cells)


def test_cell_detection_is_batched_over_the_tables_of_a_page():
    det = _StubDetector("generic")
    an = table.TableAnalyzer(_StubClassifier("wired_table"), det, use_wired_table_cells_trans_to_html=True)
    els = [LayoutElement(from_coords(10 + 40 * k, 20, 45 + 40 * k, 90 + 10 * k), "table") for k in range(6)]
    res = an.analyze_tables(PAGE, els)
    assert det.calls == [4, 2] and len(res) == 6
    assert [np.array_equal(r.bbox, e.bbox) for r, e in zip(res, els)] == [True] * 6


# ---------------------------------------------------------------------------------------------- configuration, inspection
def test_config_validation():
    api.TableCellDetectionConfig().validate()
    assert (api.TableCellDetectionConfig().score_threshold, api.TableCellDetectionConfig().max_cells) == (0.3, 300)
    for bad in (api.TableCellDetectionConfig(score_threshold=1.5), api.TableCellDetectionConfig(score_threshold=-0.1),
                api.TableCellDetectionConfig(score_threshold=float("nan")), api.TableCellDetectionConfig(max_cells=0)):
        with pytest.raises(api.OCRError) as e:
            bad.validate()
        assert e.value.code == api.OAR_INVALID_INPUT
    for mc in (api.TableCellModelConfig.rtdetr_l_wired_table_cell_det(), api.TableCellModelConfig.rtdetr_l_wireless_table_cell_det()):
        assert (mc.num_classes, mc.class_labels, mc.model_type, mc.input_size) == (1, {0: "cell"}, "rtdetr", (640, 640))
    assert api.TableCellDetectionPredictor.recommended_batch_size() == 4 and api.TableClassifier.LABELS == ["wired_table", "wireless_table"]


def test_onnx_inspect_knows_the_selection_operators():
    m, info = models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24)
    text = api.onnx_inspect(m)
    assert "!" not in text
    for op in ("TopK:2", "GatherND:1", "GatherElements:1", "Gather:2"):
        assert op in text.split(), text
    assert info["anchors"] == 336 and [t["k"] for t in info["topk"]] == [40, 24]
