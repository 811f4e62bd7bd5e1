"""Table structure recognition, host side: the reference's own unit vectors for the decoder and the grid parser (processors/table_structure_decode.rs tests),
the decode rules around eos and truncation, TableAnalyzer's structure-recognizer branches with fake predictors, the ONNX parser on a nested graph, and the
register budget of the fused decode kernel."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from oar_ocr_amd import api, table
from oar_ocr_amd.structure import LayoutElement, aabb, from_coords
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.onnx_writer import BOOL, INT64, GraphBuilder

DICT = "<html>\n<body>\n<table>\n<tr>\n<td>\n<td\n colspan=\"4\"  \n>\n</td>\n</tr>\n</table>\n</body>\n</html>\n\n"


# ------------------------------------------------------------------------------------------------ dictionary and decode
def test_dictionary_processing():
    d = api.TableStructureDecode(DICT)
    assert d.character_dict[0] == "sos" and d.character_dict[-1] == "eos" and d.end_idx == len(d.character_dict) - 1
    assert "<td>" not in d.character_dict and d.character_dict[-2] == "<td></td>"
    assert ' colspan="4"' in d.character_dict                       # trailing blanks trimmed, the leading one kept
    assert "<html>" in d.character_dict and "<td" in d.character_dict and "" not in d.character_dict
    assert d.ignored_tokens == [0, d.end_idx]
    assert d.td_token_indices == [d.character_dict.index("<td"), d.character_dict.index("<td></td>")]
    # a dictionary that already has <td></td> gets no second one
    assert api.TableStructureDecode("<tr>\n<td></td>\n</tr>\n").character_dict == ["sos", "<tr>", "<td></td>", "</tr>", "eos"]


def _scores(d, token_names, V=None, peak=0.9):
    V = V or len(d.character_dict)
    x = np.full((1, len(token_names), V), (1.0 - peak) / (V - 1), np.float32)
    for t, name in enumerate(token_names):
        x[0, t, d.character_dict.index(name) if isinstance(name, str) else name] = peak
    return x


def test_all_zero_scores_pick_the_first_token():
    assert api.TableStructureDecode.argmax_at(np.zeros(50, np.float32)) == (0, 0.0)
    assert api.TableStructureDecode.argmax_at(np.array([1.0, 3.0, 3.0, np.nan], np.float32))[0] == 1


def test_eos_stops_only_after_the_first_step():
    d = api.TableStructureDecode(DICT)
    shape = [np.array([100, 200, 2.56, 0, 0, 512], np.float32)]
    box = np.tile(np.linspace(0.1, 0.8, 8, dtype=np.float32), (1, 6, 1))
    # eos at step 0 is skipped like sos, not a stop
    tokens, boxes, scores = d.decode(_scores(d, ["eos", "<tr>", "<td></td>", "</tr>", "eos", "<tr>"]), box, shape)
    assert tokens[0] == ["<tr>", "<td></td>", "</tr>"] and len(boxes[0]) == 1
    assert scores[0] == np.float32(np.float32(np.float32(0.9) + np.float32(0.9)) + np.float32(0.9)) / np.float32(3)
    tokens, boxes, scores = d.decode(_scores(d, ["sos", "<tr>", "sos", "<td", "eos", "<tr>"]), box, shape)
    assert tokens[0] == ["<tr>", "<td"] and len(boxes[0]) == 1
    tokens, boxes, scores = d.decode(_scores(d, ["sos", "eos"]), box[:, :2], shape)
    assert tokens[0] == [] and boxes[0] == [] and scores[0] == 0.0
    # an index past the dictionary is spelled UNK_<index>
    tokens, _, _ = d.decode(_scores(d, [len(d.character_dict) + 2], V=len(d.character_dict) + 4), box[:, :1], shape)
    assert tokens[0] == [f"UNK_{len(d.character_dict) + 2}"]


def test_extract_bbox_scales_by_the_longest_side_portrait_case():
    preds = np.array([0.45, 0.25, 0.9, 0.25, 0.45, 0.8, 0.9, 0.8], np.float32)
    orig_h, orig_w, target = np.float32(600), np.float32(300), np.float32(512)
    scale = target / max(orig_h, orig_w)
    shape = [np.array([orig_h, orig_w, scale, 0.0, target - orig_w * scale, target], np.float32)]
    got = api.TableStructureDecode.extract_bbox(preds.reshape(1, 1, 8), 0, 0, shape)
    want = [min(max(p * 600.0, 0.0), 300.0 if i % 2 == 0 else 600.0) for i, p in enumerate(preds)]
    assert got.dtype == np.float32 and np.abs(got - np.array(want, np.float32)).max() < 1e-3
    assert got[2] == 300.0 and got[6] == 300.0                        # 0.9 * 600 clamps to the width
    with pytest.raises(api.OCRError):
        api.TableStructureDecode.extract_bbox(preds.reshape(1, 1, 8), 0, 0, [np.array([600, 300, 0.0, 0, 0, 512], np.float32)])


class _FakeEngine:
    def __init__(self, outs):
        self.outs = outs

    def infer(self, x):
        return self.outs

    def close(self):
        pass


def test_max_structure_length_truncates_tokens_and_boxes():
    d = api.TableStructureDecode(DICT)
    names = ["sos", "<tr>", "<td></td>", "<td></td>", "</tr>", "<tr>", "<td></td>", "</tr>", "eos"]
    p = api.TableStructureRecognitionPredictor.__new__(api.TableStructureRecognitionPredictor)
    p.config, p.decoder = api.TableStructureRecognitionConfig(), d
    p._eng = _FakeEngine([("bbox", np.full((1, len(names), 8), 0.5, np.float32)), ("probs", _scores(d, names))])
    p.preprocess = lambda images: (np.zeros((1, 3, 8, 8), np.float32), [np.array([40, 64, 0.125, 0, 0, 8], np.float32)])
    full = p.predict([np.zeros((40, 64, 3), np.uint8)])
    assert full.structures[0] == names[1:-1] and len(full.bboxes[0]) == 3 and np.allclose(full.bboxes[0][0], [32, 32] * 4)
    cut = p.predict([np.zeros((40, 64, 3), np.uint8)], api.TableStructureRecognitionConfig(max_structure_length=2))
    assert cut.structures[0] == ["<tr>", "<td></td>"] and len(cut.bboxes[0]) == 2          # take(len(tokens)) of the boxes, like the adapter
    low = p.predict([np.zeros((40, 64, 3), np.uint8)], api.TableStructureRecognitionConfig(score_threshold=0.99))
    assert low.structures[0] == full.structures[0] and low.structure_scores[0] < 0.99      # below the threshold: kept
    with pytest.raises(api.OCRError):
        p.predict([])
    assert api.TableStructureRecognitionPredictor.recommended_batch_size() == 8


# ------------------------------------------------------------------------------------------------ tokens -> grid
def _grid(tokens):
    return [(g.row, g.col, g.row_span, g.col_span) for g in table.parse_cell_grid_info(tokens)]


def test_parse_cell_grid_info_simple():
    assert _grid(["<tr>", "<td></td>", "<td></td>", "</tr>", "<tr>", "<td></td>", "<td></td>", "</tr>"]) == [(0, 0, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 1, 1)]


def test_parse_cell_grid_info_colspan():
    assert _grid(["<tr>", '<td colspan="2"></td>', "</tr>", "<tr>", "<td></td>", "<td></td>", "</tr>"]) == [(0, 0, 1, 2), (1, 0, 1, 1), (1, 1, 1, 1)]


def test_parse_cell_grid_info_rowspan():
    assert _grid(["<tr>", '<td rowspan="2"></td>', "<td></td>", "</tr>", "<tr>", "<td></td>", "</tr>"]) == [(0, 0, 2, 1), (0, 1, 1, 1), (1, 1, 1, 1)]


def test_parse_cell_grid_info_split_tokens_with_spans():
    tokens = ["<tr>", "<td", ' colspan="2"', ">", "</td>", "</tr>", "<tr>", "<td", ' rowspan="2"', ">", "</td>", "<td></td>", "</tr>", "<tr>", "<td></td>", "</tr>"]
    assert _grid(tokens) == [(0, 0, 1, 2), (1, 0, 2, 1), (1, 1, 1, 1), (2, 1, 1, 1)]


def test_parse_cell_grid_info_ignores_everything_else():
    assert _grid(["<table>", "<tbody>", "<tr>", "<td></td>", "</tr>", "</tbody>", "</table>"]) == [(0, 0, 1, 1)]
    assert _grid([]) == []


def test_wrap_table_html_with_split_tokens_and_content():
    html = table.wrap_table_html(["<tr>", "<td", ' colspan="2"', ">", "</td>", "</tr>"], ["Cell A"])
    assert '<td colspan="2">Cell A</td>' in html and html.startswith("<html><body><table>") and html.endswith("</table></body></html>")


def test_parse_span_attr():
    f = table.parse_span_attr
    assert f('<td colspan="2">', "colspan") == 2 and f('<td rowspan="3">', "rowspan") == 3
    assert f('<td colspan="2" rowspan="3">', "colspan") == 2 and f('<td colspan="2" rowspan="3">', "rowspan") == 3
    assert f("<td></td>", "colspan") is None and f("<td>", "rowspan") is None
    assert f('<td colspan="x">', "colspan") is None and f('<td colspan="2', "colspan") is None


# ------------------------------------------------------------------------------------------------ TableAnalyzer with a structure recognizer
PAGE = np.full((120, 160, 3), 255, np.uint8)
ELEMENT = LayoutElement(bbox=from_coords(10.0, 20.0, 110.0, 100.0), element_type="table")
TOKENS = ["<tr>", "<td></td>", "<td", ' colspan="2"', ">", "</td>", "</tr>"]
BOXES = [np.array([0, 0, 40, 0, 40, 30, 0, 30], np.float32), np.array([40, 2, 99, 0, 100, 30, 41, 29], np.float32)]


class _Recognizer:
    def __init__(self, name, log, fail=False, empty=False):
        self.name, self.log, self.fail, self.empty = name, log, fail, empty

    def predict(self, images):
        self.log.append(self.name)
        if self.fail:
            raise api.OCRError(api.OAR_DEVICE, "device lost")
        if self.empty:
            return api.TableStructureRecognitionOutput([], [], [])
        return api.TableStructureRecognitionOutput([list(TOKENS)], [list(BOXES)], [0.75])


class _Classifier:
    def __init__(self, label):
        self.label = label

    def predict(self, images):
        return [[SimpleNamespace(label=self.label, score=0.8)]]


class _CellDetector:
    def __init__(self, log=None, cells=None):
        self.log = log if log is not None else []
        self.cells = cells if cells is not None else [SimpleNamespace(bbox=from_coords(x, y, x + 40.0, y + 30.0), score=0.6) for y in (0.0, 30.0) for x in (0.0, 40.0)]

    def predict(self, images):
        self.log.append("cells")
        return [list(self.cells) for _ in images]


def test_recognized_structure_becomes_cells_with_grid_positions():
    log = []
    a = table.TableAnalyzer(table_structure_recognizer=_Recognizer("any", log), use_e2e_wireless_table_rec=True)
    r = a.analyze_tables(PAGE, [ELEMENT])[0]
    assert log == ["any"] and r.table_type == table.UNKNOWN and r.is_e2e and r.structure_tokens == TOKENS
    assert r.structure_confidence == 0.75 and r.detected_cell_bboxes is None
    assert [(c.row, c.col, c.row_span, c.col_span, c.confidence) for c in r.cells] == [(0, 0, 1, 1, 1.0), (0, 1, 1, 2, 1.0)]
    assert aabb(r.cells[0].bbox) == (10.0, 20.0, 50.0, 50.0) and aabb(r.cells[1].bbox) == (50.0, 20.0, 110.0, 50.0)     # the quad's extremes, moved to the page
    assert r.html_structure == '<html><body><table><tr><td></td><td colspan="2"></td></tr></table></body></html>'


@pytest.mark.parametrize("label, want", [("wired_table", "wired"), ("wireless_table", "wireless"), ("other", "any")])
def test_recognizer_fallback_order(label, want):
    log = []
    rec = {k: _Recognizer(k, log) for k in ("any", "wired", "wireless")}
    a = table.TableAnalyzer(table_classifier=_Classifier(label), table_structure_recognizer=rec["any"], wired_table_structure_recognizer=rec["wired"],
                            wireless_table_structure_recognizer=rec["wireless"], use_e2e_wired_table_rec=True, use_e2e_wireless_table_rec=True)
    a.analyze_tables(PAGE, [ELEMENT])
    assert log == [want]
    # without the preferred one: wired -> the generic one; unknown -> wireless before wired; and a wireless table never takes the wired recognizer
    log.clear()
    b = table.TableAnalyzer(table_classifier=_Classifier(label), table_structure_recognizer=None if label == "other" else rec["any"],
                            wired_table_structure_recognizer=rec["wired"] if label == "other" else None,
                            wireless_table_structure_recognizer=rec["wireless"] if label == "other" else None, use_e2e_wired_table_rec=True, use_e2e_wireless_table_rec=True)
    b.analyze_tables(PAGE, [ELEMENT])
    assert log == ["wireless" if label == "other" else "any"]
    c = table.TableAnalyzer(table_classifier=_Classifier("wireless_table"), wired_table_structure_recognizer=rec["wired"], use_e2e_wireless_table_rec=True)
    with pytest.raises(api.OCRError, match="no structure adapter available"):
        c.analyze_tables(PAGE, [ELEMENT])


def test_failing_recognizer_is_surfaced_unless_cells_to_html_stands_in():
    a = table.TableAnalyzer(table_structure_recognizer=_Recognizer("any", [], fail=True), use_e2e_wireless_table_rec=True)
    with pytest.raises(api.OCRError) as ex:
        a.analyze_tables(PAGE, [ELEMENT])
    assert "table_structure_recognition: table 0 (Unknown): structure recognition failed" in str(ex.value) and "device lost" in str(ex.value)
    # cells -> HTML: the detected cells carry the table
    b = table.TableAnalyzer(table_classifier=_Classifier("wired_table"), table_structure_recognizer=_Recognizer("any", [], fail=True), table_cell_detector=_CellDetector(),
                            use_wired_table_cells_trans_to_html=True)
    r = b.analyze_tables(PAGE, [ELEMENT])[0]
    assert len(r.cells) == 4 and r.structure_confidence == 1.0 and r.structure_tokens.count("<td></td>") == 4
    # a recognizer that answers without a payload leaves no cells
    c = table.TableAnalyzer(table_structure_recognizer=_Recognizer("any", [], empty=True), use_e2e_wireless_table_rec=True)
    with pytest.raises(api.OCRError, match="structure recognition produced no cells"):
        c.analyze_tables(PAGE, [ELEMENT])


def test_cells_to_html_overrides_the_recognized_structure_but_keeps_its_score():
    a = table.TableAnalyzer(table_classifier=_Classifier("wired_table"), table_structure_recognizer=_Recognizer("any", []), table_cell_detector=_CellDetector(),
                            use_wired_table_cells_trans_to_html=True, use_e2e_wired_table_rec=True)
    r = a.analyze_tables(PAGE, [ELEMENT])[0]
    assert len(r.cells) == 4 and [c.confidence for c in r.cells] == [0.6] * 4 and r.structure_confidence == 0.75 and r.detected_cell_bboxes is None
    assert r.structure_tokens[:3] == ["<table>", "<tbody>", "<tr>"]


def test_detected_cell_bboxes_only_in_the_non_e2e_mode():
    log = []
    det = _CellDetector(log)
    a = table.TableAnalyzer(table_structure_recognizer=_Recognizer("any", []), table_cell_detector=det)              # e2e off: the detector runs, its boxes travel along
    r = a.analyze_tables(PAGE, [ELEMENT])[0]
    assert log == ["cells"] and not r.is_e2e and r.structure_tokens == TOKENS and len(r.cells) == 2
    assert len(r.detected_cell_bboxes) == 4 and aabb(r.detected_cell_bboxes[3]) == (50.0, 50.0, 90.0, 80.0)
    log.clear()
    b = table.TableAnalyzer(table_structure_recognizer=_Recognizer("any", []), table_cell_detector=det, use_e2e_wireless_table_rec=True)
    r = b.analyze_tables(PAGE, [ELEMENT])[0]
    assert log == [] and r.is_e2e and r.detected_cell_bboxes is None                                                 # e2e: no cell detection at all
    c = table.TableAnalyzer(table_structure_recognizer=_Recognizer("any", []), table_cell_detector=_CellDetector(cells=[]))
    assert c.analyze_tables(PAGE, [ELEMENT])[0].detected_cell_bboxes is None                                         # nothing detected: nothing attached


def test_without_recognizers_nothing_changes():
    with pytest.raises(api.OCRError, match="no structure adapter available and cells->html conversion is disabled"):
        table.TableAnalyzer(table_cell_detector=_CellDetector()).analyze_tables(PAGE, [ELEMENT])
    a = table.TableAnalyzer(table_classifier=_Classifier("wired_table"), table_cell_detector=_CellDetector(), use_wired_table_cells_trans_to_html=True)
    r = a.analyze_tables(PAGE, [ELEMENT])[0]
    assert len(r.cells) == 4 and r.structure_confidence == 1.0 and r.detected_cell_bboxes is None and not r.is_e2e


# ------------------------------------------------------------------------------------------------ ONNX: graph-valued attributes
def test_parser_reads_nested_graphs_written_by_the_writer():
    inner = GraphBuilder("inner")
    inner.add_input("j", [], INT64)
    inner.add_input("c_in", [], BOOL)
    inner.add_input("v", [2])
    inner.op("Identity", ["c_in"], outputs=["c_out"])
    inner.op("Relu", ["v"], outputs=["v_out"])
    inner.add_output("c_out", [], BOOL)
    inner.add_output("v_out", [2])
    mid = GraphBuilder("mid")
    mid.add_input("i", [], INT64)
    mid.add_input("cond_in", [], BOOL)
    mid.add_input("acc", [2])
    mid.op("Identity", ["cond_in"], outputs=["cond_out"])
    t = mid.op("Add", ["acc", mid.init(np.ones(2, np.float32), "one")])
    mid.op("Loop", [mid.init(np.array(2, np.int64), "trip"), mid.init(np.array(True), "t"), t], outputs=["acc_new"], body=inner)
    mid.add_output("cond_out", [], BOOL)
    mid.add_output("acc_new", [2])
    g = GraphBuilder("outer")
    g.add_input("x", [2])
    g.op("Loop", [g.init(np.array(3, np.int64), "trip"), g.init(np.array(True), "cond"), "x"], outputs=["y"], body=mid)
    g.add_output("y", [2])
    text = api.onnx_inspect(g.model())
    assert "nodes=1 | Loop:1" in text
    assert "Loop.body{inputs=i,cond_in,acc outputs=cond_out,acc_new initializers=3 nodes=3: Add:1 Identity:1 Loop:1}" in text
    assert "Loop.body{inputs=j,c_in,v outputs=c_out,v_out initializers=0 nodes=2: Identity:1 Relu:1}" in text           # the body of the body
    # a graph without graph attributes is reported exactly as before
    flat, _ = models.build_cls()
    assert "{" not in api.onnx_inspect(flat)
    # the SLA graph: the body's interface and its weights arrive
    m, info = models.build_slanet(C=20, H=24, V=11, L=4, M=5, head_only=True)
    text = api.onnx_inspect(m)
    assert "Loop.body{inputs=sla_i,sla_cond_in,sla_h,sla_pre outputs=sla_cond_out,sla_h_new,sla_pre_new,sla_logits,sla_loc initializers=20 nodes=33:" in text
    assert set(info["weights"]) == set(models.SLA_WEIGHT_NAMES)
    # a truncated nested graph is a load error, not a crash
    blob = g.model()
    with pytest.raises(api.OCRError):
        api.onnx_inspect(blob[:len(blob) // 2])


# ------------------------------------------------------------------------------------------------ the fused decode kernel's resources
def test_sla_decode_kernel_fits_its_1024_thread_workgroup():
    """sla_decode.hip: one 1024-thread workgroup per image = 4 waves per SIMD = at most 128 registers, nothing spilled, no scratch (a spill inside the
    501-step loop would be paid on every step)"""
    from oar_ocr_amd import build
    src = build.CSRC / "sla_decode.hip"
    r = subprocess.run([build.HIPCC] + build.FLAGS + ["-c", str(src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    decode = {k: v for k, v in kernels.items() if "sla_decode_kernel" in k}
    assert len(decode) == 1, kernels
    for k, v in decode.items():
        threads = int(re.search(r"kSlaThreads = (\d+)", src.read_text()).group(1))
        assert threads in (512, 1024)
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgprs"] <= (128 if threads == 1024 else 256), (k, v)
