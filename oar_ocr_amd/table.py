"""Table analysis: `TableAnalyzer` (src/oarocr/table_analyzer.rs) with its cells -> HTML mode and, when a structure recognizer is given, the SLANet mode.

A table becomes HTML from the table classifier and the cell detector alone (`use_wired_table_cells_trans_to_html` /
`use_wireless_table_cells_trans_to_html`): `table_cells_to_html_structure` rebuilds rows, columns and spans from the detected cell boxes
(table_analyzer.rs:79-265) and `wrap_table_html` renders the tokens (processors/table_structure_decode.rs:37-160).

Host orchestration only: crops come from `structure.crop_bounding_box`, classification and cell detection run through the C-ABI predictors of
`api.py` (the cell detector over all tables of a page in batches of its recommended size, not one call per table).  All coordinate arithmetic is f32
in the reference's operation order.  Where the reference needs a structure adapter (:535-543) or ends without cells (:676-682) this module raises
`api.OCRError` with the reference's message.  With a structure recognizer (`api.TableStructureRecognitionPredictor`: the SLANet family, whose decode
loop the engine runs as one launch) the cells come from the recognized structure tokens and boxes (:481-584), `parse_cell_grid_info` gives them their
grid positions, and in the non-e2e mode the cell detector's boxes travel along as `detected_cell_bboxes` (:625-639).  Table orientation correction is
not part of this module."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import api
from .structure import F, aabb, crop_bounding_box, from_coords

WIRED, WIRELESS, UNKNOWN = "Wired", "Wireless", "Unknown"    # TableType, spelled as its Debug form (the error messages print it)


@dataclass
class CellGridInfo:
    """processors/table_structure_decode.rs:165-176"""
    row: int
    col: int
    row_span: int = 1
    col_span: int = 1


@dataclass
class TableCell:
    """domain/structure.rs TableCell: `bbox` [4, 2] f32 in page coordinates"""
    bbox: np.ndarray
    confidence: float
    row: Optional[int] = None
    col: Optional[int] = None
    row_span: Optional[int] = None
    col_span: Optional[int] = None
    text: Optional[str] = None


@dataclass
class TableResult:
    """domain/structure.rs TableResult, the fields this branch fills"""
    bbox: np.ndarray
    table_type: str
    cells: List[TableCell] = field(default_factory=list)
    html_structure: Optional[str] = None
    structure_tokens: Optional[List[str]] = None
    is_e2e: bool = False
    structure_confidence: Optional[float] = None
    classification_confidence: Optional[float] = None
    detected_cell_bboxes: Optional[List[np.ndarray]] = None


# ------------------------------------------------------------------------------------------------ cells -> structure tokens
def cluster_positions(positions: Sequence[float], tolerance: float) -> List[np.float32]:
    """table_analyzer.rs:79-105: sorted positions are chain-linked -- a position joins the current cluster when it lies within `tolerance` of the
    cluster's LAST member -- and a cluster is represented by the f32 mean of its members, summed in order."""
    if len(positions) == 0:
        return []
    pos = sorted(F(p) for p in positions)
    tol = F(tolerance)

    def mean(c):
        s = F(0.0)
        for v in c:
            s = F(s + v)
        return F(s / F(len(c)))

    out, cur = [], [pos[0]]
    for p in pos[1:]:
        if np.abs(F(p - cur[-1])) <= tol:
            cur.append(p)
        else:
            out.append(mean(cur))
            cur = [p]
    out.append(mean(cur))
    return out


def nearest_index(positions: Sequence[float], value: float) -> int:
    """table_analyzer.rs:107-118 (Iterator::min_by returns the FIRST of equal minima)"""
    best, best_d = 0, None
    for i, p in enumerate(positions):
        d = np.abs(F(F(p) - F(value)))
        if best_d is None or d < best_d:
            best, best_d = i, d
    return best


def table_cells_to_html_structure(cell_bboxes: Sequence[np.ndarray], tolerance: float = 5.0) -> Optional[Tuple[List[str], List[Tuple[int, CellGridInfo]]]]:
    """table_analyzer.rs:147-265: PaddleX-like structure tokens from cell boxes, and the row-major cell order those tokens imply as
    (index into `cell_bboxes`, grid info).  None where the reference returns None."""
    if len(cell_bboxes) == 0:
        return None
    xs, ys, boxes = [], [], []
    for b in cell_bboxes:
        x0, y0, x1, y1 = aabb(b)
        boxes.append((x0, y0, x1, y1))
        xs += [x0, x1]
        ys += [y0, y1]
    xp, yp = cluster_positions(xs, tolerance), cluster_positions(ys, tolerance)
    if len(xp) < 2 or len(yp) < 2:
        return None
    num_rows, num_cols = len(yp) - 1, len(xp) - 1
    entries, cell_map = [], {}
    for src, (x0, y0, x1, y1) in enumerate(boxes):
        x1i, x2i, y1i, y2i = nearest_index(xp, x0), nearest_index(xp, x1), nearest_index(yp, y0), nearest_index(yp, y1)
        col_start, col_end = min(x1i, x2i, num_cols - 1), min(max(x1i, x2i), num_cols)
        row_start, row_end = min(y1i, y2i, num_rows - 1), min(max(y1i, y2i), num_rows)
        row_span, col_span = max(row_end - row_start, 1), max(col_end - col_start, 1)
        e = len(entries)
        entries.append((src, row_start, col_start, row_span, col_span))
        for r in range(row_start, min(row_start + row_span, num_rows)):
            for c in range(col_start, min(col_start + col_span, num_cols)):
                cell_map.setdefault((r, c), e)
    tokens, order = ["<table>", "<tbody>"], []
    for r in range(num_rows):
        tokens.append("<tr>")
        c = 0
        while c < num_cols:
            e = cell_map.get((r, c))
            if e is None:
                c += 1
                continue
            src, row_start, col_start, row_span, col_span = entries[e]
            if row_start == r and col_start == c:
                attrs = (f' rowspan="{row_span}"' if row_span > 1 else "") + (f' colspan="{col_span}"' if col_span > 1 else "")
                tokens.append(f"<td{attrs}></td>")
                order.append((src, CellGridInfo(row_start, col_start, row_span, col_span)))
            c += max(col_span, 1)
        tokens.append("</tr>")
    tokens += ["</tbody>", "</table>"]
    return (tokens, order) if order else None


# ------------------------------------------------------------------------------------------------ tokens -> HTML
def _parse_td_tag(tokens: Sequence[str], start: int) -> Tuple[str, int]:
    """processors/table_structure_decode.rs:326-392 -> (attributes of the opening tag, index to continue from).  The Paddle dictionaries split
    `<td` attributes into tokens of their own; a token such as `<td colspan="2"></td>` carries them itself."""
    attrs = ""
    t0 = tokens[start]
    if t0.startswith("<td"):
        before_gt = t0[3:].split(">")[0]
        if before_gt:
            attrs += before_gt
    idx = start + 1
    while idx < len(tokens):
        t = tokens[idx]
        if t in (">", "</td>", "<tr>", "</tr>") or t.startswith("<td"):
            break
        attrs += t
        idx += 1
    nxt = idx
    while nxt < len(tokens):
        t = tokens[nxt]
        if t == "</td>":
            nxt += 1
            break
        if t.startswith("<td") or t in ("<tr>", "</tr>"):
            break
        nxt += 1
    return attrs, max(nxt, start + 1)


def wrap_table_html(tokens: Sequence[str], cell_texts: Optional[Sequence[Optional[str]]] = None) -> str:
    """wrap_table_html / wrap_table_html_with_content (processors/table_structure_decode.rs:37-163)"""
    out = ["<html><body>"]
    has_table = len(tokens) > 0 and "<table" in tokens[0]
    if not has_table:
        out.append("<table>")
    td, idx = 0, 0

    def text():
        return cell_texts[td] if cell_texts is not None and td < len(cell_texts) and cell_texts[td] is not None else None

    while idx < len(tokens):
        tag = tokens[idx]
        if tag == "<td></td>":
            out.append("<td>")
            if text() is not None:
                out.append(text())
            out.append("</td>")
            td += 1
            idx += 1
            continue
        if tag.startswith("<td"):
            attrs, nxt = _parse_td_tag(tokens, idx)
            out.append(f"<td{attrs}>")
            bold = nxt < len(tokens) and tokens[nxt] == "<b>"
            if text() is not None:
                out.append(("<b>" if bold else "") + text() + ("</b>" if bold else ""))
            out.append("</td>")
            td += 1
            idx = nxt
            continue
        out.append(tag)
        idx += 1
    if not has_table:
        out.append("</table>")
    out.append("</body></html>")
    return "".join(out)


# ------------------------------------------------------------------------------------------------ tokens -> grid positions
def parse_span_attr(token: str, attr: str) -> Optional[int]:
    """processors/table_structure_decode.rs:293-306: the value of `attr="<unsigned integer>"` inside a tag or attribute token"""
    pattern = attr + '="'
    start = token.find(pattern)
    if start < 0:
        return None
    rest = token[start + len(pattern):]
    end = rest.find('"')
    if end < 0:
        return None
    v = rest[:end]
    if v.startswith("+"):                                             # usize::from_str accepts a leading plus sign
        v = v[1:]
    return int(v) if v.isascii() and v.isdigit() else None


def parse_td_tag(tokens: Sequence[str], start: int) -> Tuple[str, int, int, int]:
    """parse_td_tag (:326-392) -> (attributes, row_span, col_span, index to continue from): `_parse_td_tag` with the spans read on the way"""
    row_span = col_span = 1

    def spans(text):
        nonlocal row_span, col_span
        v = parse_span_attr(text, "colspan")
        if v is not None:
            col_span = v
        v = parse_span_attr(text, "rowspan")
        if v is not None:
            row_span = v

    t0 = tokens[start]
    if t0.startswith("<td"):
        before_gt = t0[3:].split(">")[0]
        if before_gt:
            spans(before_gt)
    idx = start + 1
    while idx < len(tokens):
        t = tokens[idx]
        if t in (">", "</td>", "<tr>", "</tr>") or t.startswith("<td"):
            break
        spans(t)
        idx += 1
    attrs, nxt = _parse_td_tag(tokens, start)
    return attrs, row_span, col_span, nxt


def parse_cell_grid_info(tokens: Sequence[str]) -> List[CellGridInfo]:
    """processors/table_structure_decode.rs:210-291: one CellGridInfo per `<td` token, in order; a rowspan occupies its columns in the rows below"""
    cells, occupied = [], set()
    row = col = idx = 0
    while idx < len(tokens):
        t = tokens[idx]
        if t == "<tr>":
            col = 0
            while (row, col) in occupied:
                col += 1
            idx += 1
        elif t == "</tr>":
            row += 1
            idx += 1
        elif t == "<td></td>":
            while (row, col) in occupied:
                col += 1
            cells.append(CellGridInfo(row, col, 1, 1))
            col += 1
            idx += 1
        elif t.startswith("<td"):
            _, row_span, col_span, nxt = parse_td_tag(tokens, idx)
            while (row, col) in occupied:
                col += 1
            cells.append(CellGridInfo(row, col, row_span, col_span))
            for r in range(1, row_span):
                for c in range(col_span):
                    occupied.add((row + r, col + c))
            col += col_span
            idx = nxt
        else:
            idx += 1
    return cells


def cell_bbox_from_coords(coords) -> np.ndarray:
    """table_analyzer.rs:120-145: the axis-aligned box of a recognized cell (four corner points, or x_min y_min x_max y_max)"""
    c = [F(v) for v in coords]
    if len(c) >= 8:
        xs, ys = c[0:8:2], c[1:8:2]
        return from_coords(min(xs), min(ys), max(xs), max(ys))
    if len(c) >= 4:
        return from_coords(c[0], c[1], c[2], c[3])
    return from_coords(F(0.0), F(0.0), F(0.0), F(0.0))


# ------------------------------------------------------------------------------------------------ the analyzer
def _translate(box: np.ndarray, dx, dy) -> np.ndarray:
    b = np.asarray(box, np.float32).reshape(-1, 2)
    return np.stack([(b[:, 0] + F(dx)).astype(np.float32), (b[:, 1] + F(dy)).astype(np.float32)], -1)


def _first(*adapters):
    for a in adapters:
        if a is not None:
            return a
    return None


class TableAnalyzer:
    """TableAnalyzer (table_analyzer.rs:267-747) without orientation adapters.  The predictors are anything with the
    interface of `api.TableClassifier` (`predict(images)` -> per image a list of objects with `.label` and `.score`), of
    `api.TableCellDetectionPredictor` (`predict(images)` -> per image a list of objects with `.bbox` and `.score`) and of
    `api.TableStructureRecognitionPredictor` (`predict(images)` -> an object with `.structures`, `.bboxes`, `.structure_scores`, one entry per image)."""

    def __init__(self, table_classifier=None, table_cell_detector=None, wired_table_cell_detector=None, wireless_table_cell_detector=None,
                 use_e2e_wired_table_rec: bool = False, use_e2e_wireless_table_rec: bool = False,
                 use_wired_table_cells_trans_to_html: bool = False, use_wireless_table_cells_trans_to_html: bool = False, cell_batch_size: int = 4,
                 table_structure_recognizer=None, wired_table_structure_recognizer=None, wireless_table_structure_recognizer=None):
        self.table_classifier = table_classifier
        self.table_structure_recognizer = table_structure_recognizer
        self.wired_table_structure_recognizer = wired_table_structure_recognizer
        self.wireless_table_structure_recognizer = wireless_table_structure_recognizer
        self.table_cell_detector = table_cell_detector
        self.wired_table_cell_detector = wired_table_cell_detector
        self.wireless_table_cell_detector = wireless_table_cell_detector
        self.use_e2e_wired_table_rec = use_e2e_wired_table_rec
        self.use_e2e_wireless_table_rec = use_e2e_wireless_table_rec
        self.use_wired_table_cells_trans_to_html = use_wired_table_cells_trans_to_html
        self.use_wireless_table_cells_trans_to_html = use_wireless_table_cells_trans_to_html
        self.cell_batch_size = max(int(cell_batch_size), 1)     # TableCellDetectionAdapter::recommended_batch_size

    def _classify(self, crop):
        """:386-404: (table type, confidence); a failing or empty classification is Unknown without a confidence"""
        if self.table_classifier is None:
            return UNKNOWN, None
        try:
            res = self.table_classifier.predict([crop])
        except api.OCRError:
            return UNKNOWN, None
        if not res or not res[0]:
            return UNKNOWN, None
        top = res[0][0]
        label = str(top.label).lower()
        kind = WIRED if label in ("wired", "wired_table") else WIRELESS if label in ("wireless", "wireless_table") else UNKNOWN
        return kind, F(top.score)

    def _plan(self, idx, element, page):
        """Everything of analyze_single_table that precedes cell detection (:309-551).  Returns the table's state or raises."""
        crop = crop_bounding_box(page, element.bbox)
        if crop is None:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"adapter execution failed: table_analyzer: table {idx}: failed to crop table region")
        x_min, y_min, _, _ = aabb(element.bbox)
        off = (max(x_min, F(0.0)), max(y_min, F(0.0)))             # the float crop start point, not the truncated one (:347-350)
        kind, cls_conf = self._classify(crop)
        use_e2e = {WIRED: self.use_e2e_wired_table_rec, WIRELESS: self.use_e2e_wireless_table_rec, UNKNOWN: self.use_e2e_wireless_table_rec}[kind]
        cells_to_html = {WIRED: self.use_wired_table_cells_trans_to_html, WIRELESS: self.use_wireless_table_cells_trans_to_html, UNKNOWN: False}[kind]
        effective_e2e = use_e2e and not cells_to_html
        detector = None
        if not use_e2e or cells_to_html:                           # :440-479
            d, wd, wl = self.table_cell_detector, self.wired_table_cell_detector, self.wireless_table_cell_detector
            detector = {WIRED: _first(wd, d, wl), WIRELESS: _first(wl, d, wd), UNKNOWN: _first(d, wd, wl)}[kind]
        r, wr, wlr = self.table_structure_recognizer, self.wired_table_structure_recognizer, self.wireless_table_structure_recognizer
        recognizer = {WIRED: _first(wr, r), WIRELESS: _first(wlr, r), UNKNOWN: _first(r, wlr, wr)}[kind]          # :424-435
        tokens, boxes, score = None, [], None
        if recognizer is None:                                     # :535-543
            if not cells_to_html or effective_e2e:
                raise api.OCRError(api.OAR_INVALID_INPUT, f"configuration: table_structure_recognition: table {idx} ({kind}): no structure adapter available and "
                                                          "cells->html conversion is disabled")
        else:                                                      # :485-533
            try:
                res = recognizer.predict([crop])
            except api.OCRError as ex:
                if not cells_to_html:                              # surfaced with the table's context; with cells -> HTML the detected cells stand in
                    raise api.OCRError(ex.code, f"adapter execution failed: table_structure_recognition: table {idx} ({kind}): structure recognition failed: {ex.message}")
            else:
                if len(res.structures) > 0 and len(res.bboxes) > 0 and len(res.structure_scores) > 0:
                    tokens, boxes, score = list(res.structures[0]), list(res.bboxes[0]), F(res.structure_scores[0])
        return {"idx": idx, "element": element, "crop": crop, "off": off, "kind": kind, "cls_conf": cls_conf, "use_e2e": use_e2e, "detector": detector,
                "cells_to_html": cells_to_html, "tokens": tokens, "boxes": boxes, "score": score}

    @staticmethod
    def _finish(st, detected) -> TableResult:
        """:553-746; `detected` is the cell detector's output for this table's crop (None: no detector, or it failed)"""
        idx, kind, (dx, dy) = st["idx"], st["kind"], st["off"]
        cells_to_html, tokens, score = st["cells_to_html"], st["tokens"], st["score"]
        cells = []
        if tokens is not None:                                     # :553-584: the recognized cells, with the grid position their token implies
            grid = parse_cell_grid_info(tokens)
            for ci, coords in enumerate(st["boxes"]):
                cell = TableCell(_translate(cell_bbox_from_coords(coords), dx, dy), 1.0)
                if ci < len(grid):
                    cell.row, cell.col, cell.row_span, cell.col_span = grid[ci].row, grid[ci].col, grid[ci].row_span, grid[ci].col_span
                cells.append(cell)
        found = list(detected or [])
        if cells_to_html and found:                                # :610-623: detected cells override the recognized ones; the tokens are regenerated below
            cells = [TableCell(_translate(c.bbox, dx, dy), float(c.score)) for c in found]
            tokens = None
        detected_page = [_translate(c.bbox, dx, dy) for c in found] if (not st["use_e2e"] and not cells_to_html and found) else None   # :625-639

        def regenerate(cells, tokens):
            crop_boxes = []
            for c in cells:
                x0, y0, x1, y1 = aabb(c.bbox)
                crop_boxes.append(from_coords(F(x0 - dx), F(y0 - dy), F(x1 - dx), F(y1 - dy)))
            got = table_cells_to_html_structure(crop_boxes, 5.0)
            if got is None:
                return cells, tokens, False
            new_tokens, order = got
            re = []
            for src, gi in order:
                if src < len(cells):
                    c = cells[src]
                    re.append(TableCell(c.bbox, c.confidence, gi.row, gi.col, gi.row_span, gi.col_span, c.text))
            return (re, new_tokens, True) if re else (cells, tokens, False)

        if cells and tokens is None:                               # :641-674
            cells, tokens, _ = regenerate(cells, tokens)
        if not cells:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"invalid input: table {idx} ({kind}): structure recognition produced no cells")
        if cells_to_html:                                          # :684-717
            cells, tokens, ok = regenerate(cells, tokens)
            if ok and score is None:
                score = 1.0
        if tokens is None:
            raise api.OCRError(api.OAR_INVALID_INPUT, f"invalid input: table {idx} ({kind}): structure recognition produced no structure tokens")
        return TableResult(bbox=np.asarray(st["element"].bbox, np.float32), table_type=kind, cells=cells, html_structure=wrap_table_html(tokens),
                           structure_tokens=tokens, is_e2e=bool(st["use_e2e"]), structure_confidence=None if score is None else float(score),
                           classification_confidence=None if st["cls_conf"] is None else float(st["cls_conf"]), detected_cell_bboxes=detected_page)

    def analyze_tables(self, page_image: np.ndarray, layout_elements: Sequence) -> List[TableResult]:
        """analyze_tables (:285-301): one TableResult per element of type "table", in order; the first table that cannot become a real result raises."""
        tables = [e for e in layout_elements if e.element_type == "table"]
        states, failed = [], None
        for idx, el in enumerate(tables):
            try:
                states.append(self._plan(idx, el, page_image))
            except api.OCRError as ex:                              # the reference stops at this table: the ones before it still run, in order
                failed = ex
                break
        # cell detection over all tables of the page, grouped by detector, in batches
        detected = {}
        by_det = {}
        for st in states:
            if st["detector"] is not None:
                by_det.setdefault(id(st["detector"]), (st["detector"], []))[1].append(st)
        for det, sts in by_det.values():
            for i0 in range(0, len(sts), self.cell_batch_size):
                chunk = sts[i0:i0 + self.cell_batch_size]
                try:
                    res = det.predict([s["crop"] for s in chunk])
                except api.OCRError:                                # `if let Ok(..)` (:590): a failing detector leaves the table without cells
                    res = [None] * len(chunk)
                for s, r in zip(chunk, res):
                    detected[s["idx"]] = r
        out = [self._finish(st, detected.get(st["idx"])) for st in states]
        if failed is not None:
            raise failed
        return out
