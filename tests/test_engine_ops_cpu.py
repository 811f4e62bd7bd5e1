"""The engine's operator table, seen from outside (host-only): Engine::supported_ops() is derived from the rows of the table in csrc/engine.cc, and
oar_onnx_inspect reports every operator name of a file that is not in it.  The 76 public names are written out here, so a row that loses or gains its
`public` mark -- or a rewrite-only name that becomes one a model file may hold -- fails this test."""
import re
from pathlib import Path

import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth.onnx_writer import GraphBuilder

PUBLIC = [
    "Constant", "Dropout", "Identity", "Cast", "Shape", "Conv", "ConvTranspose", "BatchNormalization", "Relu", "HardSwish", "HardSigmoid", "Sigmoid",
    "LeakyRelu", "Tanh", "Erf", "Sqrt", "Exp", "Abs", "Neg", "Reciprocal", "Log", "Gelu", "Softplus", "Clip", "Add", "Sub", "Mul", "Div", "Pow", "PRelu",
    "ReduceMean", "GridSample", "Pad", "GlobalAveragePool", "AveragePool", "MaxPool", "Resize", "Concat", "Reshape", "Flatten", "Squeeze", "Unsqueeze",
    "Transpose", "Split", "Slice", "Gather", "Gemm", "MatMul", "Softmax", "LayerNormalization", "Max", "Min", "Equal", "Less", "Greater", "And", "Or", "Not",
    "Floor", "Ceil", "Round", "ReduceSum", "ReduceMax", "ReduceMin", "ReduceProd", "Expand", "Tile", "Where", "ConstantOfShape", "Range", "ArgMax", "ArgMin",
    "TopK", "GatherND", "GatherElements", "Loop"]
# made by the load-time rewrites only: a model file may not hold them
INTERNAL = ["Linear", "Attention", "WindowAttention", "DeformableAttention", "RelPosAttention", "MultiHeadAttention", "SLADecode", "FormulaDecode", "SEGate", "DSBlock"]


# What dispatch() does with a plan-time input, per name, as the three hand-kept sets had it before the table: a row in the wrong class costs
# OAR_UNSUPPORTED_OP or a tensor without storage at plan time, on a shape nobody tested.
UNARY = ["Relu", "HardSwish", "HardSigmoid", "Sigmoid", "LeakyRelu", "Tanh", "Erf", "Sqrt", "Exp", "Abs", "Neg", "Reciprocal", "Log", "Gelu", "Softplus",
         "Floor", "Ceil", "Round", "Not"]
DATA0 = UNARY + ["Clip", "ReduceMean", "ReduceSum", "ReduceMax", "ReduceMin", "ReduceProd", "ArgMax", "ArgMin", "Softmax", "Expand", "Tile", "Transpose",
                 "Pad", "Resize", "GlobalAveragePool", "AveragePool", "MaxPool", "LayerNormalization", "Linear", "Gemm", "TopK", "Flatten", "Split"]
DATA01 = ["MatMul", "GridSample"]
READS_HOST = ["Add", "Sub", "Mul", "Div", "Pow", "PRelu", "Max", "Min", "Equal", "Less", "Greater", "And", "Or", "Where", "Reshape", "Squeeze", "Unsqueeze",
              "Slice", "Gather", "GatherND", "GatherElements", "Concat", "Identity", "Cast", "ConstantOfShape", "Shape", "Range", "SLADecode", "FormulaDecode"]
BINARY = ["Add", "Sub", "Mul", "Div", "Pow", "PRelu", "Max", "Min", "Equal", "Less", "Greater", "And", "Or"]      # k::binary's operator = the index
REDUCE = ["ReduceMean", "ReduceSum", "ReduceMax", "ReduceMin", "ReduceProd"]                                      # k::reduce_lastdim's mode = the index
NO_HANDLER = ["Constant", "Dropout", "Loop", "Shape", "Range"]

ROW = re.compile(r'^\s*\{"(\w+)",\s*(true|false),\s*(NONE|DATA0|DATA01|READS_HOST),\s*(nullptr|&Planner::(\w+))(?:,\s*(\d+))?\},\s*$')


def _rows():
    """The rows of op_table() as the source spells them: name -> (pub, host_inputs, handler or None, code)."""
    text = (Path(__file__).resolve().parent.parent / "oar_ocr_amd" / "csrc" / "engine.cc").read_text()
    body = text.split("static const OpRow rows[] = {", 1)[1].split("\n    };", 1)[0]
    rows = {}
    for line in body.strip("\n").split("\n"):
        m = ROW.match(line)
        assert m, f"not a table row: {line!r}"
        assert m.group(1) not in rows, m.group(1)
        rows[m.group(1)] = (m.group(2) == "true", m.group(3), m.group(5), int(m.group(6) or 0))
    return rows


def test_every_row_is_in_the_class_its_name_had_in_the_three_old_sets():
    rows = _rows()
    assert set(rows) == set(PUBLIC) | set(INTERNAL)
    assert {n for n, r in rows.items() if r[0]} == set(PUBLIC)
    want = {n: "NONE" for n in rows}
    want.update({n: "DATA0" for n in DATA0}, **{n: "DATA01" for n in DATA01}, **{n: "READS_HOST" for n in READS_HOST})
    assert {n: r[1] for n, r in rows.items()} == want
    assert list(rows) == sorted(rows)                                   # (ASCII order, which is what find_op's search needs)
    assert {n for n, r in rows.items() if r[2] is None} == set(NO_HANDLER)
    assert {n for n, r in rows.items() if r[2] == "op_unary_act"} == set(UNARY)
    assert {n: r[3] for n, r in rows.items() if r[2] == "op_binary_code"} == {n: i for i, n in enumerate(BINARY)}
    assert {n: r[3] for n, r in rows.items() if r[2] == "op_reduce_code"} == {n: i for i, n in enumerate(REDUCE)}
    assert all(r[3] == 0 for r in rows.values() if r[2] not in ("op_binary_code", "op_reduce_code"))


def test_inspect_reports_exactly_the_names_that_are_not_public():
    assert len(PUBLIC) == 76 and len(set(PUBLIC)) == 76 and not set(PUBLIC) & set(INTERNAL)
    g = GraphBuilder("ops")
    g.add_input("x", [1])
    names = PUBLIC + INTERNAL + ["NoSuchOp"]
    for i, name in enumerate(names):
        g.op(name, ["x"] * 5, outputs=[f"y{i}"])
    g.add_output("y0", [1])
    with pytest.raises(api.OCRError) as e:
        api.onnx_inspect(g.model())
    assert e.value.code == api.OAR_UNSUPPORTED_OP
    prefix = "operators not implemented: "
    assert prefix in e.value.message
    reported = e.value.message.split(prefix, 1)[1].split(", ")
    assert reported == sorted(INTERNAL + ["NoSuchOp"])
