"""The load-time graph rewriter, seen without a device (csrc/engine_rewrite.cc, csrc/engine_loops.cc; oar_onnx_rewrite lists what it made of a model).
Every number here was taken from the listing of the commit in front of the split of engine.cc (the rewriter was one member function of Engine then, dumped
through a constructor that stopped short of the device) -- never from the code under test: the split moved the passes, it may not change what one does."""
import collections
import re
from pathlib import Path

import pytest

from oar_ocr_amd import api, build
from oar_ocr_amd.synth import models

CSRC = Path(__file__).resolve().parent.parent / "oar_ocr_amd" / "csrc"
SWITCHES = ["OAR_FUSE_GELU", "OAR_FUSE_LAYERNORM", "OAR_FUSE_WINDOW_ATTENTION", "OAR_FUSE_RELPOS_ATTENTION", "OAR_FUSE_DEFORMABLE_ATTENTION", "OAR_FUSE_MHA_ATTENTION",
            "OAR_FUSE_ATTENTION", "OAR_FUSE_SE", "OAR_FUSE_DSBLOCK", "OAR_FUSE_SE_SCALE", "OAR_FUSE_SE_POOL", "OAR_FUSE_ADD_LAYERNORM"]

MODELS = {
    "det_tiny": lambda: models.build_det("tiny", seed=0),
    "rec_tiny": lambda: models.build_rec("tiny", vocab=97, seed=1),
    "cls4": lambda: models.build_cls(4, seed=5),
    "svtrv2_op": lambda: models.build_rec_svtrv2("svtrv2_small", vocab=97),
    "svtrv2_dec": lambda: models.build_rec_svtrv2("svtrv2_small", vocab=97, layernorm="decomposed"),
    "swin_plain": lambda: models.build_swin_block(8, 8, 16, 2, 4, seed=3),
    "swin_padded_shifted": lambda: models.build_swin_block(10, 13, 24, 3, 7, seed=3, shift=3, mask="swin", pad_value=0.0),
    "slanet": lambda: models.build_slanet(C=24, H=32, V=20, L=8, M=6, image_shape=(32, 32)),
    "formula": lambda: models.build_formulanet(D=24, nh=3, F=40, V=37, Ld=2, M=5),
    "unimernet": lambda: models.build_unimernet(image_shape=(32, 64), M=4),
    "rtdetr_decoder": lambda: models.build_rtdetr_decoder(),
    "aifi": lambda: models.build_aifi_layer(3, 4, 32, 4, 64, seed=2),
    "mha_self": lambda: models.build_mha(2, 20, 20, 4, 8, seed=3),
    "deformable": lambda: models.build_deformable_attention(2, 20, 4, 8, ((8, 8), (4, 4), (2, 2)), 4),
    "vary_vit": lambda: models.build_vary_vit(image_shape=(64, 48), seed=1),
    "add_ln_post": lambda: models.build_add_layernorm_case(2, 5, 32, "post"),
}
_built = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    build.build_lib()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def listing(name: str) -> str:
    if name not in _built:
        _built[name] = MODELS[name]()[0]
    return api.onnx_rewrite(_built[name])


def hist(text: str) -> dict:
    """operator -> count over the `node <id> <op> ...` lines"""
    return dict(collections.Counter(line.split()[2] for line in text.splitlines() if line.startswith("node ")))


# ------------------------------------------------------------------------------------------------ 1. what each pass leaves behind
HISTOGRAMS = {
    # pass 3b: the partition, the attention and the reverse of a Swin block are ONE node; pass 4 folded the residual Add into the projection
    "swin_plain": {"Identity": 1, "LayerNormalization": 1, "Linear": 4, "WindowAttention": 1},
    "swin_padded_shifted": {"Identity": 1, "LayerNormalization": 1, "Linear": 4, "WindowAttention": 1},   # pad, both rolls, mask and crop are gone as well
    # passes 1, 3, 5, 6, 7, 8, 9, 10 on the tiny recognizer
    "rec_tiny": {"Attention": 2, "AveragePool": 1, "Concat": 1, "Conv": 10, "DSBlock": 8, "LayerNormalization": 5, "Linear": 9, "SEGate": 2, "Softmax": 1, "Squeeze": 2,
                 "Transpose": 3, "Unsqueeze": 1},
    "det_tiny": {"Concat": 1, "Conv": 14, "ConvTranspose": 2, "DSBlock": 8, "Identity": 1, "Resize": 6, "SEGate": 2},
    "cls4": {"Conv": 6, "DSBlock": 2, "Flatten": 1, "Gemm": 1, "GlobalAveragePool": 1, "SEGate": 2, "Softmax": 1},
    # pass 0: the Loop is one Linear and one SLADecode (the other ops are the backbone and the initial state)
    "slanet": {"Concat": 1, "ConstantOfShape": 2, "Conv": 2, "DSBlock": 2, "Gather": 1, "Linear": 1, "Reshape": 1, "SLADecode": 1, "Shape": 1, "Softmax": 1, "Transpose": 3},
    # pass 0: one FormulaDecode; the empty initial caches left with their ConstantOfShape (one remains: the start token's)
    "formula": {"ConstantOfShape": 1, "Conv": 2, "FormulaDecode": 1, "Gather": 1, "Linear": 4, "Reshape": 5, "Shape": 1, "Transpose": 6},
    "unimernet": {"Add": 4, "ConstantOfShape": 1, "Conv": 6, "FormulaDecode": 1, "Gather": 1, "LayerNormalization": 10, "Linear": 29, "Reshape": 15, "Shape": 1, "Transpose": 15,
                  "WindowAttention": 4},
    # passes 3c and 3e
    "rtdetr_decoder": {"Add": 6, "DeformableAttention": 2, "Div": 2, "Identity": 2, "LayerNormalization": 6, "Linear": 29, "Mul": 4, "MultiHeadAttention": 2, "Reshape": 2,
                       "Sigmoid": 5, "Slice": 4, "Unsqueeze": 4},
    "aifi": {"Add": 1, "Identity": 1, "LayerNormalization": 2, "Linear": 6, "MultiHeadAttention": 1},
    "deformable": {"DeformableAttention": 1},
    # passes 2b, 2, 3, 4, 5, 10 on SVTRv2
    "svtrv2_op": {"Add": 3, "Attention": 4, "Conv": 7, "LayerNormalization": 16, "Linear": 23, "ReduceMean": 1, "Reshape": 12, "Softmax": 1, "Transpose": 13},
}


@pytest.mark.parametrize("name", sorted(HISTOGRAMS))
def test_operator_histogram_after_rewriting(name):
    text = listing(name)
    assert hist(text) == HISTOGRAMS[name]
    assert text.rstrip().endswith("fuse_add_ln 1")


def test_what_the_fused_nodes_swallowed_is_gone():
    swin = listing("swin_plain")
    assert "Softmax" not in hist(swin) and "perm=is:0,1,3,2,4,5" not in swin          # no rank-6 Transpose
    assert "Loop" not in hist(listing("slanet")) and "Loop" not in hist(listing("formula"))
    rec = listing("rec_tiny")
    assert rec.count("gap_raw=i:1") == 2 and rec.count("after_add=i:1") == 4 and "BatchNormalization" not in hist(rec)
    assert listing("svtrv2_op").count("after_add=i:1") == 14


# ------------------------------------------------------------------------------------------------ 2. two spellings meet
def test_decomposed_and_opset17_layernorm_meet():
    op, dec = listing("svtrv2_op"), listing("svtrv2_dec")
    assert hist(op) == hist(dec)
    count = lambda t: sum(1 for line in t.splitlines() if line.startswith("ln_spelled "))
    assert count(op) == 0 and count(dec) == 16                                       # pass 2c keeps what it replaced, for op_layernorm's other axes
    assert dec.count("after_add=i:1") == 14


# ------------------------------------------------------------------------------------------------ 3. each switch brings back what its pass removes
#            switch, value, model, operators that must have exactly this count with the switch set
SWITCH_CASES = [
    ("OAR_FUSE_GELU", "0", "svtrv2_op", {"Erf": 9, "Div": 9, "Mul": 18, "Add": 12}),
    ("OAR_FUSE_LAYERNORM", "0", "svtrv2_dec", {"LayerNormalization": 0, "ReduceMean": 33, "Sqrt": 16, "Pow": 16, "Sub": 16}),
    ("OAR_FUSE_WINDOW_ATTENTION", "0", "swin_plain", {"WindowAttention": 0, "Softmax": 1, "MatMul": 2, "Transpose": 7, "Reshape": 8}),
    ("OAR_FUSE_DEFORMABLE_ATTENTION", "0", "deformable", {"DeformableAttention": 0, "GridSample": 3, "Softmax": 1, "ReduceSum": 1}),
    ("OAR_FUSE_MHA_ATTENTION", "0", "mha_self", {"MultiHeadAttention": 0, "Softmax": 1, "MatMul": 2, "Transpose": 5}),
    ("OAR_FUSE_ATTENTION", "0", "rec_tiny", {"Attention": 0, "Softmax": 3, "MatMul": 4, "Split": 2, "Squeeze": 8}),
    ("OAR_FUSE_SE", "0", "cls4", {"SEGate": 0, "Conv": 10, "Mul": 2}),
    ("OAR_FUSE_DSBLOCK", "0", "det_tiny", {"DSBlock": 0, "Conv": 30}),
    ("OAR_FUSE_SE_SCALE", "0", "cls4", {"Mul": 2, "SEGate": 2, "Conv": 6}),
    ("OAR_FUSE_SE_POOL", "0", "cls4", {"GlobalAveragePool": 3, "SEGate": 2}),
    ("OAR_FUSE_ADD_LAYERNORM", "0", "add_ln_post", {"Add": 1, "LayerNormalization": 1}),
]


@pytest.mark.parametrize("switch, value, name, want", SWITCH_CASES, ids=[c[0] for c in SWITCH_CASES])
def test_switch_off_brings_back_the_operators(monkeypatch, switch, value, name, want):
    on = listing(name)
    monkeypatch.setenv(switch, value)
    off = listing(name)                                                              # read at every load: both arms in one process
    assert off != on
    h = hist(off)
    assert {k: h.get(k, 0) for k in want} == want
    if switch == "OAR_FUSE_SE_POOL":
        assert on.count("gap_raw=i:1") == 2 and off.count("gap_raw") == 0
    if switch == "OAR_FUSE_ADD_LAYERNORM":
        assert on.count("after_add=i:1") == 1 and off.count("after_add") == 0 and off.rstrip().endswith("fuse_add_ln 0")


def test_se_pool_distinguishes_unset_zero_and_one(monkeypatch):
    unset = listing("cls4")
    monkeypatch.setenv("OAR_FUSE_SE_POOL", "1")
    one = listing("cls4")
    assert hist(one) == hist(unset) == HISTOGRAMS["cls4"]                             # the pool is fused either way ...
    assert unset.count("gap_raw=i:1") == 2 and one.count("gap_raw") == 0             # ... 1 keeps the finishing launch


def test_relpos_attention_is_opt_in(monkeypatch):
    want_off = {"Add": 7, "Conv": 3, "LayerNormalization": 4, "Linear": 9, "MatMul": 8, "Mul": 2, "Pad": 1, "Reshape": 35, "Slice": 1, "Softmax": 2, "Split": 2, "Squeeze": 6,
                "Transpose": 19, "Unsqueeze": 4}
    assert hist(listing("vary_vit")) == want_off
    monkeypatch.setenv("OAR_FUSE_RELPOS_ATTENTION", "0")
    assert hist(listing("vary_vit")) == want_off
    monkeypatch.setenv("OAR_FUSE_RELPOS_ATTENTION", "1")
    assert hist(listing("vary_vit")) == {"Add": 1, "Conv": 3, "LayerNormalization": 4, "Linear": 9, "RelPosAttention": 2, "Reshape": 3, "Transpose": 3}


# ------------------------------------------------------------------------------------------------ 4. the order of the passes
def test_pass_order_is_written_in_run():
    text = (CSRC / "engine_rewrite.cc").read_text()
    run = text[text.index("RewrittenGraph run(OnnxModel& m) {"):]
    run = run[:run.index("\n    }\n")]
    called = re.findall(r"^\s+pass_([0-9]+[a-z]?)_\w+\(\);$", run, re.M)
    assert called == ["0", "1", "2", "2b", "2c", "3", "3b", "3d", "3c", "3e", "4", "5", "6", "7", "8", "9", "10"]
    defined = re.findall(r"^    void pass_([0-9]+[a-z]?)_\w+\(\) \{$", text, re.M)
    assert sorted(defined) == sorted(called) and len(set(defined)) == 17             # one member function per pass, each called once


def test_listing_reports_its_length_and_cuts():
    import ctypes as C
    model = MODELS["add_ln_post"]()[0]
    full = api.onnx_rewrite(model)
    assert full.startswith("node 0 Add out=[") and "\ninit " in full
    b = (C.c_char * len(model)).from_buffer_copy(model)
    need = C.c_size_t(0)
    buf = C.create_string_buffer(16)
    assert api.lib().oar_onnx_rewrite(C.cast(b, C.c_void_p), len(model), buf, 16, C.byref(need)) == 0
    assert need.value == len(full.encode()) and buf.value.decode() == full[:15]
    with pytest.raises(api.OCRError) as ex:
        api.onnx_rewrite(models.build_slanet(C=20, H=24, V=11, L=4, M=4, head_only=True, first_act="Relu")[0])
    assert ex.value.code == api.OAR_UNSUPPORTED_OP and "(Relu) does not fit: the attention activation must be a Tanh" in str(ex.value)
