"""The WindowAttention operator (csrc/window_attention.hip): the attention of one Swin block without shifted windows -- window partition, q / k / v
Linears, per-window multi-head attention with an additive [nh, N, N] relative-position bias, projection, window reverse -- which the engine's rewrite pass 3b
turns into ONE launch that gathers and scatters a window's tokens by address.  Graphs: synth.models.build_swin_block (the attention part of one block).

Reference: the same block in torch on the CPU, in f64 and f32 (synth/unimernet_reference.py); noise = max |f32 - f64|, tol = max(16 noise, 2^-19).  The bias is
U(-2, 2) per entry, different for every head and not symmetric in (i, j): an index that is transposed or taken from another head moves the output by O(1).
Per case: exactly one launch of class window_attention with the pass on, none with OAR_FUSE_WINDOW_ATTENTION=0, and both outputs within tol of f64."""
import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.unimernet_reference import reference_bundle, swin_block_reference

pytestmark = pytest.mark.gpu

#          B   H   W   C nh  ws
SHAPES = [(2, 14, 21, 24, 3, 7),        # N = 49, dh = 8
          (1, 10, 15, 64, 2, 5),        # N = 25, dh = 32
          (1, 12, 24, 48, 4, 12),       # N = 144, dh = 12
          (3, 4, 4, 16, 1, 4),          # one window per image, one head
          (1, 16, 32, 32, 1, 16)]       # N = 256, dh = 32: the largest N * dh, more than 64 KB of LDS
IDS = ["B%d_H%d_W%d_C%d_nh%d_ws%d" % s for s in SHAPES]
FALLBACK = (1, 8, 8, 80, 1, 4)          # dh = 80 > 64: k::window_attention_supported says no

_cache = {}


def _case(shape, scale):
    """model, input, reference bundle: computed once, never modified"""
    if (shape, scale) not in _cache:
        B, H, W, C, nh, ws = shape
        model, info = models.build_swin_block(H, W, C, nh, ws, seed=3, scale=scale)
        x = np.random.default_rng(11).standard_normal((B, H * W, C)).astype(np.float32)
        _cache[(shape, scale)] = (model, x, reference_bundle(swin_block_reference, info, x))
    return _cache[(shape, scale)]


def _run(model, x, monkeypatch, fuse):
    """-> (y, launches of class window_attention in one infer)"""
    if fuse is None:
        monkeypatch.delenv("OAR_FUSE_WINDOW_ATTENTION", raising=False)
    else:
        monkeypatch.setenv("OAR_FUSE_WINDOW_ATTENTION", fuse)      # (read when the graph is loaded)
    eng = api.OrtInfer(model, profile=True)
    try:
        api.prof_reset()
        api.prof_enable(True)
        y = dict(eng.infer(x))["y"]
        snap = {e["name"]: e for e in api.prof_snapshot()}
        return y, snap.get("window_attention", {}).get("launches", 0), snap
    finally:
        api.prof_enable(False)
        eng.close()


@pytest.mark.parametrize("scale", ["div", "mul"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_launch_per_block_and_both_routes_match_f64(shape, scale, monkeypatch):
    model, x, ref = _case(shape, scale)
    fused, n_fused, snap = _run(model, x, monkeypatch, None)
    plain, n_plain, snap0 = _run(model, x, monkeypatch, "0")
    e1 = float(np.abs(fused.astype(np.float64) - ref["f64"]).max())
    e0 = float(np.abs(plain.astype(np.float64) - ref["f64"]).max())
    print(f"{shape} {scale}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} | fused err {e1:.2e} ({sum(e['launches'] for e in snap.values())} launches) | "
          f"op-by-op err {e0:.2e} ({sum(e['launches'] for e in snap0.values())} launches)")
    assert n_fused == 1, sorted((k, v["launches"]) for k, v in snap.items())
    assert n_plain == 0, sorted((k, v["launches"]) for k, v in snap0.items())
    assert fused.shape == ref["f64"].shape and e1 <= ref["tol"], (e1, ref["tol"])
    assert e0 <= ref["tol"], (e0, ref["tol"])


def test_explicit_knob_on_is_the_default(monkeypatch):
    model, x, ref = _case(SHAPES[0], "div")
    a, na, _ = _run(model, x, monkeypatch, None)
    b, nb, _ = _run(model, x, monkeypatch, "1")
    assert na == nb == 1 and np.array_equal(a, b)                  # (and run-to-run identical)


def test_unsupported_head_size_keeps_the_op_by_op_route(monkeypatch):
    model, x, ref = _case(FALLBACK, "div")
    y, n, snap = _run(model, x, monkeypatch, None)
    y0, n0, _ = _run(model, x, monkeypatch, "0")
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max())
    print(f"fallback {FALLBACK}: err {err:.2e} tol {ref['tol']:.2e}")
    assert n == 0 and n0 == 0, sorted((k, v["launches"]) for k, v in snap.items())
    assert np.array_equal(y, y0) and err <= ref["tol"], (err, ref["tol"])


def test_whole_block_fuses_too(monkeypatch):
    """the whole block (conv enhance and MLP behind the attention) still fuses: one launch; its numbers are checked in test_gpu_unimernet.py"""
    B, H, W, C, nh, ws = SHAPES[0]
    model, info = models.build_swin_block(H, W, C, nh, ws, seed=3, whole=True)
    x = np.random.default_rng(11).standard_normal((B, H * W, C)).astype(np.float32)
    ref = reference_bundle(swin_block_reference, info, x)
    y, n, snap = _run(model, x, monkeypatch, None)
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max())
    print(f"whole block: err {err:.2e} tol {ref['tol']:.2e} noise {ref['noise']:.2e}")
    assert n == 1 and err <= ref["tol"], (n, err, ref["tol"])
