"""Multi-scale deformable attention without a GPU: the exported spelling synth.models writes is evaluated unchanged by the numpy oracle and agrees
with the torch reference (F.grid_sample, f64) within tol = max(16 noise, 2^-19), noise = max |f32 - f64|, for the core in both weight modes and for the
RT-DETR-shaped decoder layer by layer; the graphs that existed before are byte-identical; and the kernel's registers, scratch and occupancy are what its
design needs (it lives on memory latency: at least four waves per SIMD, nothing in scratch)."""
import hashlib
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.rtdetr_reference import deformable_attention_inputs, deformable_attention_reference, rtdetr_decoder_reference
from oar_ocr_amd.synth.unimernet_reference import reference_bundle
from oracle import onnx_np

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

#          N   Q  nh  c  levels (h, w)                        P        (tests/test_gpu_deformable_attention.py's, the fall-back shape included)
SHAPES = [(2, 7, 2, 8, ((5, 7), (3, 4)), 3),
          (1, 5, 3, 4, ((1, 1), (2, 9), (6, 1)), 4),
          (1, 300, 8, 32, ((10, 10), (5, 5), (3, 3)), 4),
          (3, 33, 4, 16, ((4, 6),), 1),
          (1, 9, 1, 64, ((3, 5), (2, 2), (2, 3), (1, 2)), 8),
          (1, 6, 2, 6, ((4, 4),), 2)]
IDS = ["N%d_Q%d_nh%d_c%d_L%d_P%d" % (s[0], s[1], s[2], s[3], len(s[4]), s[5]) for s in SHAPES]


@pytest.mark.parametrize("align_corners", [0, 1])
@pytest.mark.parametrize("mode", ["softmax", "input"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exported_spelling_agrees_with_the_reference(shape, mode, align_corners):
    model, info = models.build_deformable_attention(*shape, weights=mode, align_corners=align_corners)
    value, loc, logit = deformable_attention_inputs(info, seed=5)
    ref = reference_bundle(deformable_attention_reference, info, value, loc, logit)
    y = onnx_np.run(model, {"value": value, "loc": loc, "logit": logit})[0]
    err = float(np.abs(y.astype(np.float64) - ref["f64"]).max())
    outside = float(((loc < 0) | (loc > 1)).mean())
    print(f"{shape} {mode} align {align_corners}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e} max |y| {np.abs(ref['f64']).max():.2f} outside {outside:.2f}")
    assert y.shape == (shape[0], shape[1], shape[2] * shape[3]) and err <= ref["tol"], (err, ref["tol"])
    assert 0.25 < outside < 0.45 and np.abs(loc).max() < 3.0        # the zero padding is exercised; every location within a few widths of the image
    if mode == "input":
        w = logit.reshape(shape[0], shape[1], shape[2], -1)
        assert np.allclose(w.sum(-1), 1.0, atol=1e-5)               # normalised weights, not logits


def test_rtdetr_decoder_agrees_with_the_reference_layer_by_layer():
    model, info = models.build_rtdetr_decoder(D=32, nh=4, levels=((8, 8), (4, 4), (2, 2)), P=4, layers=2, Q=20, n_classes=3, seed=0)
    rng = np.random.default_rng(3)
    feeds = {"memory": rng.standard_normal((2, 84, 32)).astype(np.float32), "tgt": rng.standard_normal((2, 20, 32)).astype(np.float32),
             "ref_logit": rng.uniform(-1.5, 1.5, (2, 20, 4)).astype(np.float32)}
    names = ["boxes", "logits"] + info["layer_outputs"]
    assert info["layer_outputs"] == ["out0", "ref0", "out1", "ref1"]
    outs = dict(zip(names, onnx_np.run(model, feeds)))
    for nm in info["layer_outputs"] + ["boxes", "logits"]:
        ref = reference_bundle(rtdetr_decoder_reference, info, feeds["memory"], feeds["tgt"], feeds["ref_logit"], want=nm)
        err = float(np.abs(outs[nm].astype(np.float64) - ref["f64"]).max())
        print(f"{nm}: noise {ref['noise']:.2e} tol {ref['tol']:.2e} err {err:.2e}")
        assert outs[nm].shape == ref["f64"].shape and err <= ref["tol"], (nm, err, ref["tol"])
    assert np.array_equal(outs["boxes"], outs["ref1"])               # the boxes are the last layer's refined reference


def test_existing_table_cell_detector_bytes_are_unchanged():
    m = models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24)[0]
    assert len(m) == 287396
    assert hashlib.sha256(m).hexdigest() == "fc70273f09319c31308ac88f6dfb320868e7f64794c03c912506f210f95603fe"


def test_detector_with_decoder_declares_its_selections():
    m, info = models.build_table_cell_det(image_shape=(128, 128), queries=40, keep=24, decoder_layers=2)
    parsed = onnx_np.parse_model(m)
    ops = [nd["op"] for nd in parsed["nodes"]]
    assert ops.count("GridSample") == 2 * 3 and ops.count("TopK") == 2 and info["decoder_layers"] == 2
    declared = {o["name"] if isinstance(o, dict) else o for o in parsed["outputs"]}
    for t in info["topk"]:
        assert t["input"] in declared and t["index"] in declared


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_kernel_resources():
    """the compiler's resource remarks only: no spill, nothing in scratch (a run-time-indexed register array or argument field would land there), and at
    least four waves per SIMD"""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'oar_ocr_amd' / 'csrc'}", f"-I{ROOT / 'include'}",
                        "--cuda-device-only", "-c", str(ROOT / "oar_ocr_amd" / "csrc" / "deformable_attention.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    block = r.stderr[r.stderr.index("deformable_attention_kernel"):]
    get = lambda pat: int(re.search(pat, block).group(1))
    res = {"vgprs": get(r" VGPRs: (\d+)"), "spill": get(r"VGPRs Spill: (\d+)"), "sgpr_spill": get(r"SGPRs Spill: (\d+)"), "scratch": get(r"ScratchSize \[bytes/lane\]: (\d+)"),
           "occupancy": get(r"Occupancy \[waves/SIMD\]: (\d+)"), "lds": get(r"LDS Size \[bytes/block\]: (\d+)")}
    print(res)
    assert res["spill"] == 0 and res["sgpr_spill"] == 0 and res["scratch"] == 0 and res["occupancy"] >= 4 and res["lds"] == 0, res
