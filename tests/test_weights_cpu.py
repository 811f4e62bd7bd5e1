"""Real-weights mode (SURVEY 8d mode i; VERDICT r5 missing #3): the registry check in front of operator-supplied files, bench.py's refusal, and the
ORT stand-in's plumbing (with a stub session: onnxruntime is not installed here)."""
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oar_ocr_amd import weights

ROOT = Path(__file__).resolve().parent.parent


def test_registry_rows_restate_the_reference_registry():
    """name / sha256 / size of every row, against the rows of the reference's registry.rs stored in tests/golden/registry_rows.json."""
    for name, e in weights.REGISTRY.items():
        assert len(e.sha256) == 64 and int(e.sha256, 16) >= 0 and e.size > 0
    assert all(all(n in weights.REGISTRY for n in files) for files in weights.CONFIG_FILES.values())
    rows = {r["line"]: r for r in json.loads((ROOT / "tests" / "golden" / "registry_rows.json").read_text())["rows"]}
    assert len(rows) == len(weights.REGISTRY)
    for name, e in weights.REGISTRY.items():
        row = rows[e.line]
        assert (row["name"], row["sha256"], row["size"]) == (name, e.sha256, e.size), (name, row)


def _registry_for(tmp_path, blobs):
    reg = {}
    for name, data in blobs.items():
        (tmp_path / name).write_bytes(data)
        reg[name] = weights.Entry(hashlib.sha256(data).hexdigest(), len(data), 0)
    return reg


def test_verify_file_accepts_only_the_registry_file(tmp_path):
    rng = np.random.default_rng(0)
    blobs = {"pp-ocrv6_tiny_det.onnx": rng.bytes(5000), "pp-ocrv6_tiny_rec.onnx": rng.bytes(7000), "ppocrv6_tiny_dict.txt": "a\nb\n\n中\n".encode()}
    reg = _registry_for(tmp_path, blobs)
    det, rec, chars, report = weights.load_config(tmp_path, 1, registry=reg)
    assert det == blobs["pp-ocrv6_tiny_det.onnx"] and rec == blobs["pp-ocrv6_tiny_rec.onnx"] and chars == ["a", "b", "中"]
    assert [r["file"] for r in report] == list(weights.CONFIG_FILES[1]) and report[0]["sha256"] == reg["pp-ocrv6_tiny_det.onnx"].sha256
    # one flipped bit, same size
    bad = bytearray(blobs["pp-ocrv6_tiny_det.onnx"]); bad[100] ^= 1
    (tmp_path / "pp-ocrv6_tiny_det.onnx").write_bytes(bytes(bad))
    with pytest.raises(weights.WeightsError) as e:
        weights.load_config(tmp_path, 1, registry=reg)
    assert "sha256" in str(e.value)
    # truncated
    (tmp_path / "pp-ocrv6_tiny_det.onnx").write_bytes(blobs["pp-ocrv6_tiny_det.onnx"][:-1])
    with pytest.raises(weights.WeightsError) as e:
        weights.verify_file(tmp_path / "pp-ocrv6_tiny_det.onnx", reg)
    assert "bytes" in str(e.value)
    # a name the registry does not know, a missing file
    (tmp_path / "my_model.onnx").write_bytes(b"x")
    with pytest.raises(weights.WeightsError):
        weights.verify_file(tmp_path / "my_model.onnx", reg)
    (tmp_path / "pp-ocrv6_tiny_det.onnx").write_bytes(blobs["pp-ocrv6_tiny_det.onnx"])
    (tmp_path / "ppocrv6_tiny_dict.txt").unlink()
    with pytest.raises(weights.WeightsError) as e:
        weights.load_config(tmp_path, 1, registry=reg)
    assert "missing" in str(e.value)
    # against the REAL registry a synthetic file of the right name is refused (size first)
    (tmp_path / "pp-ocrv6_tiny_det.onnx").write_bytes(blobs["pp-ocrv6_tiny_det.onnx"])
    with pytest.raises(weights.WeightsError):
        weights.verify_file(tmp_path / "pp-ocrv6_tiny_det.onnx")


def test_bench_refuses_unverified_weights(tmp_path):
    (tmp_path / "pp-ocrv6_tiny_det.onnx").write_bytes(b"not the file")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--stub-engine", "--models-dir", str(tmp_path), "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and "refused" in r.stderr and r.stdout.strip() == ""


def test_ort_standin_plumbing_with_a_stub_session():
    """oracle/ort_standin.py routes exactly the two networks through its sessions and leaves the rest of the oracle alone: with a stub session that
    evaluates the graph with the torch interpreter, the stand-in pipeline returns the oracle pipeline's own result."""
    from oar_ocr_amd import api
    from oar_ocr_amd.synth import models, pages
    from oracle import onnx_ref, ort_standin, pipeline_ref

    class Sess:
        calls = 0

        def __init__(self, model_bytes):
            self.m = onnx_ref.parse_model(model_bytes)

        def get_inputs(self):
            return [type("I", (), {"name": self.m["inputs"][0]})()]

        def run(self, _, feeds):
            Sess.calls += 1
            return TORCH_RUN(self.m, feeds)
    TORCH_RUN = onnx_ref.run
    det, _ = models.build_det("tiny", seed=0)
    rec, _ = models.build_rec("tiny", vocab=301, seed=1)
    chars = api.read_dict(models.synth_dict(299))
    page = pages.make_page(3, (160, 320), lines=3)
    oc, run = ort_standin.make_oracle_ocr(det, rec, chars, threads=2, session_factory=Sess)
    onnx_ref.run = run
    try:
        got = oc.predict([page])[0]
    finally:
        onnx_ref.run = TORCH_RUN
    want = pipeline_ref.OracleOCR(det, rec, chars, 0.3, 0.6, 1.5, image_batch_size=1, region_batch_size=16).predict([page])[0]
    assert Sess.calls >= 2 and len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert np.array_equal(g["box"], w["box"]) and g["text"] == w["text"] and g["score"] == w["score"]
