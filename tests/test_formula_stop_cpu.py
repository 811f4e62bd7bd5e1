"""The stop token of the formula decode where no GPU is needed: the two C symbols, their Python faces, the predictor's switch, and the resources of
the one kernel that runs only with the stop on (the other kernels of formula_decode.hip are counted in test_formula_cpu.py)."""
import inspect
import re
import subprocess
from pathlib import Path

from oar_ocr_amd import api, build, formula

ROOT = Path(__file__).resolve().parent.parent


def test_symbols_are_declared_and_exported():
    build.build_lib()
    hdr = (ROOT / "include" / "oar_mi355x.h").read_text()
    L = api.lib()
    for sym in ("oar_engine_set_decode_stop", "oar_engine_decode_stats"):
        assert re.search(r"\b" + sym + r"\s*\(", hdr), sym
        assert hasattr(L, sym) and sym in api.EXPORTS, sym
    m = re.search(r"typedef struct \{([^}]*)\} oar_decode_stats;", hdr)
    assert m and [f.strip() for f in m.group(1).replace("int64_t", "").strip(" ;").split(",")] == ["steps_limit", "steps_enqueued", "steps_executed", "lookahead"]
    assert [f[0] for f in api.DecodeStats._fields_] == ["steps_limit", "steps_enqueued", "steps_executed", "lookahead"]
    assert api.C.sizeof(api.DecodeStats) == 32


def test_python_faces():
    assert callable(getattr(api.OrtInfer, "set_decode_stop", None)) and callable(getattr(api.OrtInfer, "decode_stats", None))
    assert list(inspect.signature(api.OrtInfer.set_decode_stop).parameters) == ["self", "token"]
    par = inspect.signature(formula.FormulaRecognitionPredictor.__init__).parameters
    assert "stop_at_eos" in par and par["stop_at_eos"].default is False


def test_fill_kernel_uses_no_scratch():
    src = build.CSRC / "formula_decode.hip"
    r = subprocess.run([build.HIPCC] + build.FLAGS + ["-c", str(src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    found = {k: v for k, v in kernels.items() if "fd_fill_tail_kernel" in k}
    assert len(found) == 1, sorted(kernels)
    for k, v in found.items():
        assert v["spill"] == 0 and v["scratch"] == 0 and v["vgprs"] <= 128 and v["lds"] == 0, (k, v)
