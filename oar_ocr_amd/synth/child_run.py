"""One inference in a fresh Python process: for switches the native library reads once per process (OAR_IGEMM_X6, OAR_IGEMM_RS3, ...), which a test
cannot flip inside its own.  The model, the input and the result travel through files of a directory the caller owns; one child at a time, its own
time limit, never retried."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oar_ocr_amd import api
d = sys.argv[2]
eng = api.OrtInfer(open(d + "/model.onnx", "rb").read(), profile=True)
x = np.load(d + "/x.npy")
api.prof_enable(True); api.prof_reset()
y = eng.infer(x)[0][1]
names = sorted({e["name"] for e in api.prof_snapshot()})
api.prof_enable(False)
eng.close()
np.savez(d + "/out.npz", y=y, names=np.array(names))
"""


def infer_in_child(model: bytes, x, env: dict, workdir, timeout: float = 120.0):
    """-> (first output, set of profiler classes that ran) of OrtInfer(model).infer(x) in a child process started with `env` on top of this one's"""
    d = Path(workdir)
    d.mkdir(parents=True, exist_ok=True)
    (d / "model.onnx").write_bytes(model)
    np.save(d / "x.npy", np.ascontiguousarray(x, np.float32))
    out = d / "out.npz"
    if out.exists():
        out.unlink()
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(d)], env={**os.environ, **{k: str(v) for k, v in env.items()}},
                       timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0 and out.exists(), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    with np.load(out) as z:
        return z["y"], {str(n) for n in z["names"]}
