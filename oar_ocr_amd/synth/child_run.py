"""One inference in a fresh Python process: for switches the native library reads once per process (OAR_IGEMM_X6, OAR_IGEMM_RS3, ...), which a test
cannot flip inside its own.  The model, the input and the result travel through files of a directory the caller owns; one child at a time, its own
time limit, never retried.  infer_* run api.OrtInfer, recognize_many_in_child runs api.TextRecognitionPredictor (the recognizer seam: its fused CTC tail),
stem_many_in_child runs api.k_stem_u8 next to its twin on api.OrtInfer, detect_in_child runs api.TextDetectionPredictor (the detector seam: its stem and finish)."""
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


_CHILD_MANY = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oar_ocr_amd import api
d, count = sys.argv[2], int(sys.argv[3])
api.prof_enable(True)
for i in range(count):
    eng = api.OrtInfer(open(f"{d}/job{i}.onnx", "rb").read(), profile=True)
    with np.load(f"{d}/job{i}.in.npz") as z:
        feed = [(k, z[k]) for k in z.files]
    api.prof_reset()
    first = eng.infer(feed)
    again = eng.infer(feed)
    names = sorted({e["name"] for e in api.prof_snapshot() if e["launches"]})
    eng.close()
    same = len(first) == len(again) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for (_, a), (_, b) in zip(first, again))
    np.savez(f"{d}/job{i}.out.npz", names=np.array(names), same=np.array(same), **{f"y{j}": a for j, (_, a) in enumerate(first)})
    print("job", i, "done", flush=True)
api.prof_enable(False)
"""


_CHILD_REC = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oar_ocr_amd import api
from oar_ocr_amd.synth import models
d, count = sys.argv[2], int(sys.argv[3])
api.prof_enable(True)
for i in range(count):
    with np.load(f"{d}/job{i}.in.npz") as z:
        crops, classes = list(z["crops"]), int(z["classes"])
    pred = api.TextRecognitionPredictor(open(f"{d}/job{i}.onnx", "rb").read(), api.read_dict(models.synth_dict(classes - 2)))
    api.prof_reset()
    first = pred.predict(crops)
    again = pred.predict(crops)
    names = sorted({e["name"] for e in api.prof_snapshot() if e["launches"]})
    pred.close()
    same = first.indices.tobytes() == again.indices.tobytes() and first.probs.tobytes() == again.probs.tobytes()
    np.savez(f"{d}/job{i}.out.npz", names=np.array(names), same=np.array(same), indices=first.indices, probs=first.probs)
    print("job", i, "done", flush=True)
api.prof_enable(False)
"""


_CHILD_STEM = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oar_ocr_amd import api
d, count = sys.argv[2], int(sys.argv[3])
api.prof_enable(True)
for i in range(count):
    model = open(f"{d}/job{i}.onnx", "rb").read()
    with np.load(f"{d}/job{i}.in.npz") as z:
        images = [z[f"img{j}"] for j in range(int(z["n"]))]
        args = dict(src=tuple(int(v) for v in z["src"]), alpha=z["alpha"], beta=z["beta"], table=bool(z["table"]), wt=int(z["wt"]))
        x = z["x"]
    api.prof_reset()
    first = api.k_stem_u8(model, images, **args)
    again = api.k_stem_u8(model, images, **args)
    names = sorted({e["name"] for e in api.prof_snapshot() if e["launches"]})
    api.prof_reset()
    eng = api.OrtInfer(model, profile=True)
    twin = eng.infer(x)[0][1]
    twin_names = sorted({e["name"] for e in api.prof_snapshot() if e["launches"]})
    eng.close()
    same = first.dtype == again.dtype and first.shape == again.shape and first.tobytes() == again.tobytes()
    np.savez(f"{d}/job{i}.out.npz", names=np.array(names), twin_names=np.array(twin_names), same=np.array(same), y=first, twin=twin)
    print("job", i, "done", flush=True)
api.prof_enable(False)
"""


_CHILD_DET = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oar_ocr_amd import api
d = sys.argv[2]
with np.load(d + "/pages.npz") as z:
    pages = [z[f"page{j}"] for j in range(len(z.files))]
api.prof_enable(True)
pred = api.TextDetectionPredictor(open(d + "/model.onnx", "rb").read())
api.prof_reset()
runs = []
for _ in range(2):
    res = pred.predict(pages)
    runs.append((np.array([len(r) for r in res]), np.array([q.bbox for r in res for q in r], np.float32).reshape(-1, 4, 2), np.array([q.score for r in res for q in r], np.float32)))
names = sorted({e["name"] for e in api.prof_snapshot() if e["launches"]})
api.prof_enable(False)
same = all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], runs[1]))
np.savez(d + "/out.npz", counts=runs[0][0], boxes=runs[0][1], scores=runs[0][2], names=np.array(names), same=np.array(same))
"""


def detect_in_child(model: bytes, pages, env: dict, workdir, timeout: float = 120.0):
    """api.TextDetectionPredictor(model).predict(pages), twice, in a fresh child started with `env` on top of this process's environment -> (counts [pages],
    boxes [sum, 4, 2], scores [sum]) of the first call, the profiler classes that ran, and whether the two calls agreed byte for byte"""
    d = Path(workdir)
    d.mkdir(parents=True, exist_ok=True)
    (d / "model.onnx").write_bytes(model)
    np.savez(d / "pages.npz", **{f"page{j}": np.ascontiguousarray(p, np.uint8) for j, p in enumerate(pages)})
    out = d / "out.npz"
    out.unlink(missing_ok=True)
    r = subprocess.run([sys.executable, "-c", _CHILD_DET, str(ROOT), str(d)], env={**os.environ, **{k: str(v) for k, v in env.items()}},
                       timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0 and out.exists(), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    with np.load(out) as z:
        return (z["counts"], z["boxes"], z["scores"]), {str(n) for n in z["names"]}, bool(z["same"])


class StemResult:
    """one job of stem_many_in_child"""

    def __init__(self, y, twin, names, twin_names, same):
        self.y, self.twin, self.names, self.twin_names, self.same = y, twin, names, twin_names, same


def stem_many_in_child(jobs, env: dict, workdir, timeout: float = 300.0):
    """jobs: [(model bytes, images, dict(src, alpha, beta, table, wt), x)] with images a list of u8 [h, w_i, 3] arrays and x the f32 tensor the stem would
    have seen.  Every job is api.k_stem_u8 twice and the same model once on api.OrtInfer fed x (the twin), in ONE fresh child started with `env` on top of
    this process's environment -> one StemResult per job: y (the first stem run), twin, names and twin_names (the profiler classes that ran during the stem
    runs and during the twin's) and same (were the two stem runs byte-identical?).  One child at a time, its own time limit, never retried."""
    d = Path(workdir)
    d.mkdir(parents=True, exist_ok=True)
    count = 0
    for model, images, args, x in jobs:
        (d / f"job{count}.onnx").write_bytes(model)
        np.savez(d / f"job{count}.in.npz", n=np.array(len(images)), src=np.asarray(args["src"], np.int32), alpha=np.asarray(args["alpha"], np.float32),
                 beta=np.asarray(args["beta"], np.float32), table=np.array(bool(args["table"])), wt=np.array(int(args["wt"])), x=np.ascontiguousarray(x, np.float32),
                 **{f"img{j}": np.ascontiguousarray(im, np.uint8) for j, im in enumerate(images)})
        (d / f"job{count}.out.npz").unlink(missing_ok=True)
        count += 1
    r = subprocess.run([sys.executable, "-c", _CHILD_STEM, str(ROOT), str(d), str(count)], env={**os.environ, **{k: str(v) for k, v in env.items()}},
                       timeout=timeout, capture_output=True, text=True)
    for i in range(count):
        (d / f"job{i}.in.npz").unlink()
    assert r.returncode == 0 and all((d / f"job{i}.out.npz").exists() for i in range(count)), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = []
    for i in range(count):
        with np.load(d / f"job{i}.out.npz") as z:
            res.append(StemResult(z["y"], z["twin"], {str(n) for n in z["names"]}, {str(n) for n in z["twin_names"]}, bool(z["same"])))
        (d / f"job{i}.out.npz").unlink()
    return res


class RecResult:
    """one job of recognize_many_in_child"""

    def __init__(self, indices, probs, names, same):
        self.indices, self.probs, self.names, self.same = indices, probs, names, same


def recognize_many_in_child(jobs, env: dict, workdir, timeout: float = 300.0):
    """jobs: [(model bytes, classes, crops)] with crops a list of equally sized u8 [h, w, 3] images and `classes` the model's vocabulary size (blank and
    space included: the dictionary is models.synth_dict(classes - 2)).  Every job is one TextRecognitionPredictor and two predict() calls in ONE fresh
    child started with `env` on top of this process's environment -> one RecResult per job: indices and probs [n, T] of the first call, names (the
    profiler classes that ran during the job) and same (were the two calls' results byte-identical?).  One child at a time, its own time limit, never
    retried."""
    d = Path(workdir)
    d.mkdir(parents=True, exist_ok=True)
    count = 0
    for model, classes, crops in jobs:
        (d / f"job{count}.onnx").write_bytes(model)
        np.savez(d / f"job{count}.in.npz", crops=np.stack([np.ascontiguousarray(c, np.uint8) for c in crops]), classes=np.array(classes))
        (d / f"job{count}.out.npz").unlink(missing_ok=True)
        count += 1
    r = subprocess.run([sys.executable, "-c", _CHILD_REC, str(ROOT), str(d), str(count)], env={**os.environ, **{k: str(v) for k, v in env.items()}},
                       timeout=timeout, capture_output=True, text=True)
    for i in range(count):
        (d / f"job{i}.in.npz").unlink()
    assert r.returncode == 0 and all((d / f"job{i}.out.npz").exists() for i in range(count)), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = []
    for i in range(count):
        with np.load(d / f"job{i}.out.npz") as z:
            res.append(RecResult(z["indices"], z["probs"], {str(n) for n in z["names"]}, bool(z["same"])))
    return res


def infer_many_in_child(jobs, env: dict, workdir, timeout: float = 300.0):
    """jobs: [(model bytes, {input name: array})] -> one ChildResult per job: outputs() (the first run's arrays, in graph order), names (the profiler
    classes that ran during the job) and same (the job ran twice in the child: were the two runs' outputs byte-identical?).  All jobs run in ONE fresh
    child started with `env` on top of this process's environment -- one child at a time, its own time limit, never retried."""
    d = Path(workdir)
    d.mkdir(parents=True, exist_ok=True)
    count = 0
    for model, feed in jobs:     # (any iterable: a generator keeps one job's inputs in memory at a time)
        (d / f"job{count}.onnx").write_bytes(model)
        np.savez(d / f"job{count}.in.npz", **{k: np.ascontiguousarray(v, np.float32) for k, v in feed.items()})
        out = d / f"job{count}.out.npz"
        if out.exists():
            out.unlink()
        count += 1
    r = subprocess.run([sys.executable, "-c", _CHILD_MANY, str(ROOT), str(d), str(count)], env={**os.environ, **{k: str(v) for k, v in env.items()}},
                       timeout=timeout, capture_output=True, text=True)
    for i in range(count):
        (d / f"job{i}.in.npz").unlink()
    assert r.returncode == 0 and all((d / f"job{i}.out.npz").exists() for i in range(count)), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = []
    for i in range(count):
        with np.load(d / f"job{i}.out.npz") as z:
            res.append(ChildResult(d / f"job{i}.out.npz", {str(n) for n in z["names"]}, bool(z["same"])))
    return res


class ChildResult:
    """one job of infer_many_in_child: names, same, and outputs() -- read from the child's file when asked for, so that a long list of large results
    does not sit in memory at once"""

    def __init__(self, path, names, same):
        self.path, self.names, self.same = path, names, same

    def discard(self):
        """delete the child's file (the caller is done with this job)"""
        Path(self.path).unlink(missing_ok=True)

    def outputs(self):
        with np.load(self.path) as z:
            return [z[f"y{j}"] for j in range(sum(1 for k in z.files if k.startswith("y")))]


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
