"""Engine lanes (OAR_DET_LANES / OAR_REC_LANES): detector sub-batches and recognition batches alternate over several engine
instances on their own streams.  Only the stream a kernel runs on changes, so every entry point returns exactly what one lane
returns, and the profiler counts the same launches per class whatever the lane count."""
import ctypes as C

import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import models, pages

pytestmark = pytest.mark.gpu

ONE_LANE = {"OAR_DET_LANES": "1", "OAR_REC_LANES": "1"}


@pytest.fixture(scope="module")
def nets():
    det, _ = models.build_det("tiny_full", seed=0)
    rec, _ = models.build_rec("tiny_full", vocab=6906, seed=1)
    return det, rec, api.read_dict(models.synth_dict(6904))


def _builder(nets, n_pages):
    det, rec, chars = nets
    cfg = api.TextDetectionConfig(score_threshold=0.3, box_threshold=0.6, unclip_ratio=1.5)
    return api.OAROCRBuilder(det, rec, chars).text_detection_config(cfg).image_batch_size(min(n_pages, 32)).region_batch_size(256)


def _build(nets, n_pages, env, monkeypatch, lanes=1):
    """lane counts are read when the handle is created"""
    for k in ONE_LANE:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ocr = _builder(nets, n_pages).lanes(lanes).build()
    for k in ONE_LANE:
        monkeypatch.delenv(k, raising=False)
    return ocr


def _arrays(pk):
    return [np.asarray(pk.region_offsets), np.asarray(pk.points), np.asarray(pk.scores), np.frombuffer(pk.utf8, np.uint8), np.asarray(pk.text_offsets)]


def _assert_same(a, b):
    for x, y in zip(_arrays(a), _arrays(b)):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def _workload(kind):
    if kind == "mixed":   # several resize groups in one call, tiny (padded) pages included
        sizes = [(960, 960), (480, 640), (20, 30), (960, 960), (1200, 700), (640, 480), (960, 960), (300, 900), (16, 16)]
        return [pages.make_page(50 + i, s, 40 if min(s) > 200 else 1) for i, s in enumerate(sizes)]
    return [pages.make_page(i, (960, 960), 40) for i in range(kind)]


@pytest.mark.parametrize("kind", [32, 1, 5, 13, "mixed"])
def test_default_lanes_equal_one_lane(nets, monkeypatch, kind):
    host = _workload(kind)
    n = len(host)
    _, ptrs, ws, hs = api._img_arrays(host)
    one = _build(nets, n, ONE_LANE, monkeypatch)
    want = one.predict_packed(ptrs, ws, hs, n)
    one.close()
    ocr = _build(nets, n, {}, monkeypatch)
    for _ in range(2):   # a second call reuses every per-lane buffer
        _assert_same(ocr.predict_packed(ptrs, ws, hs, n), want)
    ocr.close()
    if kind == 32:
        assert len(want.scores) > 500


def test_lanes_through_async_and_device_entries(nets, monkeypatch):
    host = _workload(13)
    n = len(host)
    _, ptrs, ws, hs = api._img_arrays(host)
    one = _build(nets, n, ONE_LANE, monkeypatch)
    want = one.predict_packed(ptrs, ws, hs, n)
    one.close()

    ocr = _build(nets, n, {}, monkeypatch, lanes=2)   # two calls in flight, each one using the engine lanes
    tickets = [ocr.submit_packed(ptrs, ws, hs, n) for _ in range(4)]
    for t in tickets:
        _assert_same(ocr.wait_packed(t, n), want)
    ocr.close()

    bufs = [api.DeviceBuffer(p, 0) for p in host]
    try:
        dptrs = (C.c_void_p * n)(*[int(b.ptr.value) for b in bufs])
        ocr = _build(nets, n, {}, monkeypatch)
        _assert_same(ocr.predict_packed(dptrs, ws, hs, n, device=True), want)
        ocr.close()
    finally:
        for b in bufs:
            b.free()


def _profile(ocr, ptrs, ws, hs, n):
    ocr.predict_packed(ptrs, ws, hs, n)
    api.prof_filter("")
    api.prof_sampling(1, 0)
    api.prof_enable(True)
    api.prof_reset()
    try:
        ocr.predict_packed(ptrs, ws, hs, n)
        return {e["name"]: e for e in api.prof_snapshot() if e["launches"] > 0}
    finally:
        api.prof_enable(False)


def test_profiler_counts_and_times_each_launch_alone(nets, monkeypatch):
    host = _workload(32)
    n = len(host)
    _, ptrs, ws, hs = api._img_arrays(host)
    one = _build(nets, n, ONE_LANE, monkeypatch)
    a = _profile(one, ptrs, ws, hs, n)
    one.close()
    ocr = _build(nets, n, {}, monkeypatch)
    b = _profile(ocr, ptrs, ws, hs, n)
    ocr.close()
    assert {k: v["launches"] for k, v in a.items()} == {k: v["launches"] for k, v in b.items()}
    # every launch is sampled here, so every lane launch is fenced: the classes that carry most of the time keep their
    # single-lane durations (overlapping launches would each be charged the other lane's work as well)
    top = sorted(a.values(), key=lambda e: -e["total_ms"])[:4]
    for e in top:
        ratio = b[e["name"]]["total_ms"] / e["total_ms"]
        assert 0.7 < ratio < 1.3, (e["name"], e["total_ms"], b[e["name"]]["total_ms"])
