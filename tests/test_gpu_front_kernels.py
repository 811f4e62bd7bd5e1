"""The byte-level kernels every inference enters and leaves through, called directly: the u8 RGB stem k::conv_smallcin_u8 in all six
instantiations, the crop resize pp::rec_resize_u8, pp::normalize_pages, and the detector's finish pp::db_keep_and_pack / pp::pack_mask_bits.

The stem's case table, byte families, expected detail names and references live in oar_ocr_amd/synth/front_cases.py.  All stem cases of one switch group run
in ONE child process started with OAR_PROF_DETAIL=1 (read once per process, as OAR_STEM_SW is), every job twice.  Per case and byte family: the detail name
that ran is front_cases.form's; two runs agree byte for byte; the output equals, bit for bit, the same model run by api.OrtInfer on the f32 tensor the stem
would have seen (the twin runs k::conv_smallcin_kernel: both kernels issue the same fmaf sequence per output channel, from the same bias, over the same taps
-- the equality follows from the code, not from a measurement); with OAR_STEM_SW=0 the output is the default's, bit for bit; and on its own, max |y - f64| / S
<= tol_S over the whole output (f32_cases.bundle on the normalised f32 values; a HardSwish layer is compared in front of its activation).  The other kernels
are exact: every byte, bit and float is compared with the oracle's CPU routine or a numpy expression."""
import shutil

import numpy as np
import pytest

from oar_ocr_amd import api
from oar_ocr_amd.synth import f32_cases, models, pages
from oar_ocr_amd.synth import front_cases as F
from oar_ocr_amd.synth.child_run import detect_in_child, stem_many_in_child
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu
_RUNS = {}      # group -> {job key: StemResult}: the group's child ran (once: a failed child is not started again)
_DET = {}       # switch -> what detect_in_child returned


@pytest.fixture(scope="module")
def workroot(tmp_path_factory):
    root = tmp_path_factory.mktemp("front")
    yield root
    shutil.rmtree(root, ignore_errors=True)


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _lg(v):
    return f"2^{np.log2(v):.1f}" if v > 0 else "0"


# ================================================================================================ the stem
def _args(c, inp):
    return dict(src=c.src, alpha=inp["alpha"], beta=inp["beta"], table=c.table, wt=c.w)


def _jobs(c):
    """-> (key, model, images, arguments, twin input) per byte family; a HardSwish layer also without its activation"""
    for fam in F.BYTE_FAMILIES:
        inp = F.inputs(c, fam)
        x = F.stem_tensor(c, inp)
        yield (c.name, fam), F.model(c, inp), inp["images"], _args(c, inp), x
        if c.act == "hswish":
            yield (c.name, fam, "linear"), F.model(c, inp, act=None), inp["images"], _args(c, inp), x


def _runs(group, workroot):
    if group not in _RUNS:
        assert None not in _RUNS.values() and None not in _DET.values(), "an earlier child failed: no further GPU work is started by this module"
        _RUNS[group] = None
        keys, jobs = [], []
        for c in F.cases_of(group):
            for key, *job in _jobs(c):
                keys.append(key)
                jobs.append(tuple(job))
        res = stem_many_in_child(jobs, {"OAR_PROF_DETAIL": "1", **F.GROUPS[group]}, workroot / group, timeout=240.0)
        _RUNS[group] = dict(zip(keys, res))
    assert _RUNS[group] is not None, f"the child of group {group} failed in an earlier test"
    return _RUNS[group]


def _check_run(c, res, env):
    """(a) the stem's launch carries the predicted detail name, the twin's convolution its own; (b) two runs agree; (c) the stem equals its twin"""
    stem_names = {n for n in res.names if n.startswith("conv_")}
    assert stem_names == {F.form(c, env)}, (c.name, F.form(c, env), sorted(res.names))
    assert {n for n in res.twin_names if n.startswith("conv_")} == {F.twin_form(c)}, (c.name, F.twin_form(c), sorted(res.twin_names))
    assert res.same, (c.name, "two runs of the same bytes differ")
    ho, wo = c.out_hw
    assert res.y.shape == (c.n, c.cout, ho, wo) and res.y.dtype == np.float32, (c.name, res.y.shape)
    if not np.array_equal(res.y, res.twin) or not _bits(res.y, res.twin):
        bad = np.argwhere(res.y.view(np.uint32) != res.twin.view(np.uint32))
        raise AssertionError((c.name, "the stem and its twin differ", F.form(c, env), F.twin_form(c), len(bad), bad[:8].tolist()))


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_stem(name, workroot):
    c = F.case_by_name(name)
    runs = _runs("default", workroot)
    for fam in F.BYTE_FAMILIES:
        inp = F.inputs(c, fam)
        b = F.bundle(c, inp)
        assert np.isfinite(b["tol_S"]) and b["tol_S"] < 2.0 ** -14, (name, fam, b["tol_S"])
        res = runs[(name, fam)]
        _check_run(c, res, {})
        got = res.y
        if c.act == "hswish":
            # in front of the activation the bound is defined; behind it: HardSwish has slope <= 1.5 and its own three f32 roundings, each <= 2^-24 |y| <= 2^-24 S
            lin = runs[(name, fam, "linear")]
            _check_run(c, lin, {})
            act, got = got, lin.y
            e_act = f32_cases.err_S(act, f32_cases.act_ref(b["f64"], "hswish"), b["S"])
            assert e_act <= 1.5 * b["tol_S"] + 2.0 ** -22, (name, fam, "behind HardSwish", e_act, b["tol_S"])
        assert np.isfinite(got).all(), (name, fam)
        err = F.error(c, got, b)
        print(f"\n[front] {name} | {F.form_key(c)} | {fam} | noise_S {_lg(b['noise_S'])} | tol_S {_lg(b['tol_S'])} | err_S {_lg(err)}")
        assert err <= b["tol_S"], (name, fam, err, b["tol_S"])
        if c.identity:      # (f) the normalisation's own bits
            if c.table:
                want = R.rec_preprocess(inp["images"], img_h=c.h, img_w=c.w, max_img_w=c.w)
                assert want.shape == got.shape and (want[1, :, :, 1:] == 0).all(), (name, want.shape)      # image 1 is one pixel wide: 39 padding columns
            else:
                want = np.stack([R.normalize(im, inp["alpha"], inp["beta"], c.src, "chw") for im in inp["images"]])
            assert _bits(got, want), (name, fam, "the identity stem does not return the normalised tensor")


@pytest.mark.parametrize("name", [c.name for c in F.cases_of("sw_off")])
def test_stem_without_the_scalar_cache_route(name, workroot):
    """(d) OAR_STEM_SW=0 moves every full-group 3x3 stem to the LDS instantiation: same name but for the last word, same bits"""
    c = F.case_by_name(name)
    env = F.GROUPS["sw_off"]
    assert F.form(c, env) == F.form(c)[:-2] + "lds"
    base, off = _runs("default", workroot), _runs("sw_off", workroot)
    for key in [k for k in off if k[0] == name]:
        _check_run(c, off[key], env)
        assert _bits(off[key].y, base[key].y), (key, "OAR_STEM_SW=0 changes the output")


def _one_conv(cout, k, n, h, w):
    c = F.StemCase("refusal", cout, k, k, n, h, w, pads=(k // 2,) * 4)
    inp = F.inputs(c, "random")
    return c, inp, F.model(c, inp)


def test_stem_refusals():
    c, inp, m = _one_conv(8, 7, 1, 9, 11)      # K = 147: stem_fusable() is false
    with pytest.raises(api.OCRError) as e:
        api.k_stem_u8(m, inp["images"], c.src, inp["alpha"], inp["beta"])
    assert e.value.code == api.OAR_UNSUPPORTED_OP and "fusable RGB stem" in str(e.value)
    c, inp, m = _one_conv(8, 3, 33, 4, 5)
    with pytest.raises(api.OCRError) as e:
        api.k_stem_u8(m, inp["images"], c.src, inp["alpha"], inp["beta"])
    assert e.value.code == api.OAR_INVALID_INPUT and "at most 32 pages" in str(e.value)
    c, inp, m = _one_conv(8, 3, 2, 4, 5)
    with pytest.raises(api.OCRError) as e:
        api.k_stem_u8(m, inp["images"], c.src, inp["alpha"], inp["beta"], table=True, wt=4)
    assert e.value.code == api.OAR_INVALID_INPUT and "wider than the tensor" in str(e.value)
    assert api.k_stem_u8(m, inp["images"], c.src, inp["alpha"], inp["beta"]).shape == (2, 8, 4, 5)      # the same call, allowed


# ================================================================================================ rec_resize_u8
SENTINEL = 0xA5


def _check_resize(crops, flips, img_h=48):
    got, wt, pool = api.k_rec_resize_u8(crops, flips, img_h=img_h, sentinel=SENTINEL)
    tw, rws = R.rec_tensor_width([(c.shape[1], c.shape[0]) for c in crops], img_h)
    assert wt == tw and [g.shape for g in got] == [(img_h, int(rw), 3) for rw in rws]
    outside = np.ones(pool.size, bool)
    off = 0
    for i, (c, g) in enumerate(zip(crops, got)):
        want = R.resize_triangle(R.rotate_rgb(c, 2) if flips is not None and flips[i] else c, int(rws[i]), img_h)
        assert np.array_equal(g, want), (i, c.shape, int(rws[i]), int((g != want).sum()))
        outside[off:off + g.size] = False
        off += (g.size + 63) & ~63
    assert off == pool.size and (pool[outside] == SENTINEL).all(), ("a byte outside the images was written", np.flatnonzero(outside & (pool != SENTINEL))[:8].tolist())
    return got, wt


def _crops(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (w, h) in sizes]


@pytest.mark.parametrize("flips", ["none", "all", "mixed"])
def test_rec_resize_u8_over_the_scale_range(flips):
    crops = _crops(F.RESIZE_SIZES, 31)      # more than 8 vertical taps (300 rows -> 48), the identity copy (96 x 48), widths capped at the tensor's
    fl = {"none": None, "all": [True] * len(crops), "mixed": [i % 3 == 1 for i in range(len(crops))]}[flips]
    _check_resize(crops, fl)


@pytest.mark.parametrize("img_h", [48, 32])
def test_rec_resize_u8_batches(img_h):
    _check_resize(_crops([(77, 31)], 5), None, img_h)                                 # n = 1
    _check_resize(_crops([(2600, 40), (3, 9)], 6), [False, True], img_h)              # the grid is sized by the widest image: the 3-pixel crop's blocks find nothing to do
    _check_resize(_crops(F.RESIZE_SIZES[:6], 7), [i % 2 == 0 for i in range(6)], img_h)


def test_rec_resize_u8_feeds_the_table_stem(workroot):
    """the two kernels chained as the recognizer chains them: resized u8 images -> table stem (BGR) == the model on api.k_rec_preprocess of the same crops"""
    crops = _crops([(96, 48), (31, 48), (3, 9), (200, 12), (333, 24)], 8)
    flips = [False, True, False, False, True]
    imgs, wt = _check_resize(crops, flips)
    c = F.StemCase("chained", 16, 3, 3, len(crops), 48, wt, pads=(1, 1, 1, 1), src=(2, 1, 0), widths=tuple(im.shape[1] for im in imgs))
    inp = F.inputs(c, "random")
    m = F.model(c, inp)
    got = api.k_stem_u8(m, imgs, (2, 1, 0), table=True, wt=wt)
    x = api.k_rec_preprocess(crops, flips=flips)
    assert x.shape == (len(crops), 3, 48, wt)
    eng = api.OrtInfer(m)
    twin = eng.infer(x)[0][1]
    eng.close()
    assert _bits(got, twin), ("the chained front end and the packed-tensor route differ", int((got != twin).sum()))


# ================================================================================================ normalize_pages
ALPHA, BETA = np.float32([0.017, 0.0171, 0.0169]), np.float32([-2.1, -2.0, -1.8])


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("src", [(0, 1, 2), (2, 1, 0)])
def test_normalize_pages(layout, src):
    rng = np.random.default_rng(11)
    for h, w in F.NORMALIZE_PLANES:
        for n in F.NORMALIZE_N:
            pg = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
            want = np.stack([R.normalize(p, ALPHA, BETA, src, layout) for p in pg])
            size = h * w * 3
            packed = api.k_normalize_pages(pg, ALPHA, BETA, src, layout)
            assert _bits(packed, want), (h, w, n, "back to back")
            for shift in range(4):      # page i begins (i + shift) % 4 bytes past a 4-byte boundary: every residue, in every position of the batch
                offs = [i * ((size + 3) // 4 * 4 + 8) + (i + shift) % 4 for i in range(n)]
                got = api.k_normalize_pages(pg, ALPHA, BETA, src, layout, byte_offsets=offs)
                assert _bits(got, want), (h, w, n, shift)


def test_normalize_pages_refuses_33_pages():
    pg = [np.zeros((2, 2, 3), np.uint8)] * 33
    with pytest.raises(api.OCRError) as e:
        api.k_normalize_pages(pg, ALPHA, BETA)
    assert e.value.code == api.OAR_INVALID_INPUT and "at most 32 pages" in str(e.value)


# ================================================================================================ db_keep_and_pack / pack_mask_bits
THRESH = np.float32(0.3)


def _net_out(rng, n, ch, h, w):
    x = rng.random((n, ch, h, w)).astype(np.float32)
    special = [THRESH, np.nextafter(THRESH, np.float32(1)), np.nextafter(THRESH, np.float32(0)), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0)]
    flat = x[:, 0].reshape(-1)
    at = rng.permutation(flat.size)
    for i, v in enumerate(special * 2):
        if i < flat.size:
            flat[at[i]] = v
    x[:, 0] = flat.reshape(n, h, w)
    return x


def test_db_keep_and_pack():
    rng = np.random.default_rng(12)
    seen = set()
    for w in F.FINISH_W:
        for h in F.FINISH_H:
            for n in F.FINISH_N:
                for ch in F.FINISH_C:      # two channels and an odd plane: image 1's channel 0 begins off its alignment
                    x = _net_out(rng, n, ch, h, w)
                    seen |= {v.tobytes() for v in x[:, 0].reshape(-1)[np.isin(x[:, 0].reshape(-1).view(np.uint32), np.float32([0.3, -0.0, np.inf, -np.inf]).view(np.uint32))]}
                    with np.errstate(invalid="ignore"):
                        want_bits = np.packbits(x[:, 0] > THRESH, axis=-1, bitorder="little")
                    for off in range(4):
                        probs, bits = api.k_db_keep_and_pack(x, float(THRESH), float_offset=off)
                        assert _bits(probs, np.ascontiguousarray(x[:, 0])), (w, h, n, ch, off, "probs")
                        assert _bits(bits, want_bits), (w, h, n, ch, off, "bits")
                    mask = api.k_threshold(np.ascontiguousarray(x[:, 0]), float(THRESH))
                    assert set(np.unique(mask)) <= {0, 255}
                    assert _bits(api.k_pack_mask_bits(mask), want_bits), (w, h, n, ch, "threshold + pack_mask_bits")
    assert len(seen) == 4      # the threshold itself, -0.0 and both infinities were among the inputs (NaN and the neighbours are set with them)


def test_pack_mask_bits():
    rng = np.random.default_rng(13)
    for w in F.FINISH_W:
        for h in F.FINISH_H:
            for n in F.FINISH_N:
                mask = rng.choice(np.uint8([0, 0, 1, 128, 255]), (n, h, w))
                want = np.packbits(mask != 0, axis=-1, bitorder="little")
                for off in range(8):
                    assert _bits(api.k_pack_mask_bits(mask, byte_offset=off), want), (w, h, n, off)


# ================================================================================================ the detector seam
DET_ROUTES = {"default": {}, "stem_off": {"OAR_FUSE_STEM": "0"}, "finish_off": {"OAR_DB_FINISH_FUSED": "0"}}


def _det(route, workroot):
    if route not in _DET:
        assert None not in _RUNS.values() and None not in _DET.values(), "an earlier child failed: no further GPU work is started by this module"
        _DET[route] = None
        det, _ = models.build_det("tiny", seed=0)
        pg = [pages.make_page(0, (320, 480), lines=6), pages.make_page(1, (300, 450), lines=6)]      # the second is resized to a multiple of 32
        _DET[route] = detect_in_child(det, pg, {"OAR_PROF_DETAIL": "1", **DET_ROUTES[route]}, workroot / ("det_" + route))
    assert _DET[route] is not None, f"the child of route {route} failed in an earlier test"
    return _DET[route]


def test_detector_routes_agree(workroot):
    """fused stem against normalize_pages + the f32 stem, fused finish against copy2d + threshold + pack_mask_bits: the same boxes and scores, exactly"""
    (counts, boxes, scores), names, same = _det("default", workroot)
    assert same and counts.shape == (2,) and counts.min() >= 1, counts
    stem = lambda ns: sorted(n for n in ns if n.startswith("conv_smallcin"))
    assert all(n.startswith("conv_smallcin_u8 ") and " pages " in n for n in stem(names)) and len(stem(names)) == 2, stem(names)      # one per page size
    assert "resize_triangle" in names and "threshold" in names and not {"normalize", "pack_mask"} & names, sorted(names)
    (c1, b1, s1), n1, same1 = _det("stem_off", workroot)
    assert same1 and "normalize" in n1 and all(n.startswith("conv_smallcin px=") for n in stem(n1)) and len(stem(n1)) == 2, sorted(n1)
    (c2, b2, s2), n2, same2 = _det("finish_off", workroot)
    assert same2 and {"pack_mask", "threshold"} <= n2 and "normalize" not in n2 and stem(n2) == stem(names), sorted(n2)
    for c, b, s in ((c1, b1, s1), (c2, b2, s2)):
        assert _bits(c, counts) and _bits(b, boxes) and _bits(s, scores)
