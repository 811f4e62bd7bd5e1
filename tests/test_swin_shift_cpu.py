"""Shifted, masked and padded Swin windows, host side: the builders' default bytes, the new spellings through the ONNX oracles against the
torch f64 reference, inputs that tell a wrong roll / mask / pad-key rule from the right one, the kernel's address map (kernels.h, compiled for the host and
checked exhaustively, once more under the address and undefined-behaviour sanitizers), the kernel's resources, and the conditioning of the encoder that
tests/test_gpu_swin_shift.py decodes."""
import hashlib
import re
import subprocess

import numpy as np
import pytest

from oar_ocr_amd import build, formula
from oar_ocr_amd.synth import models
from oar_ocr_amd.synth.formula_reference import formula_reference_bundle
from oar_ocr_amd.synth.unimernet_reference import reference_bundle, swin_block_reference, unimernet_encoder_reference

#          B   H   W   C nh  ws  s  mask          (the shapes of tests/test_gpu_swin_shift.py)
SHAPES = [(2, 10, 13, 24, 3, 7, 3, "swin"),      # padded on both axes, shifted, 4 windows
          (1, 8, 8, 16, 2, 4, 2, "swin"),        # aligned, shifted
          (1, 8, 12, 16, 2, 4, 2, "random"),     # mask indexing, 6 windows, hb != wb
          (1, 9, 6, 32, 1, 4, 0, None),          # padded only: pad keys carry the k / v biases
          (2, 6, 12, 16, 2, 6, 3, "swin"),       # one window row, the roll wraps inside it
          (1, 16, 32, 32, 1, 16, 8, "swin"),     # N = 256, with a mask
          (1, 8, 8, 16, 2, 4, 0, "random")]      # a mask without a roll
IDS = ["B%d_H%d_W%d_C%d_nh%d_ws%d_s%d_%s" % s for s in SHAPES]
ORACLE_TOL = 64 * 4 * 2.0 ** -23                 # tests/test_unimernet_cpu.py's rule: 64 times the f32 rounding of values up to ~5

_cache = {}


def random_mask(H, W, ws):
    """U(-4, 0) per (window, i, j): no two windows, rows or columns alike"""
    nW = -(-H // ws) * -(-W // ws)
    return (-4.0 * np.random.default_rng(5).random((nW, ws * ws, ws * ws))).astype(np.float32)


def _case(shape, scale="div"):
    """model, info, input, reference bundle: computed once, never modified"""
    if (shape, scale) not in _cache:
        B, H, W, C, nh, ws, s, mask = shape
        model, info = models.build_swin_block(H, W, C, nh, ws, seed=3, scale=scale, shift=s, mask=random_mask(H, W, ws) if mask == "random" else mask, pad_value=0.0)
        x = np.random.default_rng(11).standard_normal((B, H * W, C)).astype(np.float32)
        _cache[(shape, scale)] = (model, info, x, reference_bundle(swin_block_reference, info, x))
    return _cache[(shape, scale)]


def _rows(H, W, ws, sy, sx):
    """[nW, N]: the image-order row of every window's every token, -1 for padding -- numpy's pad -> roll -> partition of an index grid"""
    hb, wb = -(-H // ws), -(-W // ws)
    g = np.pad(np.arange(H * W).reshape(H, W), ((0, hb * ws - H), (0, wb * ws - W)), constant_values=-1)
    g = np.roll(g, (-sy, -sx), (0, 1))
    return g.reshape(hb, ws, wb, ws).transpose(0, 2, 1, 3).reshape(hb * wb, ws * ws)


def _by_address(info, x, variant=None):
    """The block as DESIGN 4.33.1 states it for the kernel, in numpy f64: q, k, v of LN1(x) in image order; a window gathers its rows through the address
    map; a padding token is a key with the k / v biases and no query; scale, bias, mask in that order; the output goes back to the same rows.
    variant: one of the wrong readings that test_the_inputs_can_tell_wrong_readings_apart lists."""
    w = {k: np.asarray(v, np.float64) for k, v in info["weights"].items()}
    H, W, C, nh, ws = info["H"], info["W"], info["C"], info["nh"], info["ws"]
    s, mask = info.get("shift", 0), info.get("mask")
    N, dh = ws * ws, C // nh
    x = np.asarray(x, np.float64)
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + 1e-5) * w["ln1_g"] + w["ln1_b"]
    q, k, v = (y @ w["w" + n].T + w["b" + n] for n in "qkv")
    rows = _rows(H, W, ws, 0 if variant == "shift 0" else s, 0 if variant in ("shift 0", "one axis") else s)
    if mask is not None:
        mask = np.asarray(mask, np.float64)
        mask = None if variant == "no mask" else np.broadcast_to(mask[:1], mask.shape) if variant == "mask of window 0" else mask
    c = np.float64(np.float32(np.sqrt(dh))) if info["scale"] == "div" else np.float64(np.float32(dh ** -0.5))
    o = np.zeros_like(x)
    for b in range(x.shape[0]):
        for wi, r in enumerate(rows):
            real = r >= 0
            kw = np.where(real[:, None], k[b, r], 0.0 if variant == "zero pad keys" else w["bk"])      # (r = -1 reads the last row: replaced here)
            vw = np.where(real[:, None], v[b, r], 0.0 if variant == "zero pad keys" else w["bv"])
            for h in range(nh):
                hs = slice(h * dh, (h + 1) * dh)
                sc = q[b, r[real]][:, hs] @ kw[:, hs].T
                sc = (sc / c if info["scale"] == "div" else sc * c) + w["bias"][h][real]
                if mask is not None:
                    sc = sc + mask[wi][real]
                if variant == "pad keys excluded":
                    sc = np.where(real[None, :], sc, -np.inf)
                e = np.exp(sc - sc.max(-1, keepdims=True))
                o[b, r[real], hs] = (e / e.sum(-1, keepdims=True)) @ vw[:, hs]
    return x + o @ w["wp"].T + w["bp"]


# ------------------------------------------------------------------------------------------------ the builders
def test_default_bytes_are_those_of_the_parent():
    """with shift, mask and pad_value at their defaults the builders write what they wrote before these keywords existed: SHA-256 as computed on the parent"""
    sha = lambda m: hashlib.sha256(m[0]).hexdigest()
    assert sha(models.build_swin_block(14, 21, 24, 3, 7, seed=3)) == "8846212ecc6f31f685bc0af9ed7e676f8955265dd9204d6e8ba97a39b9c79734"
    assert sha(models.build_swin_block(14, 21, 24, 3, 7, seed=3, whole=True)) == "15c2f4cbf550bda5a21516b70345b6b8f266fb97b943050583acba3e3fb1e4a1"
    assert sha(models.build_unimernet()) == "04f5d76c4d2e6253280b7d5104ef61ca594befa9df553d0b2271943c1e2379b7"
    assert models.build_swin_block(14, 21, 24, 3, 7, seed=3, shift=0, mask=None, pad_value=0.0)[0] == models.build_swin_block(14, 21, 24, 3, 7, seed=3)[0]
    assert models.build_unimernet(shifted=False)[0] == models.build_unimernet()[0]


def test_swin_mask_is_the_standard_one():
    """8 x 8, ws 4, shift 2, worked out by hand: window 0 lies in one region (no -100); window 1 (top right) splits at column 2 of the window; window 3 in four"""
    m = models.swin_shift_mask(8, 8, 4, 2)
    assert m.shape == (4, 16, 16) and m.dtype == np.float32 and set(np.unique(m)) == {-100.0, 0.0}
    assert not m[0].any()
    col = np.arange(16) % 4 >= 2
    assert np.array_equal(m[1] != 0, col[:, None] != col[None, :])
    quad = (np.arange(16) // 4 >= 2) * 2 + col
    assert np.array_equal(m[3] != 0, quad[:, None] != quad[None, :])
    assert models.swin_shift_mask(10, 13, 7, 3).shape == (4, 49, 49)                                # on the padded 14 x 14 grid
    with pytest.raises(ValueError):
        models.build_swin_block(8, 8, 16, 2, 4, shift=8)                                           # shift >= min(Hp, Wp)
    with pytest.raises(ValueError):
        models.build_swin_block(8, 8, 16, 2, 4, mask=np.zeros((3, 15, 16), np.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_new_spellings_compute_what_the_reference_computes(shape):
    """The graph through the ONNX oracle against synth/unimernet_reference.py in f64, test_unimernet_cpu.py's tolerance.  oracle/onnx_np.py (f64) has no Pad,
    so a padded graph goes through oracle/onnx_ref.py, the same interpreter over torch f32, which has one."""
    from oracle import onnx_np, onnx_ref
    for scale in ("div", "mul"):
        model, info, x, ref = _case(shape, scale)
        padded = info["H"] % info["ws"] or info["W"] % info["ws"]
        got = np.asarray((onnx_ref if padded else onnx_np).run(onnx_ref.parse_model(model), {"x": x})[0], np.float64)
        err = float(np.abs(got - ref["f64"]).max())
        print(f"{shape} {scale}: oracle err {err:.2e} tol {ORACLE_TOL:.2e}")
        assert got.shape == ref["f64"].shape and err <= ORACLE_TOL, (err, ORACLE_TOL)


def test_fall_back_spellings_compute_what_the_reference_computes():
    """pad_value = 1.0 and a reverse roll that is not the forward one: the reference models both"""
    from oracle import onnx_ref
    x = np.random.default_rng(11).standard_normal((2, 10 * 13, 24)).astype(np.float32)
    for kw in (dict(pad_value=1.0), dict(unroll=2)):
        model, info = models.build_swin_block(10, 13, 24, 3, 7, seed=3, shift=3, mask="swin", **{"pad_value": 0.0, **kw})
        got = np.asarray(onnx_ref.run(onnx_ref.parse_model(model), {"x": x})[0], np.float64)
        assert float(np.abs(got - swin_block_reference(info, x)).max()) <= ORACLE_TOL
        plain = dict(info, pad_value=0.0, unroll=3)
        assert float(np.abs(swin_block_reference(plain, x) - swin_block_reference(info, x)).max()) > 1e-2     # (and the fall-back form is not the matched one)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_inputs_can_tell_wrong_readings_apart(shape):
    """The by-address statement of the block equals the torch reference, and every wrong reading of it that applies to the shape -- the mask dropped, window
    0's mask for all windows, no shift, the shift on one axis only, padding keys left out of the soft-max, padding keys with zero k / v instead of the
    Linears' biases -- moves the output by more than 100 tol, tol the larger of the oracle's and the GPU test's (max(16 noise, 2^-19))."""
    B, H, W, C, nh, ws, s, mask = shape
    model, info, x, ref = _case(shape)
    tol = max(ORACLE_TOL, ref["tol"])
    assert float(np.abs(_by_address(info, x) - ref["f64"]).max()) <= 1e-11
    padded = bool(H % ws or W % ws)
    applies = {"no mask": mask is not None, "mask of window 0": mask is not None and info["mask"].shape[0] > 1, "shift 0": s > 0, "one axis": s > 0,
               "pad keys excluded": padded, "zero pad keys": padded}
    assert any(applies.values())
    for variant, on in applies.items():
        if on:
            d = float(np.abs(_by_address(info, x, variant) - ref["f64"]).max())
            print(f"{shape} {variant}: moves the output by {d:.2e} | 100 tol {100 * tol:.2e}")
            assert d > 100 * tol, (variant, d, tol)


# ------------------------------------------------------------------------------------------------ the kernel's address map and resources
MAP_MAIN = r'''
#include <cstdio>
#include "kernels.h"
int main() {
    for (int ws = 1; ws <= 5; ++ws) for (int s = 0; s < ws; ++s) for (int H = 1; H <= 11; ++H) for (int W = 1; W <= 11; ++W) {
        const int hb = (H + ws - 1) / ws, wb = (W + ws - 1) / ws;
        std::printf("%d %d %d %d", H, W, ws, s);
        for (int wy = 0; wy < hb; ++wy) for (int wx = 0; wx < wb; ++wx) for (int n = 0; n < ws * ws; ++n)
            std::printf(" %d", oar::k::window_token_row(wy, wx, n, ws, H, W, hb * ws, wb * ws, s));
        std::printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def map_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wa_map")
    (d / "wa_map.cpp").write_text(MAP_MAIN)
    base = [build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", str(build.CSRC), "-I", str(build.CSRC.parent.parent / "include"), str(d / "wa_map.cpp")]
    for exe, flags in (("wa_map", ["-O0"]), ("wa_map_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        r = subprocess.run(base + flags + ["-o", str(d / exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
    return d


def test_address_map_is_pad_roll_partition(map_programs):
    """k::window_token_row for every (H, W, ws, s), 1 <= ws <= 5, H, W <= 11, 0 <= s < ws, against numpy's pad -> roll -> partition of an index grid; the real
    rows of all windows are a permutation of 0 .. H W - 1 (every token is read, and written, exactly once)"""
    out = subprocess.run([str(map_programs / "wa_map")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 15 * 121
    seen = set()
    for line in lines:
        v = np.array(line.split(), np.int64)
        H, W, ws, s = (int(t) for t in v[:4])
        want = _rows(H, W, ws, s, s).reshape(-1)
        assert np.array_equal(v[4:], want), (H, W, ws, s)
        assert np.array_equal(np.sort(want[want >= 0]), np.arange(H * W)), (H, W, ws, s)
        seen.add((H, W, ws, s))
    assert len(seen) == 15 * 121 and (11, 11, 5, 4) in seen and (1, 1, 1, 0) in seen


def test_address_map_is_clean_under_the_sanitizers(map_programs):
    """the same program, stand-alone with its own main, under -fsanitize=address,undefined with no recovery: ends clean and prints the same"""
    plain = subprocess.run([str(map_programs / "wa_map")], capture_output=True, text=True)
    san = subprocess.run([str(map_programs / "wa_map_san")], capture_output=True, text=True)
    assert san.returncode == 0 and "runtime error" not in san.stderr and "Sanitizer" not in san.stderr, san.stderr[-2000:]
    assert san.stdout == plain.stdout


def test_window_attention_kernel_keeps_its_resources(tmp_path):
    """window_attention.hip after the shift, the mask and the padding became run-time fields of its one kernel: still one kernel, no scratch, no spills, at
    most 128 registers, no static LDS, and the dynamic LDS formula unchanged (71,680 bytes at most; 10,960 at N = 36, 40,768 at N = 144, dh = 32)"""
    src = build.CSRC / "window_attention.hip"
    assert "window_attention.hip" in build.SOURCES
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
    assert len(kernels) == 1 and "window_attention_kernel" in next(iter(kernels)), sorted(kernels)
    v = next(iter(kernels.values()))
    print(v)
    assert v["spill"] == 0 and v["scratch"] == 0 and v["vgprs"] <= 128 and v["lds"] == 0, v
    prog = tmp_path / "wa_lds.cpp"
    prog.write_text('#include <cstdio>\n#include "kernels.h"\nint main() { size_t m = 0; for (int ws = 1; ws * ws <= oar::k::kWinMaxN; ++ws) for (int d = 1; d <= oar::k::kWinMaxDh; ++d) '
                    'if (ws * ws * d <= oar::k::kWinMaxNd) { size_t b = oar::k::window_attention_lds_bytes(ws * ws, d); if (b > m) m = b; } '
                    'std::printf("%zu %zu %zu\\n", m, oar::k::window_attention_lds_bytes(36, 32), oar::k::window_attention_lds_bytes(144, 32)); return 0; }\n')
    exe = tmp_path / "wa_lds"
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O0", "-I", str(build.CSRC), "-I", str(build.CSRC.parent.parent / "include"), str(prog), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["71680", "10960", "40768"], (out.stdout, out.stderr)


# ------------------------------------------------------------------------------------------------ the encoder that pads and shifts
ENC = dict(image_shape=(64, 96), ws=7, shifted=True, depths=(2, 2), V=61, M=24, seed=1)            # tests/test_gpu_swin_shift.py builds the same


def enc_crop(seed):
    """a 96 x 64 crop with ink in two opposite corners: the margin crop keeps it whole and both resizes are the identity"""
    rng = np.random.default_rng(seed)
    img = np.full((64, 96, 3), 245, np.uint8)
    img[0, 0] = img[63, 95] = 0
    for _ in range(10):
        y, x = int(rng.integers(4, 52)), int(rng.integers(4, 78))
        img[y:y + int(rng.integers(2, 6)), x:x + int(rng.integers(4, 14))] = (int(rng.integers(0, 90)), int(rng.integers(0, 90)), int(rng.integers(0, 90)))
    return img


def test_padding_shifting_encoder_graph_and_its_conditioning():
    """build_unimernet(image_shape=(64, 96), ws=7, shifted=True): token grids 16 x 24 (padded to 21 x 28) and 8 x 12 (to 14 x 14).  The graph through the
    oracle equals the f64 encoder; and what the GPU test's predictor check relies on holds for the chosen seed: f32 and f64 decode the same tokens with a
    top-two logit gap >= 8 tol.  An odd grid in front of a patch merging stays refused."""
    from oracle import onnx_ref
    enc_model, info = models.build_unimernet(encoder_only=True, **ENC)
    assert info["S"] == 8 * 12 and info["encoder"]["shifted"] is True
    text = models.build_unimernet(**ENC)[0]
    assert text != models.build_unimernet(**dict(ENC, shifted=False))[0]
    t = formula.UniMERNetPreprocessor(target_size=(96, 64)).preprocess_batch([enc_crop(1), enc_crop(2)])
    assert t.shape == (2, 1, 64, 96)
    enc = reference_bundle(unimernet_encoder_reference, info["encoder"], t)
    got = np.asarray(onnx_ref.run(onnx_ref.parse_model(enc_model), {"x": t})[0], np.float64)
    assert got.shape == (2, 96, 64) and float(np.abs(got - enc["f64"]).max()) <= ORACLE_TOL
    plain = unimernet_encoder_reference({k: v for k, v in info["encoder"].items() if k != "shifted"}, t)
    assert float(np.abs(plain - enc["f64"]).max()) > 1e-2                                          # the shift and its mask matter to `memory`
    w = models.build_unimernet(**ENC)[1]["weights"]
    ref = formula_reference_bundle(w, enc["f64"], ENC["M"])
    print(f"gap {ref['gap']:.2e} tol {ref['tol']:.2e} tokens {ref['tokens'].tolist()}")
    assert np.array_equal(ref["f32"]["tokens"], ref["f64"]["tokens"]) and ref["gap"] >= 8 * ref["tol"], (ref["gap"], ref["tol"])
    with pytest.raises(ValueError):
        models.build_unimernet(image_shape=(60, 96), ws=7, shifted=True)                           # 60 is no multiple of 8: the second stage could not merge
