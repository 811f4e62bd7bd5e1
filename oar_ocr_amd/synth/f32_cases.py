"""The f32 convolution kernels' case matrix: which compiled variant a layer runs on, restated in Python, and the float64 references and tolerances that
hold every variant to f32 accuracy -- the counterpart of x6_cases.py for the layers the bf16x6 rules do not take.

A case is one Conv or ConvTranspose node.  `plan(case)` restates the selection of the native code (engine.cc op_conv / op_convt: the kind; igemm.hip
igemm_weight_format and conv_igemm's branches; kernels.hip conv_dw / conv_direct) and returns the profiler name the layer must run under with
OAR_PROF_DETAIL=1 -- shape and variant -- so that tests/test_gpu_f32_conv_kernels.py fails when a threshold moves and this restatement does not.
`bundle` gives the float64 reference, S = the same operation on absolute values, and tol_S = 4 noise_S with noise_S the larger of two honest f32 evaluations
against float64 on the case's sample (in units of S): the in-order chain of x6_cases.f32_matmul on the im2col view, and torch's float32 convolution.

CPU only: numpy and torch."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from . import x6_cases
from .onnx_writer import GraphBuilder

F32 = np.float32
FAMILIES = ("normal", "positive")
KINDS = ("ws_1x1", "ws_1x1_nt43", "ws_1x1_nt21", "ws_gen", "ws_gen_nt43", "ws_gen_nt21", "ws3", "ws3_rs3off", "tile", "tile_pf4", "small", "dw", "direct")     # one child process per entry (tests/test_gpu_f32_conv_kernels.py)
KIND_ENV = {"ws3_rs3off": {"OAR_IGEMM_RS3": "0"}, "tile_pf4": {"OAR_IGEMM_PF": "4"}}                                        # switches a child needs on top of the default environment


@dataclass(frozen=True)
class Case:
    """One Conv (or ConvTranspose) on an [n, cin, h, w] input.  pads: top, left, bottom, right.  residual: 'same' = Add with a second graph input of the
    output's shape, 'up2' = Add with the nearest 2x upsampling of a half-resolution input (an FPN sum).  concat: the channels of a sibling convolution
    whose output is concatenated with this one's.  se: the convolution reads x times the squeeze-excite gate of x6_cases.se_gate.  gap: the (depthwise)
    convolution's output is pooled -- 'mean': the means are read by an identity 1x1 convolution and compared, 'gate': they feed a squeeze-excite gate.
    poison: the case also runs with three NaNs in its input (poison_at)."""
    name: str
    kind: str
    cin: int
    cout: int
    kh: int
    kw: int
    n: int
    h: int
    w: int
    strides: tuple = (1, 1)
    pads: tuple = (0, 0, 0, 0)
    dilations: tuple = (1, 1)
    group: int = 1
    bias: bool = True
    act: str = None
    residual: str = None
    concat: int = 0
    se: bool = False
    gap: str = None
    transpose: bool = False
    output_padding: tuple = (0, 0)
    poison: bool = False

    @property
    def out_hw(self):
        (sh, sw), (pt, pl, pb, pr), (dh, dw) = self.strides, self.pads, self.dilations
        if self.transpose:
            return ((self.h - 1) * sh - pt - pb + dh * (self.kh - 1) + self.output_padding[0] + 1,
                    (self.w - 1) * sw - pl - pr + dw * (self.kw - 1) + self.output_padding[1] + 1)
        return (self.h + pt + pb - dh * (self.kh - 1) - 1) // sh + 1, (self.w + pl + pr - dw * (self.kw - 1) - 1) // sw + 1

    @property
    def M(self):
        ho, wo = self.out_hw
        return self.n * ho * wo

    @property
    def w_shape(self):
        """the ONNX weight: Conv [cout, cin / group, kh, kw], ConvTranspose [cin, cout / group, kh, kw]"""
        return (self.cin, self.cout // self.group, self.kh, self.kw) if self.transpose else (self.cout, self.cin // self.group, self.kh, self.kw)


# ------------------------------------------------------------------------------------------------ the selection, restated (default environment + `env`)
def _ceil(a, b):
    return -(-a // b)


def _env_int(env, key, default):
    return int(env[key]) if key in env else default


def _os_x6_eligible(M, K, N, Cin, grouped=False):
    tiles = _ceil(M, 256) * _ceil(N, 128)
    fills = M >= 65536 or (M >= 8192 and tiles >= 256) or (grouped and M >= 4096) or (K >= 2048 and M >= 8192 and tiles >= 128)
    return Cin % 8 == 0 and K >= 256 and N >= (32 if grouped else 48) and N % 4 == 0 and fills and K < 65536


def _ws_x6_tile(K, nfrag):
    KC, best, nt = _ceil(K, 32), 1 << 30, 0
    for t in (8, 6, 4):
        if t * KC * 3072 > 150 * 1024:
            continue
        padded = _ceil(nfrag, t) * t
        if padded < best:
            best, nt = padded, t
    return nt


def _rs3_eligible(M, Cin, Cout, img_px, y_ld, env):
    return (_env_int(env, "OAR_IGEMM_RS3", 1) != 0 and Cin in (32, 64) and 4 <= Cout <= 16 and Cout % 4 == 0 and y_ld % 4 == 0 and M >= 100000 and
            img_px * Cin * 4 < (1 << 29) and M * y_ld * 4 < (1 << 31))


def _lk_candidate(c):
    """a layer the large-kernel bf16x6 rule (igemm_lk_x6.hip) could take: that rule is not restated, the matrix stays away from it"""
    return c.group == 1 and not c.transpose and ((c.kh == 9 and c.kw == 9) or (c.kh == 5 and c.kw == 5 and c.cin == 32)) and c.cin % 32 == 0


def weight_format(M, K, N, is1x1, Cin, same3x3_px, env):
    """igemm_weight_format: 'x6' or 'f32'"""
    if _env_int(env, "OAR_IGEMM_X6", 1) == 0:
        return "f32"
    if not is1x1 and same3x3_px > 0 and K == 9 * Cin and _rs3_eligible(M, Cin, N, same3x3_px, 4 * N, env):
        return "x6"
    if not is1x1:
        return "x6" if Cin > 0 and _os_x6_eligible(M, K, N, Cin) else "f32"
    nfrag = _ceil(N, 16)
    passes = _ceil(M, 16) * _ceil(nfrag, 8)
    if K % 8 == 0 and K >= 96 and N >= 96 and N % 4 == 0 and passes >= 4096 and _ws_x6_tile(K, nfrag) > 0:
        return "x6"
    return "x6" if _os_x6_eligible(M, K, N, K) else "f32"


def _best_nt(nfrag, cands):
    best, nt = 1 << 30, 0
    for t in cands:
        padded = _ceil(nfrag, t) * t
        if padded < best:
            best, nt = padded, t
    return nt


@dataclass(frozen=True)
class Plan:
    names: tuple       # the OAR_PROF_DETAIL names of the convolution's own launches (one, or one per slice / group)
    variant: str       # what conv_igemm / conv_dw append to the shape ('' for the direct kernels and the bf16x6 classes)
    inst: str          # the compiled instantiation, as tests/test_f32_cases_cpu.py lists them
    f32: bool          # runs on the f32 kernels this matrix is about


def _igemm(c, env, convt):
    ho, wo = c.out_hw
    (sh, sw), (pt, pl, pb, pr), (dh, dw) = c.strides, c.pads, c.dilations
    if convt:
        M, K, N = c.n * c.h * c.w, c.cin, 4 * c.cout
        is1x1, fmt = True, "f32"
    else:
        M, K, N = c.n * ho * wo, c.kh * c.kw * c.cin, c.cout
        is1x1 = c.kh == 1 and c.kw == 1 and sh == 1 and sw == 1 and pt == 0 and pl == 0
        same3x3 = c.kh == 3 and c.kw == 3 and (sh, sw, pt, pl, dh, dw) == (1, 1, 1, 1, 1, 1) and (ho, wo) == (c.h, c.w)
        assert not _lk_candidate(c), "the large-kernel rule is not restated"
        fmt = weight_format(M, K, N, is1x1, c.cin, c.h * c.w if same3x3 and not c.residual else 0, env)
    shape = f"M={M} K={K} N={N} k{c.kh}x{c.kw} s{sh}{' convT' if convt else ''}"
    nfrag = _ceil(N, 16)
    if fmt == "x6":
        same3x3 = not convt and c.kh == 3 and c.kw == 3 and (sh, sw, pt, pl, dh, dw) == (1, 1, 1, 1, 1, 1) and (ho, wo) == (c.h, c.w)
        if same3x3 and not c.residual and not c.se and _rs3_eligible(M, c.cin, c.cout, c.h * c.w, c.cout, env):
            cls = "_rs3_x6"
        else:
            tile = _ws_x6_tile(K, nfrag)
            prefer_os = is1x1 and not c.se and c.act in (None, "relu") and K >= 320 and N >= 512 and 0 < tile <= 4 and _os_x6_eligible(M, K, N, c.cin)
            cls = "_os_x6" if (not is1x1 or tile == 0 or prefer_os) else "_x6"
        return Plan((f"conv_igemm{cls} {shape}",), "", "x6:" + cls[1:], False)
    KC = _ceil(K, 16)
    NT = _best_nt(nfrag, (4, 3, 2, 1))
    ny = _ceil(nfrag, NT)
    pf_env = _env_int(env, "OAR_IGEMM_PF", 2)
    PF = pf_env if pf_env in (1, 4) else 2
    while PF > 1 and _ceil(M, 4 * PF * 16) * ny < 1024:
        PF >>= 1
    vec_ok = c.cout % 4 == 0     # (y_ld = Cout: no convolution is placed in a wider buffer by the planner)
    ws_auto = (N >= 96 and _ceil(M, 16) * _ceil(nfrag, 8) >= 4096) or (K >= 512 and M >= 262144)
    res_up = c.residual == "up2"
    ws_nt = 0
    if not res_up and vec_ok and KC >= 2 and ws_auto:
        ws_nt = _best_nt(nfrag, [t for t in (8, 6, 4, 3, 2, 1) if t * KC * 1024 <= 150 * 1024])
    ws3 = (not res_up and _env_int(env, "OAR_IGEMM_WS3", 1) != 0 and vec_ok and not convt and c.kh == 3 and c.kw == 3 and
           (sh, sw, dh, dw, pt, pl) == (1, 1, 1, 1, 1, 1) and (ho, wo) == (c.h, c.w) and c.cin % 16 == 0 and nfrag <= 2 and 100000 <= M < (1 << 31) and
           nfrag * KC * 1024 <= 150 * 1024)
    small = not ws3 and ws_nt == 0 and _ceil(M, 16) * ny <= 4096
    kk = "1x1" if is1x1 else "kxk"
    if ws3:
        var, inst = f"ws3 NT={nfrag}", f"ws3<{nfrag},2>"
    elif ws_nt:
        pf = 1 if ws_nt >= 6 else 2
        var, inst = f"ws NT={ws_nt} PF={pf}", f"ws_{'1x1' if is1x1 else 'gen'}<{ws_nt},{pf}>"
    elif small:
        gated = c.se and se_fused(c, env)
        var, inst = f"small{' SE' if gated else ''} NT={NT}", f"small<{NT},{'1x1 SE' if gated else kk}>"
    else:
        var, inst = f"tile NT={NT} PF={PF}", f"tile<{NT},{PF},{kk}>"
    return Plan((f"conv_igemm{'_ws' if ws3 or ws_nt else ''} {shape} {var}",), var, inst, True)


def se_fused(c, env=()):
    """op_conv + conv_igemm_se_ok on an f32 layer: the gate rides on the latency variant's loads (else a Mul runs first)"""
    env = dict(env)
    if not c.se or c.transpose or c.group != 1 or (c.kh, c.kw, c.strides, c.pads) != (1, 1, (1, 1), (0, 0, 0, 0)) or c.residual or c.cin % 8:
        return False
    M, K, N = c.M, c.cin, c.cout
    if weight_format(M, K, N, True, K, 0, env) != "f32" or K % 4 or N % 4:
        return False
    nfrag, KC = _ceil(N, 16), _ceil(K, 16)
    NT = _best_nt(nfrag, (4, 3, 2, 1))
    ws_auto = (N >= 96 and _ceil(M, 16) * _ceil(nfrag, 8) >= 4096) or (K >= 512 and M >= 262144)
    return not (KC >= 2 and ws_auto) and _ceil(M, 16) * _ceil(nfrag, NT) <= 4096


def plan(c, env=()):
    """-> Plan of the case's convolution under the default environment plus `env`"""
    env = dict(env)
    ho, wo = c.out_hw
    (sh, sw), (pt, pl, pb, pr), (dh, dw) = c.strides, c.pads, c.dilations
    px = c.n * ho * wo
    if c.transpose:
        fast = (c.kh, c.kw, sh, sw) == (2, 2, 2, 2) and c.pads == (0, 0, 0, 0) and c.output_padding == (0, 0) and c.cin % 4 == 0 and (dh, dw) == (1, 1)
        if fast:
            return _igemm(c, env, True)
        return Plan((f"convt_direct px={px} Cin={c.cin} Cout={c.cout} k{c.kh}x{c.kw} s{sh}x{sw}",), "", "convt_direct", True)
    g, cg, og = c.group, c.cin // c.group, c.cout // c.group
    if 1 < g < c.cin and cg % 8 == 0 and og % 4 == 0 and not c.se and c.residual != "up2" and env.get("OAR_GROUPED_X6") != "0" and _os_x6_eligible(px, c.kh * c.kw * cg, og, cg, True):
        return Plan((f"conv_igemm_os_x6 M={px} K={c.kh * c.kw * cg} N={og} k{c.kh}x{c.kw} s{sh}",), "", "x6:os_x6 grouped", False)
    same3x3 = c.kh == 3 and c.kw == 3 and (sh, sw, pt, pl, dh, dw) == (1, 1, 1, 1, 1, 1) and (ho, wo) == (c.h, c.w)
    if (g == 1 and c.cout <= 16 and 64 < c.cin <= 256 and c.cin % 32 == 0 and same3x3 and not c.residual and not c.se and c.h * c.w * c.cin * 4 < (1 << 29) and
            _rs3_eligible(px, 64, c.cout, c.h * c.w, 4 * c.cout, env)):
        widths = [min(64, c.cin - c0) for c0 in range(0, c.cin, 64)]
        return Plan(tuple(f"conv_igemm_rs3_x6 M={px} K={9 * cs} N={c.cout} k3x3 s1" for cs in widths), "", "x6:rs3_x6 slices", False)
    if g == 1 and c.cin % 4 == 0:
        return _igemm(c, env, False)
    if g == c.cin and g == c.cout and c.cout % 4 == 0:
        tiled = c.kh == c.kw and (dh, dw) == (1, 1) and c.kh in (3, 5) and sh in (1, 2) and sw in (1, 2) and c.kh * c.kw * c.cout * 4 <= 96 * 1024
        if not tiled:
            return Plan((f"conv_dw px={px} C={c.cout} k{c.kh} s{sh} generic",), "generic", "dw_generic", True)
        th = 2 if c.n * _ceil(ho, 2) * _ceil(wo, 4) * (c.cout // 4) >= 256 * 256 * 4 else 1
        gap = bool(c.gap) and c.kh == 5 and c.cout >= 8 and c.cout <= 1024 and not c.residual
        lds96 = c.kh * c.kw * c.cout * 4 > 64 * 1024
        var = f"tiled k={c.kh} s={sh}x{sw} TH={th}{' gap' if gap else ''}{' lds96' if lds96 else ''}"
        return Plan((f"conv_dw px={px} C={c.cout} k{c.kh} s{sh} {var}",), var, f"dw_tiled<{c.kh},{sh},{sw},{th}{',gap' if gap else ''}>{' lds96' if lds96 else ''}", True)
    cls = "conv_smallcin" if g == 1 and c.cin <= 4 and c.kh * c.kw * c.cin <= 128 else "conv_direct"
    return Plan((f"{cls} px={px} Cin={c.cin} Cout={c.cout} g{g} k{c.kh}x{c.kw} s{sh}x{sw}",), "", cls[5:], True)


def expected_variant(c, env=()):
    """the variant string the native code appends to the layer's detail name ('' where the kernel has one form)"""
    return plan(c, env).variant


def ws_tiles_per_wave(c):
    """weight-stationary layers: wave tiles per wave of the busiest workgroup (launch_igemm_ws: 32 workgroups x 16 waves per XCD band, split into
    min(ny, 32) teams) -- a wave crosses a tile boundary when this exceeds 1, twice when it exceeds 2"""
    p = plan(c)
    assert p.inst.startswith("ws_"), p.inst
    nt, pf = (int(v) for v in p.inst[p.inst.index("<") + 1:-1].split(","))
    ny = _ceil(_ceil(c.cout, 16), nt)
    groups = min(ny, 32)
    team = _ceil(32, groups)
    per_xcd = _ceil(_ceil(c.M, 16 * pf), 8)
    return _ceil(per_xcd, team) / 16.0


# ------------------------------------------------------------------------------------------------ inputs
def case_inputs(c, family, seed=0):
    """-> dict(x, w, b, r): x6_cases.family_inputs' draws (b None without a bias); w in the ONNX layout of the node; r the residual operand or None"""
    x, w, b = x6_cases.family_inputs(family, (c.n, c.cin, c.h, c.w), (c.cout, c.cin // c.group, c.kh, c.kw), seed)
    if c.transpose:     # [cout, cin / g, kh, kw] -> [cin, cout / g, kh, kw]
        g, cg, og = c.group, c.cin // c.group, c.cout // c.group
        w = np.ascontiguousarray(w.reshape(g, og, cg, c.kh, c.kw).transpose(0, 2, 1, 3, 4).reshape(c.cin, og, c.kh, c.kw))
    r = None
    if c.residual:
        ho, wo = c.out_hw
        f = 2 if c.residual == "up2" else 1
        rng = np.random.default_rng([seed, c.n, c.cout, ho, wo, FAMILIES.index(family), 7])
        r = (rng.standard_normal((c.n, c.cout, ho // f, wo // f)) if family == "normal" else rng.uniform(1, 2, (c.n, c.cout, ho // f, wo // f))).astype(F32)
    return dict(x=x, w=w, b=b if c.bias else None, r=r)


def poison_at(c):
    """-> three (image, channel, row, column): the image corner; the input pixel under the last output pixel (the last, partial pixel fragment); a pixel
    in the middle of the last image, last channel (the channel quad that the zero-padded K tail of the last chunk reads again)"""
    ho, wo = c.out_hw
    (sh, sw), (pt, pl, _, _) = c.strides, c.pads
    if c.transpose:
        last = (c.h - 1, c.w - 1)
    else:
        last = (min(c.h - 1, max(0, (ho - 1) * sh - pt + (c.kh // 2) * c.dilations[0])), min(c.w - 1, max(0, (wo - 1) * sw - pl + (c.kw // 2) * c.dilations[1])))
    return (0, 0, 0, 0), (c.n - 1, c.cin // 2, *last), (c.n - 1, c.cin - 1, c.h // 2, c.w // 2)


def poisoned(c, x):
    x = x.copy()
    for at in poison_at(c):
        x[at] = np.nan
    return x


# ------------------------------------------------------------------------------------------------ references
def _res_full(c, r):
    if r is None:
        return None
    return r.repeat(2, axis=2).repeat(2, axis=3) if c.residual == "up2" else r


def gated(c, x):
    return x * x6_cases.se_gate(c)[4][None, :, None, None] if c.se else x


def conv_ref(c, x, w, b, dtype="float64", r=None, edit=None):
    """The node in `dtype` with torch (conv2d / conv_transpose2d; the pads applied with an explicit F.pad), plus the residual; no activation.
    edit 'clamp': the padding replicates the edge pixel instead of reading zero (Conv only); 'bias': the bias is left out of the channels past the first
    16 -- two of the wrong references of tests/test_f32_cases_cpu.py."""
    import torch
    import torch.nn.functional as Fn
    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    xt, wt = torch.from_numpy(np.ascontiguousarray(gated(c, x))).to(dt), torch.from_numpy(np.ascontiguousarray(w)).to(dt)
    bt = None
    if b is not None:
        bt = torch.from_numpy(np.ascontiguousarray(b)).to(dt).clone()
        if edit == "bias":
            bt[16:] = 0
    pt, pl, pb, pr = c.pads
    with torch.no_grad():
        if c.transpose:
            y = Fn.conv_transpose2d(xt, wt, bt, stride=c.strides, padding=0, output_padding=c.output_padding, groups=c.group, dilation=c.dilations)
            y = y[:, :, pt:y.shape[2] - pb, pl:y.shape[3] - pr]
        else:
            if pt or pl or pb or pr:
                xt = Fn.pad(xt, (pl, pr, pt, pb), mode="replicate") if edit == "clamp" else Fn.pad(xt, (pl, pr, pt, pb))
            y = Fn.conv2d(xt, wt, bt, stride=c.strides, padding=0, dilation=c.dilations, groups=c.group)
        if r is not None:
            y = y + torch.from_numpy(np.ascontiguousarray(_res_full(c, r))).to(dt)
    out = y.contiguous().numpy()
    assert out.shape == (c.n, c.cout, *c.out_hw), (out.shape, c)
    return out


def act_ref(a, kind):
    return x6_cases.act_ref(a, kind)


def sample_rows(c, rows=256):
    return np.unique(np.linspace(0, c.M - 1, rows).astype(np.int64))


def gemm_view(c, x, w, rows, cols=64):
    """-> T [P, taps, cin] f32 (the input pixel under every tap of the output pixels `rows`, zero where the tap reads padding), wsel(tap, ci) -> the
    weights [ncols] and chan(ci) -> the input channel [ncols] of the first `cols` output channels: k = (tap row, tap column, channel) as the kernels walk it"""
    ho, wo = c.out_hw
    (sh, sw), (pt, pl, _, _), (dh, dw) = c.strides, c.pads, c.dilations
    img, rr = np.divmod(np.asarray(rows), ho * wo)
    oy, ox = np.divmod(rr, wo)
    xl = np.ascontiguousarray(np.asarray(gated(c, x), F32).transpose(0, 2, 3, 1))
    T = np.zeros((len(rows), c.kh * c.kw, c.cin), F32)
    for i in range(c.kh):
        for j in range(c.kw):
            if c.transpose:
                ny_, nx_ = oy + pt - i * dh, ox + pl - j * dw
                ok = (ny_ % sh == 0) & (nx_ % sw == 0)
                iy, ix = ny_ // sh, nx_ // sw
            else:
                iy, ix = oy * sh - pt + i * dh, ox * sw - pl + j * dw
                ok = np.ones(len(rows), bool)
            ok &= (iy >= 0) & (iy < c.h) & (ix >= 0) & (ix < c.w)
            T[ok, i * c.kw + j] = xl[img[ok], iy[ok], ix[ok]]
    ncols = min(cols, c.cout)
    co = np.arange(ncols)
    cg, og = c.cin // c.group, c.cout // c.group
    chan = lambda ci: (co // og) * cg + ci
    if c.transpose:
        wsel = lambda tap, ci: np.asarray(w, F32)[chan(ci), co % og, tap // c.kw, tap % c.kw]
    else:
        wsel = lambda tap, ci: np.asarray(w, F32)[co, ci, tap // c.kw, tap % c.kw]
    return T, wsel, chan, co


def f32_chain(c, x, w, b, r, rows, cols=64):
    """the plain f32 evaluation of the sample: bias first, then k ascending, one rounding per multiplication and per addition, the residual last.
    group 1: x6_cases.f32_matmul on the im2col view itself; grouped: the same chain with every output channel's own input channels."""
    T, wsel, chan, co = gemm_view(c, x, w, rows, cols)
    bias = np.zeros(len(co), F32) if b is None else np.asarray(b, F32)[co]
    cg = c.cin // c.group
    if c.group == 1:
        Wm = np.stack([wsel(tap, ci) for tap in range(c.kh * c.kw) for ci in range(cg)])
        acc = x6_cases.f32_matmul(T.reshape(len(rows), -1), Wm, bias)
    else:
        acc = np.broadcast_to(bias, (len(rows), len(co))).copy()
        for tap in range(c.kh * c.kw):
            for ci in range(cg):
                acc += T[:, tap, chan(ci)] * wsel(tap, ci)[None, :]
    if r is not None:
        acc = acc + pick(c, _res_full(c, r), rows, co)
    return acc, co


def pick(c, full, rows, co):
    """[n, cout, ho, wo] -> [len(rows), len(co)]"""
    ho, wo = c.out_hw
    return np.ascontiguousarray(full.transpose(0, 2, 3, 1)).reshape(c.n * ho * wo, c.cout)[np.asarray(rows)][:, co]


def bundle(c, x, w, b, r=None):
    """-> dict(f64, S, noise_S, tol_S, y32): f64 and S = the operation on |x|, |w|, |b| (+ |r|) as [n, cout, ho, wo], no activation; noise_S the larger of the
    f32 chain's and torch float32's error against f64 on the sample, in units of S; tol_S = 4 noise_S (DESIGN 4.38's factor for a third summation order)."""
    absb = None if b is None else np.abs(b)
    f64 = conv_ref(c, x, w, b, "float64", r)
    S = conv_ref(c, np.abs(x), np.abs(w), absb, "float64", None if r is None else np.abs(r))
    y32 = conv_ref(c, x, w, b, "float32", r)
    rows = sample_rows(c)
    chain, co = f32_chain(c, x, w, b, r, rows)
    f, s = pick(c, f64, rows, co), pick(c, S, rows, co)
    s = np.where(s > 0, s, 1.0)     # (an output that adds nothing but zeros: both evaluations give 0 exactly)
    n_chain = float((np.abs(chain.astype(np.float64) - f) / s).max())
    n_torch = float((np.abs(pick(c, y32, rows, co).astype(np.float64) - f) / s).max())
    noise = max(n_chain, n_torch)
    return dict(f64=f64, S=S, noise_S=noise, tol_S=4.0 * noise, noise_chain=n_chain, noise_torch=n_torch)


def err_S(got, f64, S):
    """max |got - f64| / S over the whole output (S = 0: an output of nothing but zero terms must be exactly 0)"""
    d = np.abs(np.asarray(got, np.float64) - f64)
    z = S == 0
    assert not (z & (d != 0)).any(), "a non-zero output where every term is zero"
    return float((d[~z] / S[~z]).max()) if (~z).any() else 0.0


def reduced(c, h=11, w=13):
    """the case on at most two small images (the CPU test's wrong edits): same node, h x w input or as small as the kernel allows"""
    need_h = c.dilations[0] * (c.kh - 1) + 1
    need_w = c.dilations[1] * (c.kw - 1) + 1
    return replace(c, n=min(c.n, 2), h=min(c.h, max(h, need_h)), w=min(c.w, max(w, need_w)), residual=("same" if c.residual else None))


# ------------------------------------------------------------------------------------------------ graphs
def _conv_attrs(c):
    return dict(kernel_shape=[c.kh, c.kw], strides=list(c.strides), pads=list(c.pads), group=c.group, dilations=list(c.dilations))


def _se_src(g, c, src):
    """GlobalAveragePool -> Conv + Relu -> Conv + HardSigmoid -> Mul with x6_cases.se_gate's weights: the gate is 1, 0.5 or 0.25 by channel whatever x is"""
    w1, b1, w2, b2, _ = x6_cases.se_gate(c)
    one = dict(kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
    h = g.op("Relu", [g.op("Conv", [g.op("GlobalAveragePool", [src]), g.init(w1), g.init(b1)], **one)])
    return g.op("Mul", [src, g.op("HardSigmoid", [g.op("Conv", [h, g.init(w2), g.init(b2)], **one)], alpha=x6_cases.SE_ALPHA, beta=x6_cases.SE_BETA)])


def _node(g, c, w, b, src="x"):
    ins = [src, g.init(w)] + ([g.init(b)] if b is not None else [])
    if c.transpose:
        return g.op("ConvTranspose", ins, output_padding=list(c.output_padding), **_conv_attrs(c))
    return g.op("Conv", ins, **_conv_attrs(c))


def model(c, w, b, act="case", sibling=None):
    """The one-layer graph.  act: 'case' = the case's activation, None = none (a HardSwish layer compared in front of its activation).
    sibling: (case, w, b, first) -- the graph's output is Concat of this convolution and the sibling's, the sibling first if `first`.
    Inputs: x, and r for a residual.  Outputs: the layer; for gap cases the layer and the pooled branch ('mean': [n, c, 1, 1] means, 'gate': layer x gate)."""
    act = c.act if act == "case" else act
    ho, wo = c.out_hw
    g = GraphBuilder("f32")
    g.add_input("x", [c.n, c.cin, c.h, c.w])
    src = _se_src(g, c, "x") if c.se else "x"
    y = _node(g, c, w, b, src)
    if c.residual:
        f = 2 if c.residual == "up2" else 1
        g.add_input("r", [c.n, c.cout, ho // f, wo // f])
        other = "r"
        if f == 2:     # (the identity pool makes the operand channels-last, as the deferred Resize asks)
            t = g.op("AveragePool", ["r"], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0])
            other = g.op("Resize", [t, "", g.init(np.array([1, 1, 2, 2], F32), "scales")], mode="nearest", coordinate_transformation_mode="asymmetric", nearest_mode="floor")
        y = g.op("Add", [y, other])
    if act == "relu":
        y = g.op("Relu", [y])
    elif act == "hswish":
        y = g.op("HardSwish", [y])
    if sibling is not None:
        sc, sw_, sb, first = sibling
        z = _node(g, sc, sw_, sb)
        y = g.op("Concat", [z, y] if first else [y, z], axis=1)
        g.add_output(y, [c.n, c.cout + sc.cout, ho, wo])
        return g.model()
    g.add_output(y, [c.n, c.cout, ho, wo])
    if c.gap == "mean":
        eye = np.eye(c.cout, dtype=F32).reshape(c.cout, c.cout, 1, 1)
        q = g.op("Conv", [g.op("GlobalAveragePool", [y]), g.init(eye)], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
        g.add_output(q, [c.n, c.cout, 1, 1])
    elif c.gap == "gate":
        g.add_output(_se_src(g, replace(c, cin=c.cout), y), [c.n, c.cout, ho, wo])
    return g.model()


def sibling_of(c):
    """the convolution a `concat` case shares its Concat with: the same node with `concat` output channels"""
    return replace(c, name=c.name + " sibling", cout=c.concat, concat=0, poison=False)


# ------------------------------------------------------------------------------------------------ the matrix
def _p(k, d=1):
    return d * (k // 2)


def _c1(name, kind, cin, cout, n, h, w, **kw):
    return Case(name, kind, cin, cout, 1, 1, n, h, w, **kw)


def _c3(name, kind, cin, cout, n, h, w, k=3, **kw):
    kw.setdefault("pads", (_p(k),) * 4)
    return Case(name, kind, cin, cout, k, k, n, h, w, **kw)


def _dw(name, c, k, s, n, h, w, **kw):
    kw.setdefault("pads", (_p(k),) * 4)
    return Case(name, "dw", c, c, k, k, n, h, w, strides=s, group=c, **kw)


_SMALL_M = {1: (1, 1, 1), 15: (1, 3, 5), 17: (1, 1, 17), 63: (1, 7, 9), 65: (1, 5, 13)}


def _small_grid():
    out = []
    ms = list(_SMALL_M)
    k1 = {1: 8, 2: 24, 3: 48, 4: 64, 5: 76, 7: 112}                                   # 1x1: KC -> Cin (K = Cin; 24 and 76: a K tail)
    kk = {1: (1, 3, 4), 2: (1, 3, 8), 3: (3, 3, 4), 4: (1, 3, 20), 5: (3, 3, 8), 7: (3, 3, 12)}     # k x k: KC -> (kh, kw, Cin)
    i = 0
    for nt, cout in ((1, 16), (2, 32), (3, 44), (4, 64)):
        for kc in (1, 2, 3, 4, 5, 7):
            n, h, w = _SMALL_M[ms[i % 5]]
            out.append(_c1(f"small 1x1 NT{nt} KC{kc} M{ms[i % 5]}", "small", k1[kc], cout, n, h, w, act="relu" if i % 2 else None, bias=i % 3 != 0))
            i += 1
            n, h, w = _SMALL_M[ms[i % 5]]
            kh, kw, cin = kk[kc]
            out.append(Case(f"small {kh}x{kw} NT{nt} KC{kc} M{ms[i % 5]}", "small", cin, cout, kh, kw, n, h, w, pads=(_p(kh), _p(kw), _p(kh), _p(kw)),
                            act="relu" if i % 2 else None, bias=i % 3 != 0))
            i += 1
    return out


_WS_SHAPES = ((8, 128, (1, 443, 445)), (6, 96, (1, 443, 445)), (4, 320, (3, 171, 169)), (3, 144, (2, 261, 263)), (2, 160, (3, 171, 169)), (1, 112, (1, 255, 259)))
_WS_GEN_SHAPES = ((8, 128, (3, 257, 259)), (6, 96, (3, 257, 259)), (4, 320, (3, 171, 169)), (3, 144, (2, 261, 263)), (2, 160, (3, 171, 169)), (1, 112, (3, 149, 151)))


def _ws_kind(base, nt):
    return base + ("" if nt >= 6 else "_nt43" if nt >= 3 else "_nt21")     # (three children per kernel, by NT: bounds what one child leaves on disk)


def _ws_1x1_grid():
    """all six (NT, PF) x K = 32, 48, 64 (KC % 3 = 2, 0, 1: the stage rotation at a tile boundary), 40 (zero-padded tail of the last chunk), 80 (KC = 5), every
    one at an M where each wave of the busiest workgroup pulls three wave tiles"""
    out, i = [], 0
    for nt, cout, px in _WS_SHAPES:
        for k in (32, 48, 64, 40, 80):
            opts = dict(act=(None, "relu", None, "hswish", None)[i % 5], bias=i % 7 != 3, poison=i % 6 == 0)
            out.append(_c1(f"ws_1x1 NT{nt} K{k}", _ws_kind("ws_1x1", nt), k, cout, *px, **opts))
            i += 1
    return out


def _ws_gen_grid():
    """all six (NT, PF) x {3x3 Cin 4: K = 36, KC % 3 = 0, a K tail; 1x3 Cin 20: K = 60, KC % 3 = 1, a tail; 3x3 Cin 8: K = 72, KC % 3 = 2}, three tiles per wave,
    several images whose pixel count is no multiple of 16"""
    out, i = [], 0
    for nt, cout, px in _WS_GEN_SHAPES:
        for kh, kw, cin in ((3, 3, 4), (1, 3, 20), (3, 3, 8)):
            opts = dict(act=(None, "relu", None, "hswish")[i % 4], bias=i % 5 != 2, poison=i % 6 == 0)
            out.append(Case(f"ws_gen NT{nt} {kh}x{kw} {cin}->{cout}", _ws_kind("ws_gen", nt), cin, cout, kh, kw, *px, pads=(_p(kh), _p(kw), _p(kh), _p(kw)), **opts))
            i += 1
    return out


def _tile_grid(kind, pfs):
    """NT = 1 .. 4 x {1x1, 3x3} x PF: 66045 pixels stay under the 1024 workgroups PF = 2 asks for, 133126 do not, 266252 reach PF = 4's"""
    px = {1: (1, 255, 259), 2: (2, 257, 259), 4: (4, 257, 259)}
    out, i = [], 0
    for nt, cout in ((1, 16), (2, 32), (3, 48), (4, 64)):
        for pf in pfs:
            cin = (8, 24, 16, 20)[(nt + pf) % 4]     # K = 8 and 16: KC = 1; 24 and 20: a K tail
            out.append(_c1(f"{kind} 1x1 NT{nt} PF{pf} K{cin}", kind, cin, cout, *px[pf], act=(None, "relu", "hswish")[i % 3], bias=i % 4 != 3, poison=i % 4 == 0))
            i += 1
            cin = (4, 8)[(nt + pf) % 2]
            out.append(_c3(f"{kind} 3x3 NT{nt} PF{pf} {cin}->{cout}", kind, cin, cout, *px[pf], act=(None, "relu", "hswish")[i % 3], bias=i % 4 != 3, poison=i % 4 == 0))
            i += 1
    return out


CASES = (
    # ---- conv_igemm_ws_kernel<NT, PF, true>: 1x1, N >= 96, K < 96 (K >= 96 is a bf16x6 layer), >= 4096 (16-pixel, 128-cout) passes.  The six (NT, PF) by the
    # padded-fragment rule: N = 128, 96, 320, 144, 160, 112.  M: >= 3 wave tiles per wave of the busiest workgroup (ws_tiles_per_wave), no multiple of 16 PF
    *_ws_1x1_grid(),
    _c1("ws_1x1 NT1 K32 residual", "ws_1x1_nt21", 32, 112, 1, 255, 259, residual="same"),
    _c1("ws_1x1 NT1 K48 concat", "ws_1x1_nt21", 48, 112, 1, 255, 259, concat=8),
    _c1("ws_1x1 NT4 K32 fewest pixels", "ws_1x1_nt43", 32, 320, 1, 149, 147),                   # 21903 pixels: 86 wave tiles per XCD band over 7 workgroups of 16 waves -- some waves get none
    # ---- conv_igemm_ws_kernel<NT, PF, false>: k x k with Cin 4 and 8 (K = 36 with a tail, K = 72; K < 256 and Cin % 16 != 0: neither bf16x6 nor ws3)
    *_ws_gen_grid(),
    Case("ws_gen NT1 1x3 8->112", "ws_gen_nt21", 8, 112, 1, 3, 3, 149, 151, pads=(0, 1, 0, 1)),
    Case("ws_gen NT1 3x1 8->112", "ws_gen_nt21", 8, 112, 3, 1, 3, 149, 151, pads=(1, 0, 1, 0)),                       # kw = 1: kw_one
    _c3("ws_gen NT1 3x3 s2 8->112", "ws_gen_nt21", 8, 112, 3, 297, 301, strides=(2, 2)),
    _c3("ws_gen NT1 3x3 s(2,1) 4->112", "ws_gen_nt21", 4, 112, 3, 297, 151, strides=(2, 1)),
    _c3("ws_gen NT1 3x3 d2 8->112", "ws_gen_nt21", 8, 112, 3, 149, 151, dilations=(2, 2), pads=(2, 2, 2, 2)),
    _c3("ws_gen NT1 3x3 pads(0,1,2,1) 4->112", "ws_gen_nt21", 4, 112, 3, 149, 151, pads=(0, 1, 2, 1)),
    _c3("ws_gen NT1 3x3 8->112 residual", "ws_gen_nt21", 8, 112, 3, 149, 151, residual="same"),
    # ---- conv_igemm_ws3_kernel<NT, 2>: 3x3 same, Cin % 16, Cout <= 32, M >= 100000.  Cin 32 / 64 with Cout <= 16 is a row-streaming bf16x6 layer by default:
    # Cin 16 (and Cout 32) stay f32; 32 -> 16 reaches this kernel only with OAR_IGEMM_RS3=0 (its own child)
    _c3("ws3 NT1 16->16", "ws3", 16, 16, 1, 317, 317, poison=True),
    _c3("ws3 NT2 16->32 relu", "ws3", 16, 32, 1, 317, 317, act="relu"),
    _c3("ws3 NT2 32->32 ragged", "ws3", 32, 32, 3, 150, 231, poison=True),
    _c3("ws3 NT2 48->20 hswish", "ws3", 48, 20, 1, 317, 317, act="hswish"),                # KC = 27, half of the second fragment idle
    _c3("ws3 NT1 32->16 (rs3 off)", "ws3_rs3off", 32, 16, 1, 317, 317),
    _c3("ws3 NT1 64->8 (rs3 off) relu", "ws3_rs3off", 64, 8, 3, 150, 231, act="relu"),
    # ---- conv_igemm_kernel<NT, PF, 1x1 | k x k>: more than 4096 wave tiles on layers the ws rule refuses (N < 96, or KC = 1); PF = 2 from 1024 workgroups
    *_tile_grid("tile", (1, 2)),
    _c1("tile 1x1 NT1 ny5 K8 wide", "tile", 8, 80, 1, 255, 259),                            # KC = 1 keeps an N >= 96-class layer off ws too: N = 80, five cout tiles
    _c1("tile 1x1 NT2 Cout30 scalar stores", "tile", 16, 30, 1, 255, 259, poison=True),
    _c1("tile 1x1 NT2 residual", "tile", 16, 32, 1, 255, 259, residual="same"),
    _c1("tile 1x1 NT2 upsampled residual", "tile", 16, 32, 2, 182, 186, residual="up2"),
    _c3("tile 5x5 s2 NT2 4->24", "tile", 4, 24, 1, 509, 517, k=5, strides=(2, 2)),
    Case("tile convT 2x2 8->3", "tile", 8, 3, 2, 2, 1, 257, 259, strides=(2, 2), transpose=True),                  # gemm N = 12: scalar scatter
    Case("tile convT 2x2 16->8 relu", "tile", 16, 8, 2, 2, 1, 257, 259, strides=(2, 2), transpose=True, act="relu", poison=True),
    # ---- conv_igemm_kernel<NT, 4, .> ships and no default path selects it: a child with OAR_IGEMM_PF=4, at the 1024 workgroups of 256 pixels PF = 4 asks for
    *_tile_grid("tile_pf4", (4,)),
    # ---- conv_igemm_small_kernel: at most 4096 wave tiles
    *_small_grid(),
    _c3("small 3x3 NT4 two blocks", "small", 8, 64, 1, 9, 15, poison=True),                  # M = 135: three 64-pixel workgroups
    _c1("small 1x1 NT4 64 blocks", "small", 32, 64, 1, 61, 67, poison=True),                 # 4087 pixels
    _c1("small 1x1 NT1 65511 pixels", "small", 16, 16, 1, 251, 261, act="relu"),             # 4095 wave tiles: the upper end of the rule (4096)
    _c1("small 1x1 SE 48->64", "small", 48, 64, 2, 9, 13, se=True),
    _c1("small 1x1 SE 24->20 relu", "small", 24, 20, 3, 5, 7, se=True, act="relu"),
    _c1("small 1x1 SE 24->16", "small", 24, 16, 2, 5, 7, se=True),
    _c1("small 1x1 SE 40->44", "small", 40, 44, 2, 5, 7, se=True),
    _c1("small 1x1 residual", "small", 24, 32, 1, 7, 9, residual="same"),
    _c3("small 3x3 residual", "small", 8, 48, 2, 7, 9, residual="same"),
    Case("small convT 2x2 4->8", "small", 4, 8, 2, 2, 2, 5, 7, strides=(2, 2), transpose=True),
    _c1("small 1x1 hswish", "small", 24, 32, 2, 7, 9, act="hswish"),
    _c3("small 3x3 hswish", "small", 8, 44, 1, 9, 15, act="hswish"),
    _c1("small 1x1 Cin4 stem", "small", 4, 16, 1, 9, 11),                                    # Cin = 4 is an implicit-GEMM layer (Cin % 4 == 0), not a conv_smallcin one
    # ---- depthwise: conv_dw_tiled_kernel<K, SH, SW, 4, TH, GAP> and the generic kernel
    _dw("dw 3x3 s1x1 TH1", 48, 3, (1, 1), 2, 19, 23, act="relu", poison=True),
    _dw("dw 3x3 s2x2 TH1", 24, 3, (2, 2), 1, 37, 41),
    _dw("dw 3x3 s2x1 TH1", 16, 3, (2, 1), 2, 21, 19),
    _dw("dw 3x3 s1x2 TH1", 16, 3, (1, 2), 2, 21, 19, act="hswish"),
    _dw("dw 5x5 s1x1 TH1", 32, 5, (1, 1), 1, 20, 21, poison=True),
    _dw("dw 5x5 s2x2 TH1", 24, 5, (2, 2), 1, 37, 51, act="relu"),
    _dw("dw 5x5 s2x1 TH1", 16, 5, (2, 1), 2, 13, 39),
    _dw("dw 5x5 s1x2 TH1", 16, 5, (1, 2), 2, 13, 39),
    _dw("dw 3x3 s1x1 TH2", 64, 3, (1, 1), 2, 181, 363, poison=True),                         # 2 x 91 x 91 x 16 = 264992 threads of two rows: odd Ho, Wo % 4 = 3
    _dw("dw 3x3 s1x1 TH2 C772", 772, 3, (1, 1), 1, 75, 143),                                 # 193 float4 lanes: 38 x 36 x 193 = 264024 threads
    _dw("dw 5x5 s1x2 TH2", 64, 5, (1, 2), 2, 181, 725, act="relu"),
    _dw("dw 5x5 s2x1 TH2", 64, 5, (2, 1), 2, 361, 363),
    _dw("dw 5x5 s1x1 TH2", 64, 5, (1, 1), 2, 181, 363),
    _dw("dw 3x3 s1x2 TH2", 64, 3, (1, 2), 2, 181, 725),
    _dw("dw 3x3 s2x1 TH2", 64, 3, (2, 1), 2, 361, 363, act="relu"),
    _dw("dw 3x3 C4", 4, 3, (1, 1), 1, 3, 5),                                                 # one float4 lane; 15 outputs: seven of eight XCD bands empty
    _dw("dw 5x5 C768 lds96", 768, 5, (1, 1), 1, 9, 13, act="hswish"),                        # 77 KB of weights
    _dw("dw 3x3 pads(0,1,2,1)", 16, 3, (1, 1), 2, 11, 13, pads=(0, 1, 2, 1)),
    _dw("dw 5x5 s1x1 gap mean", 16, 5, (1, 1), 3, 7, 21, gap="mean", act="relu"),
    _dw("dw 5x5 s2x2 gap mean", 24, 5, (2, 2), 2, 37, 51, gap="mean"),
    _dw("dw 5x5 s2x1 gap mean", 16, 5, (2, 1), 2, 13, 39, gap="mean"),
    _dw("dw 5x5 s1x2 gap mean", 16, 5, (1, 2), 2, 13, 39, gap="mean"),
    _dw("dw 5x5 s1x1 gap gate", 48, 5, (1, 1), 2, 6, 40, gap="gate", act="relu"),
    _dw("dw 5x5 s2x1 gap gate TH2", 192, 5, (2, 1), 6, 91, 160, gap="gate"),                 # 6 x 23 x 40 x 48 = 264960 threads
    _dw("dw 5x5 s1x1 gap mean TH2", 64, 5, (1, 1), 2, 181, 363, gap="mean"),
    _dw("dw 5x5 s1x2 gap gate TH2", 192, 5, (1, 2), 6, 46, 319, gap="gate", act="relu"),
    _dw("dw 7x7 generic", 16, 7, (1, 1), 2, 13, 17, poison=True),
    _dw("dw 3x3 d2 generic", 16, 3, (1, 1), 2, 13, 17, dilations=(2, 2), pads=(2, 2, 2, 2)),
    _dw("dw 3x3 s3 generic", 16, 3, (3, 3), 2, 19, 23),
    Case("dw 1x5 generic", "dw", 24, 24, 1, 5, 2, 9, 17, group=24, pads=(0, 2, 0, 2), act="relu"),
    _dw("dw 7x7 pads(3,2,1,0) generic", 8, 7, (1, 1), 1, 13, 17, pads=(3, 2, 1, 0)),
    # ---- the direct kernels
    _c3("smallcin 1->16 3x3", "direct", 1, 16, 2, 17, 19, poison=True),
    _c3("smallcin 2->24 7x7 s2", "direct", 2, 24, 2, 37, 41, k=7, strides=(2, 2), act="relu"),      # partial group of 16; K = 98
    _c3("direct 3->24 7x7 s2", "direct", 3, 24, 1, 37, 41, k=7, strides=(2, 2)),                    # K = 147 > 128: the stem no longer fits conv_smallcin's LDS slice
    _c3("smallcin 3->6 3x3", "direct", 3, 6, 2, 17, 19, act="hswish"),                              # y_ld % 4 != 0: scalar stores
    _c3("smallcin 2->16 5x5 no bias", "direct", 2, 16, 1, 17, 19, k=5, bias=False),
    _c3("smallcin 3->16 residual", "direct", 3, 16, 1, 17, 19, residual="same"),
    _c3("direct 6->7", "direct", 6, 7, 2, 13, 17, poison=True),
    _c3("direct 6->9 g3 relu", "direct", 6, 9, 2, 13, 17, group=3, act="relu"),
    _c3("direct 6->10 g2 s2", "direct", 6, 10, 2, 13, 17, group=2, strides=(2, 2)),
    _c3("direct 6->10 g2 hswish", "direct", 6, 10, 2, 13, 17, group=2, act="hswish"),
    _c1("direct 6->6 dw-like g6 Cout6", "direct", 6, 6, 2, 13, 17, group=6),                        # depthwise with C % 4 != 0
    Case("convt 3x3 s2 output_padding", "direct", 6, 5, 3, 3, 2, 9, 11, strides=(2, 2), pads=(1, 1, 1, 1), output_padding=(1, 1), transpose=True, poison=True),
    Case("convt 4x4 s2 p1 relu", "direct", 8, 6, 4, 4, 2, 9, 11, strides=(2, 2), pads=(1, 1, 1, 1), transpose=True, act="relu"),
    Case("convt 3x3 s2 hswish", "direct", 6, 5, 3, 3, 2, 9, 11, strides=(2, 2), pads=(1, 1, 1, 1), output_padding=(1, 1), transpose=True, act="hswish"),
    Case("convt 3x3 g3", "direct", 6, 9, 3, 3, 1, 9, 11, strides=(2, 2), group=3, transpose=True),
    Case("convt 3x3 d2", "direct", 4, 6, 3, 3, 1, 9, 11, dilations=(2, 2), pads=(2, 2, 2, 2), transpose=True),
)

def cases_of(kind):
    return [c for c in CASES if c.kind == kind]


def case_by_name(name):
    return next(c for c in CASES if c.name == name)
