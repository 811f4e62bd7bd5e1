"""The fused depthwise-separable block's case matrix: which compiled instantiation a block runs on, restated in Python, and the float64 references that
hold every instantiation to f32 accuracy -- the counterpart of f32_cases.py for csrc/dsblock*.hip.

A case is one DSBlock (depthwise k x k + act -> pointwise 1 x 1 + act, optionally Relu(Add(block, r))), or for the `rs2` family two chained blocks that
run as one launch.  `plan(case)` restates the host side of csrc/dsblock.hip -- ds_pick, rs_shape, wa_shape, cs_shape, ds_shape, rs2_shape -- and returns
the family class and the profiler name the block must run under with OAR_PROF_DETAIL=1, which names the instantiation: tests/test_gpu_dsblock_kernels.py
fails when a threshold moves and this restatement does not.  The tables RS_TABLE, CS_INST, PC_INST and RS2_INST are copies of the native ones;
tests/test_ds_cases_cpu.py reads the sources and holds the copies, the native tables and the instantiation units to each other.

`block_ref` is the operation in numpy in a chosen dtype, with the wrong edits the CPU test tells from the right reference; `bundle` gives
x6_cases.fused_bundle's tolerance, 4 max |f32 numpy - f64| (absolute).

Never set by the engine, and so not in this matrix: DsBlockP::se (the gate code of dsblock.inc and dsblock_wa.inc) and a y_ld different from Cout (the
strided store).  CPU only: numpy."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from . import x6_cases
from .onnx_writer import GraphBuilder

F32 = np.float32
FAMILIES = ("normal", "positive", "pow2")          # x6_cases.ds_inputs' families
LINEAR_ACTS = (None, "relu")                       # pow2 gives `normal`'s bits only where every activation is positively homogeneous

# ------------------------------------------------------------------------------------------------ copies of the native tables
# dsblock_rs_wpw's T (dsblock.hip) = the OAR_RS_CASE lines of dsblock_rs_k3s{11,21,12,22}.hip: sh, sw, nch, nf, x6, waves
RS_TABLE = (
    (1, 1, 1, 1, 0, 12), (1, 1, 1, 2, 0, 16), (1, 1, 2, 2, 0, 12), (1, 1, 2, 3, 0, 12), (1, 1, 2, 3, 1, 16), (1, 1, 2, 4, 0, 12), (1, 1, 2, 4, 1, 12),
    (1, 1, 3, 3, 0, 12), (1, 1, 3, 3, 1, 12), (1, 1, 3, 6, 0, 12), (1, 1, 3, 6, 1, 12), (1, 1, 4, 4, 0, 8), (1, 1, 4, 4, 1, 8), (1, 1, 4, 8, 0, 8),
    (1, 1, 4, 8, 1, 8), (1, 1, 5, 5, 0, 8), (1, 1, 5, 5, 1, 8), (1, 1, 6, 6, 0, 8), (1, 1, 6, 6, 1, 6), (1, 1, 2, 8, 0, 12),
    (2, 1, 3, 6, 0, 12), (2, 1, 3, 6, 1, 12), (2, 1, 2, 4, 0, 12), (2, 1, 2, 4, 1, 12), (2, 1, 1, 2, 0, 12), (2, 1, 4, 8, 0, 8), (2, 1, 4, 8, 1, 8),
    (1, 2, 1, 2, 0, 12), (1, 2, 2, 4, 0, 12), (1, 2, 2, 4, 1, 12), (1, 2, 3, 6, 0, 8), (1, 2, 3, 6, 1, 8), (1, 2, 4, 8, 0, 6), (1, 2, 4, 8, 1, 6),
    (2, 2, 2, 2, 0, 12), (2, 2, 2, 4, 0, 12), (2, 2, 2, 4, 1, 8), (2, 2, 4, 8, 0, 4), (2, 2, 4, 8, 1, 4), (2, 2, 1, 2, 0, 12), (2, 2, 3, 6, 0, 6), (2, 2, 3, 6, 1, 6),
)
CS_INST = ((5, 1, 1, 12, 12, 4), (3, 1, 2, 6, 12, 4), (3, 1, 1, 6, 6, 4), (5, 1, 1, 8, 8, 4), (3, 1, 1, 8, 8, 4), (3, 1, 1, 16, 16, 2), (3, 2, 2, 8, 16, 2))     # kInst: ks, sh, sw, nch, nf, rows
PC_INST = ((5, 1, 1, 12, 12, 4),)                                                                                                                    # OAR_PC_INSTANCES
RS2_INST = ((2, 3, 3, 8), (1, 2, 3, 16))                                                                                                             # kRs2: nch1, nf1, nf2, waves
WA_NF = (1, 2, 3, 4, 5, 6, 8, 12)
WA_RING = 2                                                                                                                                          # kWaRing (dsblock_dev.h)
DS_LAYOUTS = ((1, 1), (2, 1), (3, 1), (4, 1), (3, 2), (4, 2), (3, 4), (4, 4))                                                                        # (nfw, pfw)

# the per-call / per-process switches that force a family (on top of OAR_PROF_DETAIL=1)
ENV_WA = (("OAR_DSBLOCK_CS", "0"), ("OAR_DSBLOCK_RS", "0"))
ENV_WA2 = ENV_WA + (("OAR_DSBLOCK_WA", "2"),)
ENV_CS = (("OAR_DSBLOCK_CS", "2"), ("OAR_DSB_PC", "0"))
ENV_DS = (("OAR_DSBLOCK_CS", "0"), ("OAR_DSBLOCK_RS", "0"), ("OAR_DSBLOCK_WA", "0"))


@dataclass(frozen=True)
class Case:
    """One block on an [n, c, h, w] input: depthwise k x k (strides, pads top / left / bottom / right; None = k // 2 all round) + acts[0] -> pointwise
    c -> cout + acts[1].  residual: the graph is Relu(Add(pointwise, r)) with r a second input of the output's shape (acts[1] must be 'relu': that Relu).
    family 'rs2': a second 3x3 / stride-1 block cout -> c3 behind it, acts = (a1, a2, b1, b2).  env: the switches the case's child runs under.
    poison: where the case's one NaN sits (poison_at), or None."""
    name: str
    family: str           # 'rs', 'rs2', 'wa', 'cs', 'pc', 'ds': the kernel family the case is made for (plan() must agree)
    c: int
    cout: int
    k: int
    n: int
    h: int
    w: int
    strides: tuple = (1, 1)
    pads: tuple = None
    acts: tuple = (None, None)
    residual: bool = False
    c3: int = 0
    env: tuple = ()
    poison: str = None

    @property
    def pads4(self):
        return (self.k // 2,) * 4 if self.pads is None else tuple(self.pads)

    @property
    def out_hw(self):
        (sh, sw), (pt, pl, pb, pr) = self.strides, self.pads4
        return (self.h + pt + pb - self.k) // sh + 1, (self.w + pl + pr - self.k) // sw + 1

    @property
    def out_ch(self):
        return self.c3 if self.family == "rs2" else self.cout

    @property
    def in_bytes(self):
        return 4 * self.n * self.c * self.h * self.w


# ------------------------------------------------------------------------------------------------ the selection, restated
def _ceil(a, b):
    return -(-a // b)


def _plain(acts):
    return all(a in (None, "relu", "hswish") for a in acts)


def _hs(acts):
    return int(all(a == "hswish" for a in acts))


def rs_wpw(sh, sw, nch, nf, x6):
    for t in RS_TABLE:
        if t[:5] == (sh, sw, nch, nf, x6):
            return t[5]
    return 0


def rs_shape(c, env):
    """rs_shape of dsblock.hip -> dict or None"""
    (sh, sw), (pt, pl, _, _) = c.strides, c.pads4
    ho, wo = c.out_hw
    if env.get("OAR_DSBLOCK_RS") == "0" or c.k != 3:
        return None
    if c.c < 4 or c.c % 4 or c.cout <= 0 or c.cout % 4 or pt > 2 or pl > 2 or c.residual or not _plain(c.acts):
        return None
    if c.h * c.w * c.c * 4 >= 1 << 29 or c.n * ho * wo * c.cout * 4 >= 1 << 31:
        return None
    nch, nf = _ceil(c.c, 16), _ceil(c.cout, 16)
    x6 = int(int(env["OAR_DSB_RS_X6"]) != 0) if "OAR_DSB_RS_X6" in env else int(nf * nch >= 6)
    wpw = rs_wpw(sh, sw, nch, nf, x6)
    if wpw == 0:
        x6 = 1 - x6
        wpw = rs_wpw(sh, sw, nch, nf, x6)
    if wpw == 0:
        return None
    IW, NSET, ncp = 15 * sw + 3, 2 // sh + 1, (nch + 1) // 2
    SLOT = nch * IW * 64
    pwreg = not x6 and nf * nch <= 12
    tables = 10 * nch * 64 + (nf * ncp * 3 * 1024 if x6 else 0 if pwreg else nf * nch * 1024)
    if tables + wpw * SLOT * (sh + 1) > 160 * 1024:
        return None
    NR = sh + 2 if tables + wpw * SLOT * (sh + 2) <= 160 * 1024 else sh + 1
    tiles_x = _ceil(wo, 16)
    waves = 256 * wpw
    best, R, segs, items = 1e30, 0, 0, 0
    for r in range(min(ho, 4), ho + 1):
        s = _ceil(ho, r)
        it = c.n * s * tiles_x
        rounds = _ceil(it, waves)
        cost = float(rounds) * (r + (NSET - 1) * 0.7 + 0.5)
        if cost < best - 1e-9:
            best, R, segs, items = cost, r, s, it
        if r >= 64 and rounds == 1:
            break
    if int(env.get("OAR_DSB_RS_R", "0")) > 0:
        R = min(ho, int(env["OAR_DSB_RS_R"]))
        segs = _ceil(ho, R)
        items = c.n * segs * tiles_x
    if wpw * NR * SLOT + tables > 160 * 1024:
        return None
    return dict(nch=nch, nf=nf, x6=x6, wpw=wpw, acts=_hs(c.acts), NR=NR, R=R, segs=segs, items=items, waves=waves, pwreg=pwreg, tiles_x=tiles_x)


def wa_shape(c, env):
    (pt, pl, _, _) = c.pads4
    ho, wo = c.out_hw
    e = env.get("OAR_DSBLOCK_WA")
    if e == "0" or c.k != 3 or c.strides != (1, 1) or c.c % 4 or c.cout % 4 or pt > 2 or pl > 2 or not _plain(c.acts):
        return None
    if c.h * c.w * c.c * 4 >= 1 << 31:
        return None
    nf = _ceil(c.cout, 16)
    if not (nf <= 6 or nf in (8, 12)) or (nf > 4 and e != "2"):
        return None
    P = 1 if nf == 12 else 2
    TR = 4 * P
    nj = ((TR + 2) * 18 * 8 + 63) // 64
    tiles = c.n * _ceil(wo, 16) * _ceil(ho, TR)
    lds = WA_RING * nj * 1024 + _ceil(c.c, 32) * 1280 + nf * 64
    grid = max(8, _ceil(min(tiles, 256 * min(4, (160 * 1024) // lds)), 8) * 8)
    return dict(nf=nf, P=P, tiles=tiles, grid=grid)


def cs_shape(c, env):
    (sh, sw), (pt, pl, _, _) = c.strides, c.pads4
    ho, wo = c.out_hw
    e = env.get("OAR_DSBLOCK_CS")
    if e == "0" or c.k not in (3, 5) or c.c % 16 or c.cout % 16 or pt >= c.k or pl >= c.k or c.residual or not _plain(c.acts):
        return None
    if c.h * c.w * c.c * 4 >= 1 << 29 or c.n * ho * wo * c.cout * 4 >= 1 << 31:
        return None
    nch, nf = c.c // 16, c.cout // 16
    rows = next((t[5] for t in CS_INST if t[:5] == (c.k, sh, sw, nch, nf)), 0)
    if rows == 0:
        return None
    items = c.n * _ceil(ho, rows) * _ceil(wo, 16)
    grid = min(256, _ceil(_ceil(items, 4), 8) * 8)
    pc = env.get("OAR_DSB_PC", "1") != "0" and (c.k, sh, sw, nch, nf) in {t[:5] for t in PC_INST}
    return dict(nch=nch, nf=nf, rows=rows, acts=_hs(c.acts), items=items, grid=grid, iters=_ceil(items, 4 * grid), forced=e == "2", pc=pc)


def ds_shape(c, env):
    (sh, sw) = c.strides
    ho, wo = c.out_hw
    if c.k not in (3, 5) or c.c % 4 or c.cout % 4 or c.cout > 256 or (c.k == 5 and c.c >= 128 and env.get("OAR_FUSE_DSBLOCK") != "2"):
        return None
    nf = _ceil(c.cout, 16)
    nfw, pfw = (nf, 1) if nf <= 4 else ((nf + 1) // 2, 2) if nf <= 8 else ((nf + 3) // 4, 4)
    if pfw != 1 and nfw < 3:
        nfw = 3
    np_cap = (6 if sw == 1 else 11) * 64
    best = None
    for tc in (16, 32, 64):
        tr = 128 // tc
        ir, ic = (tr - 1) * sh + c.k, (tc - 1) * sw + c.k
        lds = ir * ic * 128 + (c.k * c.k + 1) * 128 + 8 * 3 * 64 * 16 + ir * ic * 4 + 16
        if ir * ic > np_cap or lds > 150 * 1024:
            continue
        tiles = c.n * _ceil(wo, tc) * _ceil(ho, tr)
        if best is None or tiles < best["tiles"] or (tiles == best["tiles"] and ir * ic < best["in_px"]):
            best = dict(tiles=tiles, in_px=ir * ic, TR=tr, TC=tc, lds=lds)
    if best is None:
        return None
    grid = max(8, _ceil(min(best["tiles"], 256 * (2 if best["lds"] * 2 <= 160 * 1024 else 1)), 8) * 8)
    return dict(best, nfw=nfw, pfw=pfw, grid=grid)


def rs2_shape(c, env):
    a, b = c, second_block(c)
    if env.get("OAR_DSBLOCK_RS2") == "0":
        return None
    for p in (a, b):
        if p.k != 3 or p.strides != (1, 1) or p.pads4 != (1, 1, 1, 1) or p.residual or not _plain(p.acts) or p.c < 4 or p.c % 4 or p.cout < 4 or p.cout % 4:
            return None
    if a.h * a.w * a.c * 4 >= 1 << 29 or b.n * b.h * b.w * b.cout * 4 >= 1 << 31:
        return None
    nch1, nf1, nf2 = _ceil(a.c, 16), _ceil(a.cout, 16), _ceil(b.cout, 16)
    lag = 0 if (env.get("OAR_DSB_RS2_VARIANT") == "1" and (nch1, nf1, nf2) == (2, 3, 3)) else 1
    wpw = 12 if not lag else next((t[3] for t in RS2_INST if t[:3] == (nch1, nf1, nf2)), 0)
    if wpw == 0:
        return None
    regw = int(bool(lag) and env.get("OAR_DSB_RS2_REGW", "1") != "0" and (nch1, nf1, nf2) == (2, 3, 3))
    nch2, ncp1, ncp2 = nf1, (nch1 + 1) // 2, (nf1 + 1) // 2
    lds = wpw * 3 * nch1 * 18 * 64 + wpw * (2 if lag else 1) * nch2 * 18 * 64 + 10 * nch1 * 64 + nf1 * ncp1 * 3 * 1024 + 10 * nch2 * 64 + nf2 * ncp2 * 3 * 1024
    if lds > 160 * 1024:
        return None
    tiles_x = _ceil(a.w, 14)
    waves = 256 * wpw
    best, R, items = 1e30, 0, 0
    for r in range(min(a.h, 4), a.h + 1):
        it = a.n * _ceil(a.h, r) * tiles_x
        rounds = _ceil(it, waves)
        cost = float(rounds) * (r + (5 if lag else 4))
        if cost < best - 1e-9:
            best, R, items = cost, r, it
        if r >= 64 and rounds == 1:
            break
    return dict(nch1=nch1, nf1=nf1, nf2=nf2, wpw=wpw, regw=regw, lag=lag, acts=_hs(c.acts), R=R, items=items) if R > 0 else None


@dataclass(frozen=True)
class Plan:
    cls: str        # the family class bench.py groups by: dsblock_rs, dsblock_wa, dsblock_cs, dsblock
    name: str       # the OAR_PROF_DETAIL name: shape and instantiation
    inst: str       # the compiled instantiation, as tests/test_ds_cases_cpu.py reads them from the sources
    family: str     # 'rs', 'rs2', 'wa', 'cs', 'pc', 'ds'
    info: dict      # the family's shape plan (rs_shape, ...)


def second_block(c):
    """the rs2 family's second block as a Case of its own (3x3, stride 1, cout -> c3 on the first block's output)"""
    return replace(c, name=c.name + " block 2", family="rs", c=c.cout, cout=c.c3, c3=0, acts=c.acts[2:], strides=(1, 1), pads=None)


def plan(c, env=None):
    """-> Plan of the case under the default environment plus `env` (default: the case's own switches)"""
    env = dict(c.env if env is None else env)
    (sh, sw) = c.strides
    ho, wo = c.out_hw
    px = c.n * ho * wo
    if c.family == "rs2":
        s = rs2_shape(c, env) if len(c.acts) == 4 else None
        assert s is not None, ("not a pair the two-block kernel takes", c)
        rw = "regw" if s["regw"] else "ldsw"
        name = f"dsblock2 px={px} C={c.c}-{c.cout}-{c.c3} rs2 R{s['R']} {s['nch1']}-{s['nf1']}-{s['nf2']} w{s['wpw']} {rw} lag{s['lag']} acts{s['acts']}"
        return Plan("dsblock_rs", name, f"rs2<{s['nch1']},{s['nf1']},{s['nf2']},{s['wpw']},{s['acts']},{s['regw']},{s['lag']}>", "rs2", s)
    head = f"dsblock px={px} C={c.c} N={c.cout} k{c.k} s{sh}x{sw}"
    cs = cs_shape(c, env)
    rs = rs_shape(c, env)
    wa = wa_shape(c, env)
    if rs is not None and not (cs is not None and cs["forced"]):
        name = f"{head} rs R{rs['R']} {rs['nch']}-{rs['nf']} {'x6' if rs['x6'] else 'f32'} acts{rs['acts']} w{rs['wpw']}"
        return Plan("dsblock_rs", name, f"rs<{sh},{sw},{rs['nch']},{rs['nf']},{rs['wpw']},{rs['acts']},{rs['x6']}>", "rs", rs)
    if wa is not None and not (cs is not None and cs["forced"]):
        return Plan("dsblock_wa", f"{head} wa{wa['P']} nf{wa['nf']}", f"wa<{wa['nf']},{wa['P']}>", "wa", wa)
    if cs is not None:
        fam = "pc" if cs["pc"] else "cs"
        return Plan("dsblock_cs", f"{head} {fam}", f"{fam}<{c.k},{sh},{sw},{cs['nch']},{cs['nf']},{cs['rows']},{cs['acts']}>", fam, cs)
    ds = ds_shape(c, env)
    assert ds is not None, ("no fused kernel takes the block", c)
    return Plan("dsblock", f"{head} t{ds['TR']}x{ds['TC']} l{ds['nfw']}x{ds['pfw']}", f"ds<{c.k},{sw},{ds['nfw']},{ds['pfw']}>", "ds", ds)


# ------------------------------------------------------------------------------------------------ inputs
def case_inputs(c, family, seed=0):
    """-> dict(x, blocks=[(wd, bd, wp, bp), ...], r): x6_cases.ds_inputs' draws for the block (and for the second one: the same draws for its channels;
    under pow2 its input already carries 2^15, so only its biases are scaled); r the residual operand (pow2: times 2^15) or None"""
    x, *blk = x6_cases.ds_inputs(c, family, seed)
    blocks = [tuple(blk)]
    ho, wo = c.out_hw
    if c.family == "rs2":
        b2 = second_block(c)
        base = "normal" if family == "pow2" else family
        _, wd, bd, wp, bp = x6_cases.ds_inputs(replace(b2, n=1, h=1, w=1), base, seed + 2)
        if family == "pow2":
            bd, bp = np.ldexp(bd, x6_cases.POW2_B), np.ldexp(bp, x6_cases.POW2_B)
        blocks.append((wd, bd, wp, bp))
    r = None
    if c.residual:
        base = "normal" if family == "pow2" else family
        rng = np.random.default_rng([seed, c.n, c.cout, ho, wo, FAMILIES.index(base), 7])
        r = (rng.standard_normal((c.n, c.cout, ho, wo)) if base == "normal" else rng.uniform(1, 2, (c.n, c.cout, ho, wo))).astype(F32)
        if family == "pow2":
            r = np.ldexp(r, x6_cases.POW2_B)
    return dict(x=x, blocks=blocks, r=r)


def families_of(c):
    """pow2 reproduces `normal` bit for bit only under activations none / Relu"""
    return FAMILIES if all(a in LINEAR_ACTS for a in c.acts) else FAMILIES[:2]


# Poison: one case per family carries one NaN in its `normal` input.  fmaxf swallows a NaN, so a poisoned case has no Relu: every poison case below runs in
# its own form -- all-HardSwish (rs, rs2, cs, pc) or without activations (wa, ds) -- and is compared with its own clean `normal` run.
POISON_KINDS = {
    "last row": "the last row of image 0, in a column two strips share: must reach both strips' outputs of that image and nothing of image 1",
    "halo": "a column two 16-wide strips share (input column 16), last image: must reach both strips",
    "tail": "the last channel of a channel tail, middle of the last image",
    "corner": "rs2: the first pixel of image 1 -- its intermediate neighbours above and to the left lie outside the image",
}


def poison_at(c):
    """-> (image, channel, row, column) of the case's one NaN"""
    assert c.poison in POISON_KINDS, c.poison
    if c.poison == "last row":
        return 0, c.c // 2, c.h - 1, min(c.w - 1, 16 * c.strides[1])
    if c.poison == "halo":
        return c.n - 1, 0, c.h // 2, min(c.w - 1, 16 * c.strides[1])
    if c.poison == "tail":
        return c.n - 1, c.c - 1, c.h // 2, c.w // 2
    return min(1, c.n - 1), c.c // 2, 0, 0


def poisoned(c, x):
    x = x.copy()
    x[poison_at(c)] = np.nan
    return x


# ------------------------------------------------------------------------------------------------ references
EDITS = ("tap", "clamp", "bias", "ring", "mid", "x6")


def act_ref(a, kind):
    """x6_cases.act_ref plus swish (x sigmoid(x)): the activation only dsblock.inc takes"""
    if kind == "swish":
        with np.errstate(over="ignore"):
            return a / (a.dtype.type(1) + np.exp(-a))
    return x6_cases.act_ref(a, kind)


def _dw(xl, wd, bd, k, strides, pads, dt, edit=None, at=0):
    """depthwise k x k on channels-last xl [n, h, w, c] in dt -> [n, ho, wo, c], no activation.  edit 'clamp': the padding replicates the edge pixel;
    'tap': the tap (pt, pl) -- the one that reads a real pixel whatever the shape -- is left out of the border pixel (row 0, column `at`) of image 0"""
    n, h, w, c = xl.shape
    (sh, sw), (pt, pl, pb, pr) = strides, pads
    ho, wo = (h + pt + pb - k) // sh + 1, (w + pl + pr - k) // sw + 1
    need_h, need_w = (ho - 1) * sh + k, (wo - 1) * sw + k
    xp = np.pad(xl, ((0, 0), (pt, max(0, need_h - h - pt)), (pl, max(0, need_w - w - pl)), (0, 0)), mode="edge" if edit == "clamp" else "constant")
    wt = np.asarray(wd).astype(dt)
    t = np.broadcast_to(np.asarray(bd).astype(dt), (n, ho, wo, c)).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(k):
            for j in range(k):
                t += xp[:, i:i + (ho - 1) * sh + 1:sh, j:j + (wo - 1) * sw + 1:sw] * wt[:, 0, i, j]
        if edit == "tap":
            t[0, 0, at] -= xp[0, pt, at * sw + pl] * wt[:, 0, pt, pl]
    return t


def _block(xl, blk, k, strides, pads, acts, dt, r=None, edit=None, at=0):
    """one block on channels-last xl -> channels-last [n, ho, wo, cout] in dt.  edit: 'tap' / 'clamp' (see _dw); 'ring': the middle output row of image 0's
    first strip is computed from the input one row later; 'bias': the pointwise bias is left out of the cout fragments after the first;
    'x6' / 'x6:<fault>': the pointwise runs through x6_cases.x6_matmul on the f32 depthwise output (fault 'no mm' by default, 'x6:' = fault-free)"""
    wd, bd, wp, bp = blk
    t = _dw(xl, wd, bd, k, strides, pads, dt, edit, at)
    if edit == "ring":
        later = np.concatenate([xl[:, 1:], np.zeros_like(xl[:, :1])], 1)
        oy = t.shape[1] // 2
        t[0, oy, :16] = _dw(later, wd, bd, k, strides, pads, dt)[0, oy, :16]
    n, ho, wo, c = t.shape
    t = act_ref(t, acts[0]).reshape(-1, c)
    W = np.asarray(wp)[:, :, 0, 0].T
    b = np.asarray(bp).astype(dt).copy()
    if edit == "bias":
        b[16:] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        if edit is not None and edit.startswith("x6"):
            fault = edit[3:] if ":" in edit else "no mm"
            y = x6_cases.x6_matmul(t.astype(F32), W, np.asarray(bp, F32), fault=fault or None).astype(dt)
        else:
            y = t @ W.astype(dt) + b
        y = y.reshape(n, ho, wo, -1)
        if r is not None:
            y = y + np.asarray(r).transpose(0, 2, 3, 1).astype(dt)
    return act_ref(y, acts[1])


def block_ref(c, inp, dtype="float64", edit=None, x=None, at=0):
    """the case in `dtype` -> [n, out_ch, ho, wo].  inp: case_inputs' dict (x: another input in its place, the poisoned one).  at: the column of the
    border pixel the 'tap' edit hits.  edit: one of EDITS (see
    _block; for the two-block chain 'tap', 'clamp' and 'ring' hit block 1, 'bias' and 'x6' block 2); 'mid' (rs2 only): the intermediate tensor is not zeroed
    outside the image -- block 2's padding ring holds what block 1 computes there from the zero-extended input."""
    dt = np.dtype(dtype)
    xl = np.ascontiguousarray(np.asarray(inp["x"] if x is None else x).transpose(0, 2, 3, 1)).astype(dt)
    if c.family != "rs2":
        assert edit != "mid"
        y = _block(xl, inp["blocks"][0], c.k, c.strides, c.pads4, c.acts, dt, inp["r"], edit, at)
    elif edit == "mid":
        wide = np.pad(xl, ((0, 0), (1, 1), (1, 1), (0, 0)))
        mid = _block(wide, inp["blocks"][0], 3, (1, 1), (1, 1, 1, 1), c.acts[:2], dt)
        y = _block(mid, inp["blocks"][1], 3, (1, 1), (0, 0, 0, 0), c.acts[2:], dt)
    else:
        first = edit if edit in ("tap", "clamp", "ring") else None
        mid = _block(xl, inp["blocks"][0], 3, (1, 1), (1, 1, 1, 1), c.acts[:2], dt, None, first, at)
        y = _block(mid, inp["blocks"][1], 3, (1, 1), (1, 1, 1, 1), c.acts[2:], dt, None, None if first else edit)
    out = np.ascontiguousarray(y.transpose(0, 3, 1, 2))
    assert out.shape == (c.n, c.out_ch, *c.out_hw), (out.shape, c)
    return out


def bundle(c, inp):
    """x6_cases.fused_bundle of the case: dict(f64, scale, noise, tol), tol = 4 max |f32 numpy - f64| (absolute)"""
    return x6_cases.fused_bundle(lambda dt: block_ref(c, inp, dt))


def x6_pointwise(c, env=None):
    """does the case's (last) pointwise product run as bf16x6 -- every family but the row-streaming kernel with the f32 matrix instruction"""
    p = plan(c, env)
    return p.family != "rs" or bool(p.info["x6"])


def reads_padding(c):
    """does any tap of any output read outside the image (stride 2 on an odd size never reaches a bottom / right padding of 1)"""
    (sh, sw), (pt, pl, _, _) = c.strides, c.pads4
    ho, wo = c.out_hw
    return pt > 0 or pl > 0 or (ho - 1) * sh + c.k > c.h + pt or (wo - 1) * sw + c.k > c.w + pl


def reduced(c, h=9, w=19):
    """the case on at most two small images (the CPU test's wrong edits): same block, h x w input at most"""
    return replace(c, n=min(c.n, 2), h=min(c.h, h), w=min(c.w, w))


# ------------------------------------------------------------------------------------------------ graphs
def _act_node(g, t, kind):
    if kind == "relu":
        return g.op("Relu", [t])
    if kind == "hswish":
        return g.op("HardSwish", [t])
    if kind == "swish":
        return g.op("Mul", [t, g.op("Sigmoid", [t])])
    assert kind is None, kind
    return t


def _block_nodes(g, src, blk, k, strides, pads, acts, c, residual=None):
    wd, bd, wp, bp = blk
    t = _act_node(g, g.op("Conv", [src, g.init(wd), g.init(bd)], kernel_shape=[k, k], strides=list(strides), pads=list(pads), group=c, dilations=[1, 1]), acts[0])
    y = g.op("Conv", [t, g.init(wp), g.init(bp)], kernel_shape=[1, 1], strides=[1, 1], pads=[0, 0, 0, 0], group=1, dilations=[1, 1])
    if residual:
        assert acts[1] == "relu"
        return g.op("Relu", [g.op("Add", [y, residual])])
    return _act_node(g, y, acts[1])


def model(c, inp):
    """the one-block graph (inputs x, and r for a residual), or the two-block chain for the rs2 family"""
    g = GraphBuilder("ds")
    g.add_input("x", [c.n, c.c, c.h, c.w])
    ho, wo = c.out_hw
    if c.residual:
        g.add_input("r", [c.n, c.cout, ho, wo])
    y = _block_nodes(g, "x", inp["blocks"][0], c.k, c.strides, c.pads4, c.acts[:2], c.c, "r" if c.residual else None)
    if c.family == "rs2":
        y = _block_nodes(g, y, inp["blocks"][1], 3, (1, 1), (1, 1, 1, 1), c.acts[2:], c.cout)
    g.add_output(y, [c.n, c.out_ch, ho, wo])
    return g.model()


# ------------------------------------------------------------------------------------------------ the matrix
_GENERIC = ((None, None), ("relu", "relu"), ("hswish", "relu"), ("relu", None))     # the acts = 0 template: everything but all-HardSwish
_HS = ("hswish", "hswish")
_TAILS = ((0, 0), (1, 2), (2, 3), (3, 1), (0, 1), (2, 0))                            # (t, u): C = 16 nch - 4 t, Cout = 16 nf - 4 u


def _in_hw(ho, wo, strides, k=3):
    """an input that gives ho x wo outputs under padding k // 2 -- odd where the stride is 2"""
    return (ho - 1) * strides[0] + 1, (wo - 1) * strides[1] + 1


def _rs_grid():
    """every row of RS_TABLE with both acts templates, 2 images of 7 x (19 | 21 | 29) outputs (R = 4: the second row segment holds 3 rows; two strips, the
    second ragged), channel tails that rotate with the row"""
    out = []
    have = {t[:5] for t in RS_TABLE}
    for i, (sh, sw, nch, nf, x6, wpw) in enumerate(RS_TABLE):
        t, u = _TAILS[i % len(_TAILS)]
        cin, cout = max(8, 16 * nch - 4 * t), 16 * nf - 4 * u
        h, w = _in_hw(7, (19, 21, 29)[i % 3], (sh, sw))
        env = ()
        if (sh, sw, nch, nf, 1 - x6) in have and x6 != int(nf * nch >= 6):
            env = (("OAR_DSB_RS_X6", str(x6)),)
        for acts in (_GENERIC[i % len(_GENERIC)], _HS):
            a = "hs" if acts == _HS else "gen"
            out.append(Case(f"rs s{sh}{sw} {nch}-{nf} {'x6' if x6 else 'f32'} {a} {cin}->{cout}", "rs", cin, cout, 3, 2, h, w, strides=(sh, sw), acts=acts, env=env))
    return out


def _rs_extras():
    """per unit: pads [0, 0, 1, 1]; R = 1 and a forced R = 3 over 7 rows; more items than one round of waves.  Unit (1, 1) also unpadded."""
    out = []
    # (strides, C, Cout): a narrow f32 row and an x6 row per unit where the unit has one
    rows = {(1, 1): ((16, 32), (48, 96)), (2, 1): ((12, 32), (48, 92)), (1, 2): ((16, 28), (32, 64)), (2, 2): ((16, 32), (44, 96))}
    for (sh, sw), ((c0, n0), (c1, n1)) in rows.items():
        s = f"s{sh}{sw}"
        h, w = _in_hw(7, 21, (sh, sw))
        out.append(Case(f"rs {s} pads 0,0,1,1 {c1}->{n1}", "rs", c1, n1, 3, 2, h, w, strides=(sh, sw), pads=(0, 0, 1, 1), acts=_HS))
        out.append(Case(f"rs {s} R1 {c0}->{n0}", "rs", c0, n0, 3, 2, h, w, strides=(sh, sw), acts=("relu", "relu"), env=(("OAR_DSB_RS_R", "1"),)))
        out.append(Case(f"rs {s} R1 {c1}->{n1}", "rs", c1, n1, 3, 2, h, w, strides=(sh, sw), acts=_HS, env=(("OAR_DSB_RS_R", "1"),)))
        out.append(Case(f"rs {s} R3 of 7 {c0}->{n0}", "rs", c0, n0, 3, 2, h, w, strides=(sh, sw), acts=_HS, env=(("OAR_DSB_RS_R", "3"),)))
        out.append(Case(f"rs {s} R3 of 7 {c1}->{n1}", "rs", c1, n1, 3, 2, h, w, strides=(sh, sw), acts=(None, "relu"), env=(("OAR_DSB_RS_R", "3"),)))
    out.append(Case("rs s11 unpadded 48->96", "rs", 48, 96, 3, 2, 9, 23, pads=(0, 0, 0, 0), acts=("relu", "relu")))
    # many items: Ho = 3 or 2 (one segment), two strips, so items = 2 n: just above one round of 256 wpw waves and no multiple of it
    out.append(Case("rs s11 many items 16->16", "rs", 16, 16, 3, 1700, 3, 19, acts=_HS, poison="last row"))                                # 12 waves: 3400 items over 3072 waves
    out.append(Case("rs s21 many items 16->32", "rs", 16, 32, 3, 1700, 3, 19, strides=(2, 1), acts=("relu", "relu")))                 # 12 waves, Ho = 2
    out.append(Case("rs s12 many items 12->28", "rs", 12, 28, 3, 1700, 2, 37, strides=(1, 2), acts=_HS))                              # 12 waves, Ho = 2
    out.append(Case("rs s22 many items 60->124", "rs", 60, 124, 3, 600, 3, 37, strides=(2, 2), acts=(None, None)))                    # 4 waves: 1200 items over 1024 waves
    return out


def _rs2_grid():
    return [
        Case("rs2 24-48-48 hs", "rs2", 24, 48, 3, 2, 7, 29, acts=_HS * 2, c3=48, poison="corner"),
        Case("rs2 20-44-36 mixed two rows", "rs2", 20, 44, 3, 3, 2, 15, acts=("hswish", "relu", None, "relu"), c3=36),
        Case("rs2 16-24-48 hs one row", "rs2", 16, 24, 3, 2, 1, 13, acts=_HS * 2, c3=48),
        Case("rs2 12-20-40 mixed", "rs2", 12, 20, 3, 3, 9, 29, acts=("relu", "relu", "relu", None), c3=40),
        Case("rs2 24-48-48 ldsw hs two rows", "rs2", 24, 48, 3, 2, 2, 29, acts=_HS * 2, c3=48, env=(("OAR_DSB_RS2_REGW", "0"),)),
        Case("rs2 20-36-44 ldsw mixed", "rs2", 20, 36, 3, 2, 7, 15, acts=(None, None, "relu", "relu"), c3=44, env=(("OAR_DSB_RS2_REGW", "0"),)),
        Case("rs2 24-48-48 no lag hs", "rs2", 24, 48, 3, 2, 9, 15, acts=_HS * 2, c3=48, env=(("OAR_DSB_RS2_VARIANT", "1"),)),
        Case("rs2 28-40-36 no lag mixed one row", "rs2", 28, 40, 3, 3, 1, 29, acts=("relu", "hswish", "relu", "relu"), c3=36, env=(("OAR_DSB_RS2_VARIANT", "1"),)),
        Case("rs2 24-48-48 no lag single strip", "rs2", 24, 48, 3, 2, 5, 14, acts=(None, None, None, None), c3=48, env=(("OAR_DSB_RS2_VARIANT", "1"),)),
    ]


def _wa_grid():
    out = []
    for i, nf in enumerate(WA_NF):
        t, u = _TAILS[i % len(_TAILS)]
        cin, cout = max(8, 16 * (1 + i % 3) - 4 * t), 16 * nf - 4 * u
        env = ENV_WA if nf <= 4 else ENV_WA2
        out.append(Case(f"wa nf{nf} {cin}->{cout}", "wa", cin, cout, 3, 2, 11, (19, 21, 29)[i % 3], acts=(_HS, ("relu", "relu"), (None, None))[i % 3], env=env,
                        poison="halo" if nf == 3 else None))
    out.append(Case("wa nf3 residual 24->44", "wa", 24, 44, 3, 2, 11, 21, acts=("hswish", "relu"), residual=True, env=ENV_WA))
    out.append(Case("wa nf6 residual 40->96", "wa", 40, 96, 3, 2, 11, 21, acts=("relu", "relu"), residual=True, env=ENV_WA2))
    out.append(Case("wa nf1 more tiles than workgroups 8->12", "wa", 8, 12, 3, 3, 171, 261, acts=("relu", "relu"), env=ENV_WA))                  # 3 x 22 x 17 = 1122 tiles over 1024 workgroups
    return out


def _cs_grid():
    out = []
    for i, (ks, sh, sw, nch, nf, rows) in enumerate(CS_INST):
        ho = 9 if rows == 4 else 5                       # three segments, the last one ragged
        h, w = _in_hw(ho, 19, (sh, sw), ks)
        for acts in (_GENERIC[i % len(_GENERIC)], _HS):
            a = "hs" if acts == _HS else "gen"
            out.append(Case(f"cs k{ks} s{sh}{sw} {16 * nch}->{16 * nf} {a}", "cs", 16 * nch, 16 * nf, ks, 3, h, w, strides=(sh, sw), acts=acts, env=ENV_CS,
                            poison="last row" if (ks, nch, acts) == (5, 12, _HS) else None))                        # 3 x 3 x 2 = 18 items
    out.append(Case("cs k3 s11 96->96 two rounds", "cs", 96, 96, 3, 3, 199, 100, acts=("relu", "relu"), env=ENV_CS))            # 3 x 50 x 7 = 1050 items over 1024 waves
    return out


def _pc_grid():
    return [
        Case("pc k5 192->192 hs", "pc", 192, 192, 5, 3, 9, 19, acts=_HS, poison="last row"),
        Case("pc k5 192->192 relu", "pc", 192, 192, 5, 3, 9, 19, acts=("relu", "relu")),
        Case("pc k5 192->192 two rounds", "pc", 192, 192, 5, 3, 199, 100, acts=_HS),                                             # 1050 items over 1024 consumer groups
    ]


def _ds_grid():
    """all eight (nfw, pfw) layouts -- nf = 1, 2, 3, 4, 6, 8, 12, 16 -- in each of the four units (kernel size, column stride), the row stride alternating"""
    out = []
    i = 0
    for ks in (3, 5):
        for sw in (1, 2):
            for j, nf in enumerate((1, 2, 3, 4, 6, 8, 12, 16)):
                sh = 1 + (i + j) % 2
                t, u = _TAILS[(i + j) % len(_TAILS)]
                cin, cout = max(8, 16 * (1 + j % 2) - 4 * t), 16 * nf - 4 * u
                ho, wo = ((7, 19), (17, 21), (2, 70))[(i + j) % 3]
                h, w = _in_hw(ho, wo, (sh, sw), ks)
                acts = (("relu", "relu"), _HS, (None, None), ("hswish", "relu"))[j % 4]
                out.append(Case(f"ds k{ks} s{sh}{sw} nf{nf} {cin}->{cout}", "ds", cin, cout, ks, 2, h, w, strides=(sh, sw), acts=acts, env=ENV_DS,
                                poison="tail" if (ks, sw, nf) == (3, 1, 3) else None))
            i += 1
    out.append(Case("ds k3 residual 24->40", "ds", 24, 40, 3, 2, 13, 37, strides=(2, 2), acts=("hswish", "relu"), residual=True, env=ENV_DS))
    out.append(Case("ds k5 swish 20->12", "ds", 20, 12, 5, 2, 9, 21, acts=("swish", "swish"), env=ENV_DS))
    out.append(Case("ds k3 more tiles than workgroups 8->16", "ds", 8, 16, 3, 2, 171, 203, acts=("relu", "relu"), env=ENV_DS))
    return out


CASES = tuple(_rs_grid() + _rs_extras() + _rs2_grid() + _wa_grid() + _cs_grid() + _pc_grid() + _ds_grid())


def groups():
    """the child processes: one per distinct env tuple, in the matrix's order -> {env tuple: [cases]}"""
    out = {}
    for c in CASES:
        out.setdefault(tuple(sorted(c.env)), []).append(c)
    return out


def case_by_name(name):
    return next(c for c in CASES if c.name == name)
