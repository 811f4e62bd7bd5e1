"""The sample-local chain kernel's case matrix (csrc/chain.hip): short ONNX graphs whose middle is ONE fusable run, the planner's and the
kernel's choices for that run restated in Python, and the run in numpy -- the counterpart of ds_cases.py for chain_kernel.

A case is a list of operators on one sample-local tensor family ([n, T, C] tokens, or the same rows as an [n, C, 1, T] map): products (1 x kw convolutions
and Linears with bias, one of six activations, a residual), LayerNorm, the fused SVTR attention (spelled as models.build_rec spells it, so that rewrite pass 5
makes one Attention node of it), the full-height average pool and a two-input channel Concat.  `plan(case, env)` restates Planner::fuse_chains (engine.cc)
-- does the run fuse, copy elision, staging copies, mb / ksplit / kper, which tensors live in LDS -- and the three dispatch rules of kernels.h
(chain_gemm_path, chain_ln_float4, chain_attn_tiles), and returns the profiler name the run must go under with OAR_PROF_DETAIL=1: one token per operator
of the launch's table.  tests/test_chain_cases_cpu.py holds the restatement to the C++ sources; tests/test_gpu_chain_kernel.py holds it to what runs.

`ref(case, inputs, dtype)` is the run in numpy in a chosen dtype, with the wrong edits the CPU test tells from the right reference; `bundle` gives
x6_cases.fused_bundle's tolerance, 4 max |f32 numpy - f64| (absolute).  CPU only: numpy."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

from . import x6_cases
from .onnx_writer import GraphBuilder

F32 = np.float32
FAMILIES = ("normal", "positive", "large")
LARGE_GAIN = 3.0            # `large`: the input times this, so that the attention scores (quadratic in it) reach about +-60

# ------------------------------------------------------------------------------------------------ constants restated (tests/test_chain_cases_cpu.py reads the sources)
K_MIN_CHAIN = 3             # Planner::kMinChain
K_CHAIN_MAX_HD = 16         # kernels.h kChainMaxHd
K_LDS_BUDGET = 159 * 1024   # kernels.h kChainLdsBudget
K_MAX_MFLOP = 32.0          # fuse_chains: per-sample cap of a fused run
K_NAME_FIT = 95             # chain_detail_name: oar_prof_entry::name holds 96 bytes
K_WAVES = 16
ACT_LETTER = {None: "", "relu": "R", "hswish": "H", "hsigmoid": "G", "sigmoid": "S", "swish": "W"}
NAN_KEEPING_ACTS = (None, "sigmoid", "swish")      # the others go through a select / fmaxf that swallows a NaN

ENV_HBM = (("OAR_CHAIN_LDS", "0"),)                # every tensor of the run stays in the arena: all products take the general path
ENV_UNFUSED = (("OAR_FUSE_CHAIN", "0"),)           # the control: operator by operator


@dataclass(frozen=True)
class Op:
    """kind: 'conv' (1 x kw over the [n, C, 1, T] map), 'lin' (Linear over tokens), 'ln', 'attn', 'pool', 'cat'.
    src / res / cat: indices of the operators whose outputs are read (-1: the case's input; default src: the operator in front)."""
    kind: str
    n: int = 0                 # products: output channels
    kw: int = 1
    pl: int = 0                # left pad (right pad = kw - 1 - pl: the width stays T)
    act: str = None
    alpha: float = 0.2         # hsigmoid
    beta: float = 0.5
    res: int = None
    src: int = None
    affine: str = "gb"         # ln: 'gb' gamma and beta, 'g' gamma only
    eps: float = 1e-5
    heads: int = 0
    hd: int = 0
    scale: float = None        # attn: None = hd ** -0.5
    kh: int = 0                # pool: window rows (= the map's height); kw = window columns
    cat: tuple = ()


@dataclass(frozen=True)
class Case:
    """input: 'tok' -- a graph input [n, T, C] (the run reads the input itself: ChainRef kind 2); 'map' -- a graph input [n, C, 1, T], which a layout
    conversion in front of the run copies into the arena (kind 1); 'pool' -- [n, C, kh, W] for a pool as the first operator (W = kw T + odd)."""
    name: str
    n: int
    T: int
    c: int
    ops: tuple
    input: str = "tok"
    odd: int = 0               # pool: extra columns of the map that the pool drops
    families: tuple = ("normal", "positive")
    poison: tuple = None       # (token, channel) of sample 1's NaN, or None
    hbm_too: bool = False      # the case also runs in the OAR_CHAIN_LDS=0 child
    overflow: bool = False     # tensors exceed the LDS budget on purpose: plan() gives no exact name

    @property
    def in_shape(self):
        if self.input == "tok":
            return (self.n, self.T, self.c)
        if self.input == "map":
            return (self.n, self.c, 1, self.T)
        p = self.ops[0]
        return (self.n, self.c, p.kh, p.kw * self.T + self.odd)


# ------------------------------------------------------------------------------------------------ shapes
def _src(ops, i):
    return i - 1 if ops[i].src is None else ops[i].src


def widths(c):
    """-> output channels of every operator (index -1: the input), as a dict"""
    w = {-1: c.c}
    for i, o in enumerate(c.ops):
        if o.kind in ("conv", "lin"):
            w[i] = o.n
        elif o.kind == "attn":
            assert w[_src(c.ops, i)] == 3 * o.heads * o.hd, (c.name, i)
            w[i] = o.heads * o.hd
        elif o.kind == "cat":
            w[i] = sum(w[s] for s in o.cat)
        else:
            w[i] = w[_src(c.ops, i)]
    return w


# ------------------------------------------------------------------------------------------------ the planner and the dispatch, restated
def gemm_path(in_lds, mb, K, ksplit):
    """chain_gemm_path (kernels.h) = the product branch of chain_kernel's switch"""
    if in_lds and mb == 1 and ((K >> 4) + ksplit - 1) // ksplit < 4:
        return "gs"
    if in_lds and mb == 1:
        return "g1"
    if in_lds and mb == 2:
        return "g2"
    if in_lds:
        return "g3"
    return "gh"


def ln_float4(C):
    return C <= 256 and (C & 3) == 0


def attn_tiles(T, hd):
    if T <= 64 and (hd & 3) == 0:
        return 1 if T <= 16 else 2 if T <= 32 else 3 if T <= 48 else 4
    return 0


def mb_ksplit(T, N, K):
    """fuse_chains' work split of one product -> (mb, ksplit, kper)"""
    MT, NT, KB = (T + 15) // 16, N // 16, K // 16
    mb = 1 if (NT * MT <= 16 and KB <= 8) else (MT if MT <= 3 else (3 if MT % 3 == 0 else (2 if MT % 2 == 0 else 3)))
    MG = (MT + mb - 1) // mb
    ks = 1
    while NT * MG * ks < 16 and KB // (ks * 2) >= 2 and NT * MG * mb * ks * 2 <= 24:
        ks *= 2
    return mb, ks, (KB + ks - 1) // ks


def split_scratch(T, N, mb, ksplit):
    """chain_lds_bytes (chain.hip): the split-K partials of one product"""
    if ksplit <= 1:
        return 0
    MT = (T + 15) // 16
    return (N // 16) * ((MT + mb - 1) // mb) * mb * ksplit * 64 * 16


def detail_name(n, T, tokens):
    """chain_detail_name (chain.hip)"""
    head = f"chain n={n} T={T}"
    sig = " ".join(tokens)
    if len(head) + 1 + len(sig) <= K_NAME_FIT:
        return head + " " + sig
    seen = {}
    for t in tokens:
        seen[t] = seen.get(t, 0) + 1
    counted = head + "".join(f" {t}" + (f"x{k}" if k > 1 else "") for t, k in seen.items())
    if len(counted) <= K_NAME_FIT:
        return counted
    fam = {}
    for t, k in seen.items():
        fam[t[:2]] = fam.get(t[:2], 0) + k
    out = head + " ~" + "".join(f" {f}x{k}" for f, k in fam.items())
    assert len(out) <= K_NAME_FIT, out
    return out


def first_fit_peak(tab, bytes_of):
    """chain_place_in_lds (engine.cc) without its eviction loop: the tensors of `bytes_of` (id -> bytes) placed first-fit in the order of their first use, a
    slot reusable once its tensor's last use is an earlier operator; operator j's split-K partials own [0, scratch_j) while it runs -> the peak"""
    life = {}
    for j, e in enumerate(tab):
        for d in (e["dst"], e["src"], e["res"]):
            if d in bytes_of:
                lo, hi = life.get(d, (j, j))
                life[d] = (min(lo, j), max(hi, j))
    placed = []                                          # (offset, bytes, last)
    peak = max([e["scratch"] for e in tab] + [0])
    for d in sorted(life, key=lambda d: life[d][0]):     # (stable: ties keep the table's order, as std::sort does for the few ties a run has)
        first, last = life[d]
        busy = sorted((off, off + b) for off, b, l in placed if l >= first)
        part = max(e["scratch"] for e in tab[first:last + 1])
        if part:
            busy = sorted(busy + [(0, part)])
        off = 0
        for b0, b1 in busy:
            if off + bytes_of[d] <= b0:
                break
            off = max(off, b1)
        placed.append((off, bytes_of[d], last))
        peak = max(peak, off + bytes_of[d])
    return peak


@dataclass
class Plan:
    name: str            # the OAR_PROF_DETAIL name, None for the overflow case
    tokens: list         # one per operator of the launch's table
    table: list          # the table: dicts (type, K, N, cin, pad, mb, ksplit, kper, src, dst, res, in_lds, res_lds, op)
    lds_bytes: int       # the peak of the planner's first-fit placement with every tensor of the run in LDS (first_fit_peak)
    features: set = field(default_factory=set)


def _table(c):
    """the run as the planner records it: one entry per chainable step, tensors as ids (-1 the input, i the output of operator i, ('cat', i) a concat buffer)"""
    w = widths(c)
    tab = []
    for i, o in enumerate(c.ops):
        s = _src(c.ops, i)
        if o.kind in ("conv", "lin"):
            tab.append(dict(type="gemm", K=o.kw * w[s], N=o.n, cin=w[s], pad=o.pl, src=s, dst=i, res=o.res, act=o.act, op=i, fix=o.kw > 1))
        elif o.kind == "ln":
            tab.append(dict(type="ln", N=w[s], src=s, dst=i, res=None, op=i, fix=False))
        elif o.kind == "attn":
            tab.append(dict(type="attn", N=w[i], hd=o.hd, heads=o.heads, src=s, dst=i, res=None, op=i, fix=True))
        elif o.kind == "pool":
            tab.append(dict(type="pool", N=w[s], src=None, dst=i, res=None, op=i, fix=True))       # (its input is the sample's map: not a tensor of the run)
        elif o.kind == "cat":
            off = 0
            for s in o.cat:
                tab.append(dict(type="copy", N=w[s], src=s, dst=i, off=off, res=None, op=i, fix=False))
                off += w[s]
        else:
            raise ValueError(o.kind)
    return tab


def run_flops(c):
    """per sample, as the planner counts them: 2 M N K of every product, 4 h T T d of an attention, 8 C per LayerNorm row"""
    w = widths(c)
    f = 0.0
    for i, o in enumerate(c.ops):
        s = _src(c.ops, i)
        if o.kind in ("conv", "lin"):
            f += 2.0 * c.T * o.n * o.kw * w[s]
        elif o.kind == "attn":
            f += 4.0 * o.heads * c.T * c.T * o.hd
        elif o.kind == "ln":
            f += 8.0 * c.T * w[s]
    return f


def plan(c, env=None):
    """-> Plan of the case's run under the default environment plus `env`"""
    env = dict(env or ())
    assert env.get("OAR_FUSE_CHAIN", "1") != "0", "the control has no chain"
    T, w = c.T, widths(c)
    tab = _table(c)
    # ---- does the run fuse
    assert len(tab) >= K_MIN_CHAIN and any(e["fix"] for e in tab), (c.name, "no run")
    assert run_flops(c) <= K_MAX_MFLOP * 1e6, (c.name, run_flops(c))
    for e in tab:
        if e["type"] == "gemm":
            assert e["K"] % 16 == 0 and e["N"] % 16 == 0 and e["cin"] % 16 == 0, (c.name, e)
        if e["type"] == "attn":
            assert e["hd"] <= K_CHAIN_MAX_HD and e["hd"] % 4 == 0, (c.name, e)
        if e["type"] in ("pool", "copy"):
            assert e["N"] % 4 == 0, (c.name, e)
    last = len(c.ops) - 1                                # the run's last tensor is the graph's output: it stays in the arena
    # ---- copy elision: a Concat input produced inside the run by one operator and read by nothing else
    j = 0
    while j < len(tab):
        cp = tab[j]
        if cp["type"] == "copy" and cp["src"] >= 0:
            prod = [q for q in range(j) if tab[q]["type"] != "copy" and tab[q]["dst"] == cp["src"] and "off" not in tab[q]]
            readers = [q for q in range(len(tab)) if q != j and (tab[q]["src"] == cp["src"] or tab[q]["res"] == cp["src"])]
            if prod and not readers and cp["src"] != last:
                tab[prod[-1]].update(dst=cp["dst"], off=cp["off"])
                del tab[j]
                continue
        j += 1
    # ---- staging copies: a product whose tokens were not written in the run reads them from a transient LDS copy
    lds_on = env.get("OAR_CHAIN_LDS", "1") != "0"
    out = []
    for e in tab:
        if e["type"] == "gemm" and e["src"] == -1 and lds_on and not c.overflow:
            out.append(dict(type="copy", N=e["cin"], src=-1, dst=("stage", e["op"]), res=None, op=e["op"], fix=False))
            e = dict(e, src=("stage", e["op"]))
        out.append(e)
    tab = out
    # ---- placement: written in the run and not read after it -> LDS (the CPU test shows the budget is far away; the overflow case has no exact name)
    def in_lds(t):
        return lds_on and t is not None and t != -1 and t != last
    ld = {}
    for e in tab:
        d = e["dst"]
        ld[d] = w[d] if not isinstance(d, tuple) else e["N"]
    scratch = 0
    tokens, feats = [], set()
    for e in tab:
        if e["type"] == "gemm":
            e["mb"], e["ksplit"], e["kper"] = mb_ksplit(T, e["N"], e["K"])
            e["in_lds"], e["res_lds"] = in_lds(e["src"]), in_lds(e["res"])
            scratch = max(scratch, (split_scratch(T, e["N"], e["mb"], e["ksplit"]) + 255) & ~255)
            p = gemm_path(e["in_lds"], e["mb"], e["K"], e["ksplit"])
            has_res = e["res"] is not None
            assert not (has_res and e["act"]), (c.name, "rewrite pass 4 folds a residual only into a product without activation")
            tokens.append(p + (f"k{e['ksplit']}" if e["ksplit"] > 1 else "") + ("r" if has_res else "") + ACT_LETTER[e["act"]])
            feats |= {p, p + ("+split" if e["ksplit"] > 1 else "+whole"), "act:" + str(e["act"]), "taps:%d" % (e["K"] // e["cin"])}
            if has_res:
                feats |= {"res", "res:lds" if e["res_lds"] else "res:hbm", p + "+res"}
            if e["ksplit"] > 1 and e["ksplit"] * e["kper"] - e["kper"] >= e["K"] // 16:
                feats.add("empty slice")
            if e["ksplit"] > 1 and any((ks * e["kper"] * 16) % e["cin"] for ks in range(1, e["ksplit"]) if ks * e["kper"] * 16 < e["K"]):
                feats.add("slice starts mid-tap")
        elif e["type"] == "ln":
            tokens.append("n4" if ln_float4(e["N"]) else "n1")
            feats |= {tokens[-1], "ln:lds" if in_lds(e["src"]) else "ln:hbm"}
        elif e["type"] == "attn":
            t = attn_tiles(T, e["hd"])
            tokens.append((f"a{t}" if t else "aa") + f"d{e['hd']}")
            feats |= {f"a{t}" if t else "aa", f"d{e['hd']}"}
        elif e["type"] == "pool":
            tokens.append("p")
            feats.add("p")
        else:
            tokens.append("c")
            feats |= {"c", "c:stage" if isinstance(e["dst"], tuple) and e["dst"][0] == "stage" else "c:concat"}
    lds = first_fit_peak([dict(e, scratch=(split_scratch(T, e["N"], e["mb"], e["ksplit"]) + 255) & ~255 if e["type"] == "gemm" else 0) for e in tab],
                         {d: T * (ld[d] + 4) * 4 for d in {e["dst"] for e in tab} if in_lds(d)}) if lds_on else scratch
    if any("off" in e and e["type"] != "copy" for e in tab):
        feats.add("c:elided")
    name = None if c.overflow else detail_name(c.n, T, tokens)
    return Plan(name, tokens, tab, lds, feats)


# ------------------------------------------------------------------------------------------------ inputs
def _rng(c, *extra):
    return np.random.default_rng([zlib.crc32(c.name.encode()), *extra])


def case_inputs(c, family, seed=0):
    """-> dict(x, w): x the graph input (normal: N(0, 1); positive: U(1, 2); large: N(0, 1) LARGE_GAIN), w the per-operator constants (the same for every
    family): products (W [n, cin, kw] / sqrt(K), bias), LayerNorm (gamma, beta)"""
    assert family in FAMILIES
    base = "normal" if family == "large" else family
    r = _rng(c, seed, FAMILIES.index(base))
    x = (r.standard_normal(c.in_shape) if base == "normal" else r.uniform(1, 2, c.in_shape)).astype(F32)
    if family == "large":
        x = (x * F32(LARGE_GAIN)).astype(F32)
    wid = widths(c)
    ws = {}
    rw = _rng(c, seed, 99)
    for i, o in enumerate(c.ops):
        s = _src(c.ops, i)
        if o.kind in ("conv", "lin"):
            K = o.kw * wid[s]
            ws[i] = ((rw.standard_normal((o.n, wid[s], o.kw)) / np.sqrt(K)).astype(F32), (0.1 * rw.standard_normal(o.n)).astype(F32))
        elif o.kind == "ln":
            ws[i] = ((1.0 + 0.1 * rw.standard_normal(wid[s])).astype(F32), (0.05 * rw.standard_normal(wid[s])).astype(F32))
    return dict(x=x, w=ws)


def poisoned(c, x):
    """the input with one NaN: sample 1, token c.poison[0], channel c.poison[1]"""
    t0, ch = c.poison
    x = x.copy()
    if c.input == "tok":
        x[1, t0, ch] = np.nan
    else:
        assert c.input == "map"
        x[1, ch, 0, t0] = np.nan
    return x


# ------------------------------------------------------------------------------------------------ the reference
EDITS = ("last key", "key T", "k step", "clamp pad", "tap shift", "res before act", "ln 256", "pool div", "pool sample")


def act_ref(a, kind, alpha=0.2, beta=0.5):
    one = a.dtype.type(1)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind is None:
            return a
        if kind == "relu":
            return np.maximum(a, 0)
        if kind == "hswish":
            return a * np.clip(a * a.dtype.type(1.0 / 6.0) + a.dtype.type(0.5), 0, 1)
        if kind == "hsigmoid":
            return np.clip(a * a.dtype.type(alpha) + a.dtype.type(beta), 0, 1)
        if kind == "sigmoid":
            return one / (one + np.exp(-a))
        if kind == "swish":
            return a / (one + np.exp(-a))
    raise ValueError(kind)


def touches(c, edit):
    """does the wrong edit change anything this case computes"""
    p = plan(c)
    gem = [e for e in p.table if e["type"] == "gemm"]
    if edit in ("last key", "key T"):
        return any(o.kind == "attn" for o in c.ops) and c.T > 1          # (T = 1: the clamped row IS the one key, twice the same key changes nothing)
    if edit == "k step":
        return bool(gem)
    if edit in ("clamp pad", "tap shift"):
        return any(o.kw > 1 and o.kind == "conv" for o in c.ops) and c.T > 1
    if edit == "res before act":
        return any(e["res"] is not None and e["act"] for e in gem)
    if edit == "ln 256":
        return any(e["type"] == "ln" and e["N"] > 256 for e in p.table)
    if edit == "pool div":
        return any(o.kind == "pool" and (o.kh * o.kw) % 6 for o in c.ops)
    if edit == "pool sample":
        return any(o.kind == "pool" for o in c.ops)
    raise ValueError(edit)


def ref(c, inp, dtype="float64", edit=None, x=None, stats=None):
    """the run in `dtype` -> the last operator's output as tokens [n, T, C].  x: another input in inp['x']'s place.  stats: a dict that receives the largest
    |attention score|.  edit: one of EDITS -- the last key left out of the soft-max; key T (the clamped last row) let in; the last 16-wide K step of the
    first K slice of the run's last product dropped; a convolution's zero padding read as the clamped edge row; the tap offset shifted by one (pad taken
    as pad - 1); the residual added before the activation; the LayerNorm variance over the first 256 columns when C > 256; the pool divided by the
    window padded to a multiple of 6; sample 1 reading sample 0's pool rows."""
    dt = np.dtype(dtype)
    x = np.asarray(inp["x"] if x is None else x)
    if c.input == "tok":
        cur = x.astype(dt)
    elif c.input == "map":
        cur = x[:, :, 0, :].transpose(0, 2, 1).astype(dt)
    else:
        cur = None
    vals = {-1: cur}
    last_gemm = max((i for i, o in enumerate(c.ops) if o.kind in ("conv", "lin")), default=-1)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, o in enumerate(c.ops):
            s = _src(c.ops, i)
            if o.kind == "pool":
                m = x.astype(dt)                                              # [n, C, kh, W]
                if edit == "pool sample":
                    m = m.copy()
                    m[1] = m[0]
                win = o.kh * o.kw
                div = dt.type(-(-win // 6) * 6 if edit == "pool div" else win)
                acc = np.zeros((c.n, c.T, c.c), dt)
                for a in range(o.kh):                                         # pool2d_kernel's order: rows outside, columns inside, one division
                    for b in range(o.kw):
                        acc = acc + m[:, :, a, b:b + o.kw * c.T:o.kw].transpose(0, 2, 1)
                y = acc / div
            elif o.kind in ("conv", "lin"):
                W, b = inp["w"][i]
                W = W.astype(dt)
                a = vals[s]
                n, T, cin = a.shape
                pl = o.pl - 1 if (edit == "tap shift" and o.kw > 1) else o.pl
                pr = o.kw - 1 - o.pl + (o.pl - pl)
                ap = np.pad(a, ((0, 0), (max(pl, 0), pr), (0, 0)), mode="edge" if (edit == "clamp pad" and o.kw > 1) else "constant")
                if pl < 0:
                    ap = ap[:, -pl:]
                y = np.broadcast_to(b.astype(dt), (n, T, o.n)).copy()
                for tap in range(o.kw):
                    Wt = W[:, :, tap].T                                       # [cin, n]
                    if edit == "k step" and i == last_gemm:
                        _, ks, kper = mb_ksplit(T, o.n, o.kw * cin)
                        kb = min(kper, o.kw * cin // 16) - 1                  # the K index is tap * cin + channel
                        lo = kb * 16 - tap * cin
                        if 0 <= lo < cin:
                            Wt = Wt.copy()
                            Wt[lo:lo + 16] = 0
                    y = y + ap[:, tap:tap + T] @ Wt
                r = vals[o.res] if o.res is not None else None
                if edit == "res before act" and r is not None:
                    y = act_ref(y + r, o.act, o.alpha, o.beta)
                else:
                    y = act_ref(y, o.act, o.alpha, o.beta)
                    if r is not None:
                        y = y + r
            elif o.kind == "ln":
                g, b = inp["w"][i]
                a = vals[s]
                C = a.shape[-1]
                mean = a.mean(-1, keepdims=True, dtype=dt)
                d = a - mean
                if edit == "ln 256" and C > 256:
                    var = (d[..., :256] * d[..., :256]).sum(-1, keepdims=True, dtype=dt) / dt.type(C)
                else:
                    var = (d * d).mean(-1, keepdims=True, dtype=dt)
                y = d / np.sqrt(var + dt.type(o.eps)) * g.astype(dt)
                if o.affine == "gb":
                    y = y + b.astype(dt)
            elif o.kind == "attn":
                a = vals[s]
                n, T, _ = a.shape
                dim = o.heads * o.hd
                q, k, v = (a[..., j * dim:(j + 1) * dim].reshape(n, T, o.heads, o.hd).transpose(0, 2, 1, 3) for j in range(3))
                if edit == "key T":
                    k, v = np.concatenate([k, k[:, :, -1:]], 2), np.concatenate([v, v[:, :, -1:]], 2)
                if edit == "last key" and T > 1:
                    k, v = k[:, :, :-1], v[:, :, :-1]
                scale = dt.type(o.hd ** -0.5 if o.scale is None else o.scale)
                sc = (q * scale) @ k.transpose(0, 1, 3, 2)
                if stats is not None:
                    stats["score"] = max(stats.get("score", 0.0), float(np.nanmax(np.abs(sc))))
                sc = sc - sc.max(-1, keepdims=True)
                p = np.exp(sc)
                p = p / p.sum(-1, keepdims=True, dtype=dt)
                y = (p @ v).transpose(0, 2, 1, 3).reshape(n, T, dim)
            elif o.kind == "cat":
                y = np.concatenate([vals[j] for j in o.cat], -1)
            else:
                raise ValueError(o.kind)
            vals[i] = y.astype(dt)
    out = vals[len(c.ops) - 1]
    assert out.shape == (c.n, c.T, widths(c)[len(c.ops) - 1]), (c.name, out.shape)
    return out


def bundle(c, inp):
    """x6_cases.fused_bundle of the case: dict(f64, scale, noise, tol), tol = 4 max |f32 numpy - f64| (absolute)"""
    return x6_cases.fused_bundle(lambda dt: ref(c, inp, dt))


# ------------------------------------------------------------------------------------------------ graphs
def _act_node(g, t, o):
    if o.act is None:
        return t
    if o.act == "relu":
        return g.op("Relu", [t])
    if o.act == "hswish":
        return g.op("HardSwish", [t])
    if o.act == "hsigmoid":
        return g.op("HardSigmoid", [t], alpha=float(o.alpha), beta=float(o.beta))
    if o.act == "sigmoid":
        return g.op("Sigmoid", [t])
    if o.act == "swish":
        return g.op("Mul", [t, g.op("Sigmoid", [t])])
    raise ValueError(o.act)


def model(c, inp):
    """the case's graph: input x, one output -- the run's last tensor, raw, as tokens [n, T, C] (behind a convolution or a concat: the Squeeze / Transpose
    view of the map, as models.build_rec leaves its neck; a map output would be converted by a launch behind the run, inside the run's last node, and the
    planner then keeps what that node reads in the arena).  -> model bytes"""
    g = GraphBuilder("chain")
    g.add_input("x", list(c.in_shape))
    i64 = lambda v, nm: g.init(np.array(v, np.int64), nm)
    have = {(-1, c.input if c.input != "pool" else "raw"): "x"}
    wid = widths(c)

    def get(j, layout):
        """operator j's output in the layout asked for, converted as models.build_rec converts (views: no launch)"""
        if (j, layout) in have:
            return have[(j, layout)]
        if layout == "tok":
            t = g.op("Transpose", [g.op("Squeeze", [have[(j, "map")], i64([2], "axes")])], perm=[0, 2, 1])
        else:
            t = g.op("Unsqueeze", [g.op("Transpose", [have[(j, "tok")]], perm=[0, 2, 1]), i64([2], "axes")])
        have[(j, layout)] = t
        return t

    lay = None
    for i, o in enumerate(c.ops):
        s = _src(c.ops, i)
        if o.kind == "pool":
            y, lay = g.op("AveragePool", ["x"], kernel_shape=[o.kh, o.kw], strides=[o.kh, o.kw], pads=[0, 0, 0, 0]), "map"
        elif o.kind == "conv":
            W, b = inp["w"][i]
            y = g.op("Conv", [get(s, "map"), g.init(np.ascontiguousarray(W[:, :, None, :])), g.init(b, "b")], kernel_shape=[1, o.kw], strides=[1, 1],
                     pads=[0, o.pl, 0, o.kw - 1 - o.pl], group=1, dilations=[1, 1])
            y, lay = _act_node(g, y, o), "map"
            if o.res is not None:
                y = g.op("Add", [y, get(o.res, "map")])
        elif o.kind == "lin":
            W, b = inp["w"][i]
            y = g.op("Add", [g.op("MatMul", [get(s, "tok"), g.init(np.ascontiguousarray(W[:, :, 0].T))]), g.init(b, "b")])
            y, lay = _act_node(g, y, o), "tok"
            if o.res is not None:
                y = g.op("Add", [get(o.res, "tok"), y])
        elif o.kind == "ln":
            gm, b = inp["w"][i]
            y = g.op("LayerNormalization", [get(s, "tok"), g.init(gm)] + ([g.init(b)] if o.affine == "gb" else []), axis=-1, epsilon=float(o.eps))
            lay = "tok"
        elif o.kind == "attn":
            dim = o.heads * o.hd
            qkv = g.op("Reshape", [get(s, "tok"), i64([0, -1, 3, o.heads, o.hd], "shape")])
            qkv = g.op("Transpose", [qkv], perm=[2, 0, 3, 1, 4])
            q, k, v = g.op("Split", [qkv], n_out=3, axis=0)
            ax0 = i64([0], "axes")
            q, k, v = g.op("Squeeze", [q, ax0]), g.op("Squeeze", [k, ax0]), g.op("Squeeze", [v, ax0])
            q = g.op("Mul", [q, g.init(np.array(o.hd ** -0.5 if o.scale is None else o.scale, F32), "scale")])
            att = g.op("Softmax", [g.op("MatMul", [q, g.op("Transpose", [k], perm=[0, 1, 3, 2])])], axis=-1)
            y = g.op("Transpose", [g.op("MatMul", [att, v])], perm=[0, 2, 1, 3])
            y, lay = g.op("Reshape", [y, i64([0, -1, dim], "shape")]), "tok"
        elif o.kind == "cat":
            y, lay = g.op("Concat", [get(j, "map") for j in o.cat], axis=1), "map"
        have[(i, lay)] = y
    last = len(c.ops) - 1
    g.add_output(get(last, "tok"), [c.n, c.T, wid[last]])
    return g.model()


# ------------------------------------------------------------------------------------------------ the matrix
def _qkv(dim):
    return Op("lin", 3 * dim)


def _products():
    """the (T, N, K) table of DESIGN 4.49, one run each: a 1 x 3 convolution 16 -> cin fixes the partition, the product under test (cin kw -> N) reads its
    output from LDS.  Without a residual it carries the row's activation and a LayerNorm follows; with one it has no activation (rewrite pass 4 folds an Add
    only then) and adds a second product's output, read from LDS.  PRODUCT_ROWS also holds what the planner must choose: path, ksplit, kper."""
    out = []
    for name, T, N, (cin, kw), act, res, _ in PRODUCT_ROWS:
        first = Op("conv", cin, kw=3, pl=1, act="swish")
        kind = "conv" if kw > 1 else "lin"
        if res:
            ops = (first, Op("lin", N, act="swish"), Op(kind, N, kw=kw, pl=kw // 2, src=0, res=1))
        else:
            ops = (first, Op(kind, N, kw=kw, pl=kw // 2, act=act), Op("ln"))
        out.append(Case(f"product {name} T{T} N{N} K{kw * cin}", 2, T, 16, ops, input="map"))
    return out


# (name, T, N, (cin, kw), activation, residual?, (path, ksplit, kper))
PRODUCT_ROWS = (
    ("short", 1, 16, (16, 1), None, False, ("gs", 1, 1)), ("short k2", 7, 64, (64, 1), "relu", True, ("gs", 2, 2)),
    ("short 3 taps", 17, 16, (16, 3), "hswish", False, ("gs", 1, 3)), ("lds1 k4", 16, 64, (512, 1), None, True, ("g1", 4, 8)),
    ("lds1 whole", 49, 64, (64, 1), "sigmoid", False, ("g1", 1, 4)), ("lds1 k4 last slice of 2 steps", 16, 64, (272, 1), "swish", False, ("g1", 4, 5)),
    ("short k8 two empty slices", 16, 16, (272, 1), None, True, ("gs", 8, 3)), ("lds2 whole", 64, 64, (256, 1), "hsigmoid", False, ("g2", 1, 16)),
    ("lds2 k4", 64, 16, (256, 1), None, True, ("g2", 4, 4)), ("lds3 k2", 40, 64, (192, 1), "relu", False, ("g3", 2, 6)),
    ("lds3 k8 slice of 2 steps", 48, 16, (256, 1), None, True, ("g3", 8, 2)), ("lds3 ragged group", 65, 64, (64, 1), "swish", False, ("g3", 1, 4)),
    ("lds3 ragged group k4", 65, 16, (32, 5), None, True, ("g3", 4, 3)), ("lds3 MT9", 137, 64, (64, 1), None, True, ("g3", 1, 4)),
)


def _cases():
    L = []
    # ---- products: the table, then split-K with a residual on every LDS path, taps, slices, acts
    L += _products()
    # split-K product WITH the residual in its own epilogue (after the reduction), the residual from LDS (the run's first product) or from HBM (the input)
    L.append(Case("splitk res short", 2, 7, 64, (Op("conv", 64, kw=3, pl=1), Op("lin", 64, act="swish"), Op("lin", 64, res=0)), poison=(6, 5), hbm_too=True))
    L.append(Case("splitk res lds1", 3, 15, 64, (Op("conv", 512, kw=3, pl=1, act="relu"), Op("lin", 64, res=-1), Op("ln")), hbm_too=True))
    L.append(Case("splitk res lds2", 2, 63, 16, (Op("conv", 256, kw=3, pl=1, act="hswish"), Op("lin", 16, res=-1), Op("ln"))))
    L.append(Case("splitk res lds3", 2, 40, 64, (Op("conv", 192, kw=3, pl=1), Op("lin", 64, res=-1), Op("lin", 64, act="sigmoid")), poison=(39, 0)))
    # taps: kw 2 both ways, 5; cin 32 x 3 taps split in two (the second slice starts mid-tap)
    L.append(Case("poison lds2 lds1", 2, 49, 64, (Op("conv", 64, kw=3, pl=1), Op("lin", 64, act="swish"), Op("ln")), poison=(48, 63)))
    L.append(Case("taps kw2 left", 2, 21, 32, (Op("conv", 32, kw=2, pl=1), Op("lin", 32, act="swish"), Op("ln")), poison=(0, 3)))
    L.append(Case("taps kw2 right", 2, 21, 32, (Op("conv", 32, kw=2, pl=0), Op("lin", 32, act="relu"), Op("ln")), input="map"))
    L.append(Case("taps kw5", 2, 19, 16, (Op("conv", 32, kw=5, pl=2, act="hsigmoid", alpha=0.3, beta=0.4), Op("lin", 32), Op("ln", affine="g")), hbm_too=True))
    L.append(Case("taps mid-tap slice", 2, 7, 32, (Op("lin", 32), Op("conv", 64, kw=3, pl=1), Op("lin", 64, act="sigmoid")), poison=(3, 31)))
    # ---- LayerNorm
    for C, T, aff in ((16, 1, "gb"), (64, 4, "g"), (256, 5, "gb"), (272, 21, "gb"), (384, 5, "g")):
        L.append(Case(f"ln C{C} T{T} {aff}", 2, T, C, (Op("ln", affine=aff), Op("conv", 16, kw=3, pl=1, act="swish"), Op("lin", C), Op("ln", affine=aff)),
                      poison=(T - 1, C - 1) if C == 272 else None, hbm_too=C in (64, 272)))
    L.append(Case("ln C64 T67", 2, 67, 64, (Op("ln"), Op("conv", 64, kw=3, pl=1), Op("ln", affine="g")), input="map"))
    # ---- attention: every head size, every tile count, the any-T form; `large` where the run reads the input straight into the QKV product
    for hd, heads, T in ((4, 4, 1), (8, 2, 16), (12, 4, 17), (16, 1, 32), (16, 4, 33), (8, 8, 48), (4, 4, 49), (16, 2, 64), (12, 4, 65), (16, 1, 100)):
        dim = heads * hd
        sc = 0.3 if (hd, T) == (8, 16) else None
        L.append(Case(f"attn hd{hd} h{heads} T{T}", 9 if T == 17 else 2, T, dim, (_qkv(dim), Op("attn", heads=heads, hd=hd, scale=sc), Op("lin", dim, res=-1)),
                      families=FAMILIES, poison=(T // 2, 1) if T in (33, 65) else None, hbm_too=T in (33, 100)))
    # ---- pool
    for kh, kw, C, odd, n in ((6, 2, 32, 0, 2), (4, 2, 16, 1, 3), (5, 3, 48, 2, 2), (8, 8, 16, 0, 2)):
        L.append(Case(f"pool {kh}x{kw} C{C}", n, 13, C, (Op("pool", kh=kh, kw=kw), Op("conv", 32, kw=3, pl=1, act="swish"), Op("lin", 32)), input="pool", odd=odd))
    L.append(Case("pool 5x3 C20", 3, 9, 20, (Op("pool", kh=5, kw=3), Op("ln"), Op("ln", affine="g")), input="pool", odd=1))
    # ---- concat: an elided copy (the producer is read by nothing else) at a column offset, a real copy (the producer is a residual too)
    L.append(Case("concat elided and real", 2, 21, 32, (Op("conv", 32, kw=3, pl=1, act="swish"), Op("conv", 48), Op("conv", 32, src=0, res=0), Op("cat", cat=(0, 1)),
                                                        Op("conv", 32, kw=1, src=3), Op("cat", cat=(2, 4))), input="map", hbm_too=True))
    # ---- the tiny recognizer's neck, restated at T = 40: pool, 1x3, 1x1, two blocks, LayerNorm, 1x1, concat, 1x3, 1x1
    blk = lambda z: (Op("ln", src=z), _qkv(64), Op("attn", heads=4, hd=16), Op("lin", 64, res=z), Op("ln"), Op("lin", 128, act="swish"), Op("lin", 64, res=z + 4))
    neck = (Op("pool", kh=6, kw=2), Op("conv", 32, kw=3, pl=1, act="swish"), Op("conv", 64, act="swish")) + blk(2) + blk(9) + \
           (Op("ln"), Op("conv", 256, act="swish"), Op("cat", cat=(0, 18)), Op("conv", 32, kw=3, pl=1, act="swish"), Op("conv", 64, act="swish"))
    L.append(Case("neck tiny T40", 2, 40, 256, neck, input="pool"))
    # ---- tensors beyond the LDS budget: three 64-channel tensors of 512 tokens are alive together, the planner sends the largest back to the arena
    L.append(Case("overflow T512", 2, 512, 64, (Op("conv", 64, kw=3, pl=1), Op("conv", 64, act="swish"), Op("conv", 64, res=0)), input="map", overflow=True,
                  families=("normal",)))
    return tuple(L)


CASES = _cases()

# advertised by the kernel, reachable from no graph the engine accepts -> the reason
NOT_REACHED = {
    "res+act": "a product with a residual AND an activation (ch_epilogue: act, then + res): rewrite pass 3 folds the activation first, and pass 4 folds an Add "
               "only into a Linear / Conv without activation -- the Add stays a launch of its own and ends the run",
}


def features():
    """every feature the matrix must reach (tests/test_chain_cases_cpu.py: reached by a case, or in NOT_REACHED)"""
    f = {"gs", "g1", "g2", "g3", "gh", "n4", "n1", "a1", "a2", "a3", "a4", "aa", "d4", "d8", "d12", "d16", "p", "c", "c:stage", "c:concat", "c:elided",
         "res", "res:lds", "res:hbm", "res+act", "empty slice", "slice starts mid-tap", "ln:lds", "ln:hbm"}
    f |= {p + s for p in ("gs", "g1", "g2", "g3", "gh") for s in ("+split", "+whole")}
    f |= {p + "+res" for p in ("gs", "g1", "g2", "g3", "gh")}
    f |= {"act:" + str(a) for a in ACT_LETTER} | {"taps:1", "taps:2", "taps:3", "taps:5"}
    return f


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def jobs_of(c, group):
    """the (family | 'poison') runs of a case in a group: 'default', 'hbm' (OAR_CHAIN_LDS=0), 'unfused' (the control: poison cases only)"""
    if group == "default":
        return list(c.families) + (["poison"] if c.poison else [])
    if group == "hbm":
        return ["normal"] + (["poison"] if c.poison else []) if c.hbm_too else []
    return ["normal", "poison"] if c.poison else []


GROUPS = {"default": (), "hbm": ENV_HBM, "unfused": ENV_UNFUSED}
