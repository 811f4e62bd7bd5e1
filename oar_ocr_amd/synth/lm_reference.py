"""Torch-CPU reference of the decoder-only language model (vl.CausalLM / lm_decode.hip), written from the formulas, in f64 and f32; the test cases; the tolerance.

  RMSNorm        y = x * rsqrt(mean(x^2) + eps) * g
  rotary         inv_freq_i = theta^(-2 i / dh), i < dh / 2; cos / sin over dh = (freqs ‖ freqs); M-RoPE: the dh entries are split into the sections
                 mrope_section ‖ mrope_section and chunk j takes the positions of axis j mod 3; x' = x cos + rotate_half(x) sin, rotate_half(x) = (-x2 ‖ x1)
  attention      query head h uses kv head h // (heads / kv_heads); scores scaled by dh^-0.5; position p sees cache positions 0 .. p
  MLP            down(silu(gate(x)) * up(x))
  decoding       greedy argmax, lowest index first; generated token i sits at position max(position_ids) + 1 + i on all three axes

`fault` (a name from FAULTS) swaps one of these for a plausible wrong variant: the CPU tests show that each moves the logits far beyond the tolerance.
`skip_key=j` is a sensitivity variant of its own: every row at a cache position greater than j ignores key j (what an attention loop that drops one key computes); the
CPU tests show that at every boundary of the attention kernel's key loop it moves the logits of the long-cache cases far beyond the tolerance."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

FAULTS = ("rotate_interleaved", "wrong_axis", "kv_head_mod", "causal_minus_one", "silu_on_up", "eps_outside_sqrt", "positions_from_T")


@dataclass(frozen=True)
class LmCase:
    name: str
    D: int
    L: int
    heads: int
    kv_heads: int
    head_dim: int
    F: int
    vocab: int
    mrope_section: tuple
    qkv_bias: bool = False
    tie: bool = True
    eps: float = 1e-5
    theta: float = 10000.0


# the smallest shapes at which each part can still go wrong (tests/test_gpu_lm_decode.py)
CASES = {
    "A": LmCase("A", 64, 2, 4, 2, 16, 96, 97, (2, 3, 3)),
    "B": LmCase("B", 48, 2, 2, 1, 128, 80, 131, (16, 24, 24)),
    "C": LmCase("C", 40, 1, 5, 5, 8, 52, 33, (4, 0, 0), qkv_bias=True, tie=False),
    "D": LmCase("D", 1544, 1, 2, 1, 64, 1540, 64, (8, 12, 12)),
    # the branches real checkpoints take, one layer each so that an error is not diluted (G = query heads per kv head; the arithmetic the comments lean on is
    # asserted from the header's own functions in tests/test_lm_reference_cpu.py)
    "E": LmCase("E", 64, 1, 16, 2, 128, 96, 97, (16, 24, 24)),                             # G = 8: lm_attn_kernel<8>, ERNIE-4.5-0.3B's geometry
    "F": LmCase("F", 56, 1, 14, 2, 32, 96, 97, (4, 6, 6), qkv_bias=True),                  # G = 7: <4>, two chunks of heads, the second with 3
    "G": LmCase("G", 40, 1, 6, 2, 20, 52, 33, (4, 3, 3)),                                  # G = 3: <4>, one partial chunk; head size 20 leaves 3 idle lanes of 8
    "H": LmCase("H", 40, 1, 12, 1, 8, 52, 33, (4, 0, 0), qkv_bias=True, tie=False),        # G = 12: <8>, chunks of 8 and 4
    # the rows kernels' row-group loop (a workgroup of 4 waves x 2 rows takes ceil(N / 4096) groups of 8 rows): the lm-head with 3 row groups, 417 workgroups and
    # a combine over more than 256 partials, the input (K = 32) staged once
    "V": LmCase("V", 32, 1, 2, 1, 16, 48, 10007, (2, 3, 3), tie=False),
    # gate / up N = 4104: 2 row groups, the input (K = 1028: chunks of 1024 and 4 columns) staged again per group; the down projection's K = 2052 ends in a chunk of 4 too
    "W": LmCase("W", 1028, 1, 2, 1, 64, 2052, 64, (8, 12, 12)),
}
PROMPT_LENGTHS = (1, 17, 37)
TEACHER_STEPS = 20
FREE_STEPS = 24

# Long caches: two layers, so that every row's attention output feeds the second layer's keys and every key count n = 1 .. T reaches the final logits.  (case, T): a prompt of
# T positions with the image block in its middle, LONG_STEPS forced steps that cross a boundary of the attention kernel's key loop (a wave takes kpw = 64 / lanes-per-key keys
# a turn, the 8 waves `turn` = 8 kpw, and U = 4 turns are loaded together), in a cache of exactly T + LONG_STEPS positions; its step mate is a one-position prompt.
LONG_STEPS = 12
LONG_CASES = {
    "LA": (LmCase("LA", 64, 2, 16, 2, 128, 96, 97, (16, 24, 24)), 122),                    # kpw 2, turn 16, U turn 64: crosses 128
    "LB": (LmCase("LB", 48, 2, 6, 2, 80, 80, 131, (10, 15, 15)), 122),                     # head size 80: 12 idle lanes of 32; crosses 128
    "LC": (LmCase("LC", 40, 2, 7, 1, 20, 52, 33, (4, 3, 3)), 506),                         # kpw 8, turn 64, U turn 256: crosses 512
    "LD": (LmCase("LD", 64, 2, 4, 2, 16, 96, 97, (2, 3, 3)), 250),                         # case A; kpw 16, turn 128, U turn 512: crosses 256
    "LE": (LmCase("LE", 48, 2, 6, 2, 12, 80, 131, (2, 2, 2)), 250),                        # head size 12: 1 idle lane of 4; crosses 256
    "LF": (LmCase("LF", 40, 2, 5, 5, 8, 52, 33, (4, 0, 0), qkv_bias=True, tie=False), 250),   # case C with two layers; kpw 32, turn 256: crosses 256
}

# Equal maxima: case V's geometry with lm-head row v a copy of row v - d wherever (v // d) is odd, so every row is one of two identical rows d apart.
TIE_CASE = "V"

# greedy-safe (tests/test_lm_reference_cpu.py checks the margins, and for the long cases the skip_key condition; A-D keep the seeds they had)
SEEDS = {"A": 0, "B": 0, "C": 0, "D": 4, "E": 0, "F": 0, "G": 0, "H": 1, "V": 0, "W": 0, "LA": 0, "LB": 0, "LC": 2, "LD": 1, "LE": 0, "LF": 0}
# (seed 0 failed a condition on H: margin 2.7 tol; on LC, and seed 1 too: skip_key moved the logits by 14 and 12 tol only; on LD: margin 4.0 tol)
TIE_SEEDS = {}   # distance d -> seed; SEEDS[TIE_CASE] where absent


def make_lm(case: LmCase, seed: int) -> Dict[str, np.ndarray]:
    """Checkpoint-named float32 tensors.  Matrices ~ N(0, 1 / fan_in); the lm-head is scaled up so that the logits spread over a few units."""
    rng = np.random.default_rng(seed)
    D, Hd, Kd, F, V = case.D, case.heads * case.head_dim, case.kv_heads * case.head_dim, case.F, case.vocab
    w = {}

    def mat(n, k, gain=1.0):
        return (rng.standard_normal((n, k)) * (gain / np.sqrt(k))).astype(np.float32)

    w["model.embed_tokens.weight"] = rng.standard_normal((V, D)).astype(np.float32)
    for l in range(case.L):
        p = f"model.layers.{l}."
        w[p + "input_layernorm.weight"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        w[p + "post_attention_layernorm.weight"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        w[p + "self_attn.q_proj.weight"] = mat(Hd, D, 2.0)
        w[p + "self_attn.k_proj.weight"] = mat(Kd, D, 2.0)
        w[p + "self_attn.v_proj.weight"] = mat(Kd, D)
        w[p + "self_attn.o_proj.weight"] = mat(D, Hd)
        if case.qkv_bias:
            w[p + "self_attn.q_proj.bias"] = (0.3 * rng.standard_normal(Hd)).astype(np.float32)
            w[p + "self_attn.k_proj.bias"] = (0.3 * rng.standard_normal(Kd)).astype(np.float32)
            w[p + "self_attn.v_proj.bias"] = (0.3 * rng.standard_normal(Kd)).astype(np.float32)
        w[p + "mlp.gate_proj.weight"] = mat(F, D, 1.5)
        w[p + "mlp.up_proj.weight"] = mat(F, D, 1.5)
        w[p + "mlp.down_proj.weight"] = mat(D, F)
    w["model.norm.weight"] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    if case.tie:
        w["model.embed_tokens.weight"] *= np.float32(3.0 / np.sqrt(D))   # (tied: logits = h . E[v] with |h| ~ sqrt(D))
    else:
        w["lm_head.weight"] = mat(V, D, 3.0)
        w["model.embed_tokens.weight"] *= np.float32(0.003)   # (untied: mean(x^2) of a token row ~ eps, so where eps sits in the RMSNorm matters)
    return w


def to_bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (round to nearest even) as uint16."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


def make_positions(T: int) -> np.ndarray:
    """[3, T] position ids with a 3 x 4 image block in Qwen2-VL's scheme in the middle of the prompt (T >= 13): text tokens advance all three axes together;
    the block's 12 tokens share one t, and take h = start + row, w = start + column; the text after it continues from max + 1 = start + 4, so max + 1 < T."""
    if T < 13:
        return np.tile(np.arange(T, dtype=np.int32), (3, 1))
    pre = (T - 12) // 2
    cols = []
    for i in range(pre):
        cols.append((i, i, i))
    for r in range(3):
        for c in range(4):
            cols.append((pre, pre + r, pre + c))
    for i in range(T - 12 - pre):
        cols.append((pre + 4 + i,) * 3)
    return np.asarray(cols, np.int32).T.copy()


def make_prompt(case: LmCase, weights, T: int, seed: int):
    """(inputs_embeds [T, D] float32, position_ids [3, T], ids [T]): embedding rows of random ids, the image block replaced by random vectors."""
    rng = np.random.default_rng(1000 + seed * 31 + T)
    ids = rng.integers(0, case.vocab, T).astype(np.int32)
    emb = weights["model.embed_tokens.weight"][ids].astype(np.float32).copy()
    pos = make_positions(T)
    if T >= 13:
        pre = (T - 12) // 2
        emb[pre:pre + 12] = rng.standard_normal((12, case.D)).astype(np.float32)
    return emb, pos, ids


class RefLM:
    """The cached, step-by-step forward."""

    def __init__(self, case: LmCase, weights: Dict[str, np.ndarray], dtype=torch.float64, fault: Optional[str] = None, skip_key: Optional[int] = None):
        assert fault is None or fault in FAULTS, fault
        self.c, self.dt, self.fault, self.skip_key = case, dtype, fault, skip_key
        self.w = {k: torch.from_numpy(np.asarray(v, np.float32)).to(dtype) for k, v in weights.items()}
        dh = case.head_dim
        i = torch.arange(dh // 2, dtype=dtype)
        self.inv_freq = torch.tensor(case.theta, dtype=dtype) ** (-2.0 * i / dh)

    # ---- pieces
    def rms(self, x, g):
        ms = (x * x).mean(-1, keepdim=True)
        if self.fault == "eps_outside_sqrt":
            return x / (torch.sqrt(ms) + self.c.eps) * g
        return x * torch.rsqrt(ms + self.c.eps) * g

    def cos_sin(self, pos3):
        """pos3 [3, T] -> cos, sin [T, dh] after the M-RoPE selection."""
        dh = self.c.head_dim
        ang = torch.einsum("at,f->atf", pos3.to(self.dt), self.inv_freq)       # [3, T, dh / 2]
        ang = torch.cat([ang, ang], dim=-1)                                    # [3, T, dh]
        sections = list(self.c.mrope_section) * 2
        chunks, off = [], 0
        for j, n in enumerate(sections):
            axis = (j + 1) % 3 if self.fault == "wrong_axis" else j % 3
            chunks.append(ang[axis, :, off:off + n])
            off += n
        sel = torch.cat(chunks, dim=-1)
        return torch.cos(sel), torch.sin(sel)

    def rotate_half(self, x):
        if self.fault == "rotate_interleaved":
            x1, x2 = x[..., 0::2], x[..., 1::2]
            return torch.stack([-x2, x1], dim=-1).flatten(-2)
        h = x.shape[-1] // 2
        return torch.cat([-x[..., h:], x[..., :h]], dim=-1)

    def rope(self, x, cos, sin):
        """x [T, heads, dh]"""
        return x * cos[:, None, :] + self.rotate_half(x) * sin[:, None, :]

    def mlp(self, x, p):
        g = torch.einsum("td,fd->tf", x, self.w[p + "mlp.gate_proj.weight"])
        u = torch.einsum("td,fd->tf", x, self.w[p + "mlp.up_proj.weight"])
        a = torch.nn.functional.silu(u) * g if self.fault == "silu_on_up" else torch.nn.functional.silu(g) * u
        return torch.einsum("tf,df->td", a, self.w[p + "mlp.down_proj.weight"])

    # ---- one chunk of new positions against the cache
    def forward_chunk(self, x, pos3, cache):
        """x [T, D] new rows at cache positions P .. P + T - 1 (P = len of the cache); returns the hidden rows after the final norm.  cache: per layer [K, V]
        of [P, kv_heads, dh], extended in place."""
        c = self.c
        H, KVH, dh = c.heads, c.kv_heads, c.head_dim
        G = H // KVH
        cos, sin = self.cos_sin(pos3)
        T = x.shape[0]
        for l in range(c.L):
            p = f"model.layers.{l}."
            xn = self.rms(x, self.w[p + "input_layernorm.weight"])
            q = torch.einsum("td,nd->tn", xn, self.w[p + "self_attn.q_proj.weight"])
            k = torch.einsum("td,nd->tn", xn, self.w[p + "self_attn.k_proj.weight"])
            v = torch.einsum("td,nd->tn", xn, self.w[p + "self_attn.v_proj.weight"])
            if c.qkv_bias:
                q, k, v = q + self.w[p + "self_attn.q_proj.bias"], k + self.w[p + "self_attn.k_proj.bias"], v + self.w[p + "self_attn.v_proj.bias"]
            q = self.rope(q.reshape(T, H, dh), cos, sin)
            k = self.rope(k.reshape(T, KVH, dh), cos, sin)
            v = v.reshape(T, KVH, dh)
            if cache[l] is None:
                cache[l] = [k, v]
            else:
                cache[l] = [torch.cat([cache[l][0], k]), torch.cat([cache[l][1], v])]
            K, V = cache[l]
            P = K.shape[0] - T
            kv_of = [(h % KVH) if self.fault == "kv_head_mod" else (h // G) for h in range(H)]
            Kh, Vh = K[:, kv_of, :], V[:, kv_of, :]                                    # [S, H, dh]
            s = torch.einsum("thd,shd->hts", q, Kh) * dh ** -0.5
            bound = torch.arange(T)[:, None] + P + (0 if self.fault == "causal_minus_one" else 1)   # row t sees positions < P + t + 1
            if self.fault == "causal_minus_one":
                bound = torch.clamp(bound, min=1)
            mask = torch.arange(K.shape[0])[None, :] < bound
            if self.skip_key is not None:   # rows at positions beyond the key do not see it
                mask = mask & ~((torch.arange(K.shape[0])[None, :] == self.skip_key) & (torch.arange(T)[:, None] + P > self.skip_key))
            s = s.masked_fill(~mask[None], float("-inf"))
            a = torch.softmax(s, dim=-1)
            o = torch.einsum("hts,shd->thd", a, Vh).reshape(T, H * dh)
            x = x + torch.einsum("tn,dn->td", o, self.w[p + "self_attn.o_proj.weight"])
            x = x + self.mlp(self.rms(x, self.w[p + "post_attention_layernorm.weight"]), p)
        return self.rms(x, self.w["model.norm.weight"])

    def logits_of(self, hidden):
        w = self.w["model.embed_tokens.weight"] if self.c.tie else self.w["lm_head.weight"]
        return torch.einsum("td,vd->tv", hidden, w)

    def embed(self, ids):
        return self.w["model.embed_tokens.weight"][torch.as_tensor(np.asarray(ids, np.int64))]

    def generate(self, inputs_embeds=None, input_ids=None, position_ids=None, max_new_tokens=16, eos_token_id=None, forced_tokens=None, canon=None):
        """-> (tokens [max_new] int64 numpy, logits [max_new, V] torch): greedy, or fed with forced_tokens where given.  canon [V]: the lowest index among the rows
        identical to row v; the winner is reported as canon[winner], whichever of its equals the matrix product happened to favour."""
        x = self.embed(input_ids) if inputs_embeds is None else torch.from_numpy(np.asarray(inputs_embeds, np.float32)).to(self.dt)
        T = x.shape[0]
        pos3 = torch.arange(T)[None, :].repeat(3, 1) if position_ids is None else torch.as_tensor(np.asarray(position_ids, np.int64))
        nxt = T if self.fault == "positions_from_T" else int(pos3.max()) + 1
        cache = [None] * self.c.L
        h = self.forward_chunk(x, pos3, cache)[-1:]
        toks, logs, done = [], [], False
        for i in range(max_new_tokens):
            lg = self.logits_of(h)[0]
            logs.append(lg)
            tok = int(eos_token_id) if done else int((lg == lg.max()).nonzero()[0, 0])     # the lowest index among equal maxima
            if canon is not None and not done:
                tok = int(canon[tok])
            toks.append(tok)
            if eos_token_id is not None and tok == eos_token_id:
                done = True
            if i + 1 == max_new_tokens:
                break
            feed = tok
            if forced_tokens is not None and int(forced_tokens[i]) >= 0:
                feed = int(forced_tokens[i])
            p = torch.full((3, 1), nxt + i, dtype=torch.int64)
            h = self.forward_chunk(self.embed([feed]), p, cache)
        return np.asarray(toks, np.int64), torch.stack(logs)


_REFS: dict = {}


def _reference(case: LmCase, weights, seed: int, lengths, free: int, teacher: int, canon=None):
    prompts = [make_prompt(case, weights, T, seed) for T in lengths]
    r64, r32 = RefLM(case, weights, torch.float64), RefLM(case, weights, torch.float32)
    noise, runs = 0.0, []
    for emb, pos, _ in prompts:
        t64, l64 = r64.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=free, canon=canon)
        _, l32 = r32.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=teacher, forced_tokens=t64)
        noise = max(noise, float((l32.double() - l64[:teacher]).abs().max()))
        runs.append((t64, l64))
    return dict(case=case, weights=weights, prompts=prompts, runs=runs, noise=noise, tol=max(16.0 * noise, 2.0 ** -19))


def reference_for(name: str):
    """Computed once per process and shared: the case's weights, its three prompts, the f64 greedy run of FREE_STEPS tokens per prompt (its first TEACHER_STEPS
    steps are the teacher-forced run), and noise / tol over the teacher-forced steps."""
    if name not in _REFS:
        case = CASES[name]
        _REFS[name] = _reference(case, make_lm(case, SEEDS[name]), SEEDS[name], PROMPT_LENGTHS, FREE_STEPS, TEACHER_STEPS)
    return _REFS[name]


def long_reference_for(name: str):
    """The same for a long-cache case: prompts[0] / runs[0] the sequence of T positions, prompts[1] / runs[1] its one-position step mate; LONG_STEPS greedy f64 tokens each."""
    if name not in _REFS:
        case, T = LONG_CASES[name]
        _REFS[name] = dict(_reference(case, make_lm(case, SEEDS[name]), SEEDS[name], (T, 1), LONG_STEPS, LONG_STEPS), T=T)
    return _REFS[name]


_GEOMETRY: dict = {}
_GEOMETRY_PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "lm_decode.h"
int main(int argc, char** argv) {
    using namespace oar::k;
    std::printf("{\"threads\": %d, \"waves\": %d, \"rows_per_wave\": %d, \"kc\": %d, \"attn_waves\": %d, \"unroll\": %d, \"max_gt\": %d, \"kpw\": {", kLmThreads, kLmWaves, kLmR, kLmKC,
                kLmAttnWaves, kLmAttnUnroll, kLmMaxGT);
    for (int dh = kLmMinDh; dh <= kLmMaxDh; dh += 4) std::printf("%s\"%d\": %d", dh > kLmMinDh ? ", " : "", dh, lm_attn_keys_per_wave(dh));
    std::printf("}, \"rows\": {");
    for (int i = 1; i < argc; ++i) { const int n = std::atoi(argv[i]); std::printf("%s\"%d\": [%d, %d]", i > 1 ? ", " : "", n, lm_groups_for(n), lm_wgs_for(n)); }
    std::printf("}}\n");
    return 0;
}
"""


def kernel_geometry(rows: Sequence[int] = ()) -> dict:
    """The loop geometry of lm_decode.hip from its own header (csrc/lm_decode.h, compiled for the host): waves and rows per wave of the rows kernels, the staging chunk `kc`,
    the attention kernel's waves, unroll and keys per wave turn `kpw[dh]`, and for every N of `rows` the (row groups per workgroup, workgroups) of an [N][K] matrix."""
    import json
    import shutil
    import subprocess
    import tempfile
    from pathlib import Path
    key = tuple(int(n) for n in rows)
    if key not in _GEOMETRY:
        csrc = Path(__file__).resolve().parents[1] / "csrc"
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        with tempfile.TemporaryDirectory() as d:
            (Path(d) / "geometry.cc").write_text(_GEOMETRY_PROG)
            subprocess.run([cxx, "-std=c++17", f"-I{csrc}", str(Path(d) / "geometry.cc"), "-o", str(Path(d) / "geometry")], check=True, capture_output=True, timeout=300)
            g = json.loads(subprocess.run([str(Path(d) / "geometry")] + [str(n) for n in key], check=True, capture_output=True, text=True, timeout=60).stdout)
        g["kpw"] = {int(k): v for k, v in g["kpw"].items()}
        g["rows"] = {int(k): tuple(v) for k, v in g["rows"].items()}
        _GEOMETRY[key] = g
    return _GEOMETRY[key]


def attn_boundaries(head_dim: int, T: int):
    """(kpw, turn, U turn) of the attention kernel at this head size, and the key indices b - 1 and b for b in kpw, turn, U turn and its multiples below T, and T - 1."""
    g = kernel_geometry()
    kpw = g["kpw"][head_dim]
    turn = g["attn_waves"] * kpw
    ut = g["unroll"] * turn
    js = {T - 1}
    for b in [kpw, turn] + list(range(ut, T, ut)):
        if b < T:
            js |= {b - 1, b}
    return (kpw, turn, ut), sorted(js)


TIE_PLACES = ("one_wave", "next_wave", "next_row_group", "next_workgroup", "far_workgroup", "d16", "d48", "d9984")


def tie_distances() -> Dict[str, int]:
    """Where the two identical lm-head rows of a pair sit, as a distance d between them, from the rows kernel's geometry at TIE_CASE's vocabulary: a wave owns
    rows_per_wave adjacent rows, a row group is waves x rows_per_wave rows, a workgroup takes `groups` row groups in turn; `far` is half the grid, so that nearly every
    row has its copy and lm_combine meets the pair in two different threads.  16, 48 and 9984 are plain distances (two row groups; two workgroups; all but the last)."""
    V = CASES[TIE_CASE].vocab
    g = kernel_geometry((V,))
    per = g["waves"] * g["rows_per_wave"]
    groups, wgs = g["rows"][V]
    return {"one_wave": 1, "next_wave": g["rows_per_wave"], "next_row_group": per, "next_workgroup": groups * per, "far_workgroup": (wgs // 2) * groups * per,
            "d16": 16, "d48": 48, "d9984": 9984}


def tie_canon(V: int, d: int) -> np.ndarray:
    """canon[v]: the lowest index among the lm-head rows identical to row v when row v copies row v - d wherever (v // d) is odd."""
    v = np.arange(V)
    return np.where((v // d) % 2 == 1, v - d, v)


def tie_reference_for(d: int):
    """Case TIE_CASE with paired lm-head rows d apart: the usual three prompts, TEACHER_STEPS steps forced to the lowest index among the rows identical to the f64 winner's
    (runs[i][0]; computed from the rows' identity, not from a tie of f64 logits, which a BLAS may break either way).  `canon` as tie_canon."""
    key = ("tie", d)
    if key not in _REFS:
        case, seed = CASES[TIE_CASE], TIE_SEEDS.get(d, SEEDS[TIE_CASE])
        weights = make_lm(case, seed)
        canon = tie_canon(case.vocab, d)
        weights["lm_head.weight"] = np.ascontiguousarray(weights["lm_head.weight"][canon])
        _REFS[key] = dict(_reference(case, weights, seed, PROMPT_LENGTHS, TEACHER_STEPS, TEACHER_STEPS, canon=canon), canon=canon)
    return _REFS[key]


def all_end_choice(ref):
    """(i, j, eos, n_j) for the test in which every sequence ends early: eos is the very first f64 token of prompt i and prompt j's n_j-th (n_j < FREE_STEPS), its first
    occurrence there; None where the runs hold no such pair."""
    for i in reversed(range(len(ref["runs"]))):
        eos = int(ref["runs"][i][0][0])
        for j in reversed(range(len(ref["runs"]))):
            hit = np.flatnonzero(ref["runs"][j][0][:FREE_STEPS - 1] == eos)
            if j != i and len(hit):
                return i, j, eos, int(hit[0]) + 1
    return None


def greedy_margins(logits64: torch.Tensor) -> np.ndarray:
    """best - second best logit per step."""
    top = torch.topk(logits64, 2, dim=-1).values
    return (top[:, 0] - top[:, 1]).numpy()


def pair_margins(logits64: torch.Tensor, canon: np.ndarray) -> np.ndarray:
    """best logit - the best among the rows that are no copy of the winner's row, per step."""
    c = torch.from_numpy(np.asarray(canon, np.int64))
    out = []
    for lg in logits64:
        w = int(torch.argmax(lg))
        out.append(float(lg[w] - lg[c != c[w]].max()))
    return np.asarray(out)
