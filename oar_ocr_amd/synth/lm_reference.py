"""Torch-CPU reference of the decoder-only language model (vl.CausalLM / lm_decode.hip), written from the formulas, in f64 and f32; the test cases; the tolerance.

  RMSNorm        y = x * rsqrt(mean(x^2) + eps) * g
  rotary         inv_freq_i = theta^(-2 i / dh), i < dh / 2; cos / sin over dh = (freqs ‖ freqs); M-RoPE: the dh entries are split into the sections
                 mrope_section ‖ mrope_section and chunk j takes the positions of axis j mod 3; x' = x cos + rotate_half(x) sin, rotate_half(x) = (-x2 ‖ x1)
  attention      query head h uses kv head h // (heads / kv_heads); scores scaled by dh^-0.5; position p sees cache positions 0 .. p
  MLP            down(silu(gate(x)) * up(x))
  decoding       greedy argmax, lowest index first; generated token i sits at position max(position_ids) + 1 + i on all three axes

`fault` (a name from FAULTS) swaps one of these for a plausible wrong variant: the CPU tests show that each moves the logits far beyond the tolerance."""
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
}
PROMPT_LENGTHS = (1, 17, 37)
TEACHER_STEPS = 20
FREE_STEPS = 24
SEEDS = {"A": 0, "B": 0, "C": 0, "D": 4}   # greedy-safe (tests/test_lm_reference_cpu.py checks the margins)


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

    def __init__(self, case: LmCase, weights: Dict[str, np.ndarray], dtype=torch.float64, fault: Optional[str] = None):
        assert fault is None or fault in FAULTS, fault
        self.c, self.dt, self.fault = case, dtype, fault
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

    def generate(self, inputs_embeds=None, input_ids=None, position_ids=None, max_new_tokens=16, eos_token_id=None, forced_tokens=None):
        """-> (tokens [max_new] int64 numpy, logits [max_new, V] torch): greedy, or fed with forced_tokens where given."""
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


def reference_for(name: str):
    """Computed once per process and shared: the case's weights, its three prompts, the f64 greedy run of FREE_STEPS tokens per prompt (its first TEACHER_STEPS
    steps are the teacher-forced run), and noise / tol over the teacher-forced steps."""
    if name not in _REFS:
        case = CASES[name]
        weights = make_lm(case, SEEDS[name])
        prompts = [make_prompt(case, weights, T, SEEDS[name]) for T in PROMPT_LENGTHS]
        r64, r32 = RefLM(case, weights, torch.float64), RefLM(case, weights, torch.float32)
        noise, runs = 0.0, []
        for emb, pos, _ in prompts:
            t64, l64 = r64.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=FREE_STEPS)
            _, l32 = r32.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=TEACHER_STEPS, forced_tokens=t64)
            noise = max(noise, float((l32.double() - l64[:TEACHER_STEPS]).abs().max()))
            runs.append((t64, l64))
        _REFS[name] = dict(case=case, weights=weights, prompts=prompts, runs=runs, noise=noise, tol=max(16.0 * noise, 2.0 ** -19))
    return _REFS[name]


def greedy_margins(logits64: torch.Tensor) -> np.ndarray:
    """best - second best logit per step."""
    top = torch.topk(logits64, 2, dim=-1).values
    return (top[:, 0] - top[:, 1]).numpy()
