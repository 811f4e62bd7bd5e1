"""Repetition penalty and no-repeat-ngram in front of the greedy choice (csrc/lm_logits.hip): the two processors in plain Python, written from the
rules; an f64 generate with them; the model cases with their pinned seeds; the direct cases of the select kernel.

  history     the ids the caller gives for the prompt, then every token fed back (the forced token where one is given, else the chosen one)
  penalty r   every DISTINCT id t of the history with 0 <= t < V:  x = logits[t];  logits[t] = x * r if x < 0 else x / r      (f32: one rounding each)
  ban n       n > 1 and H = len(history) >= n: for every i in 0 .. H - n with history[i : i + n - 1] == history[H - n + 1 : H] the id history[i + n - 1] is
              banned (value -inf); ids >= V take part in the comparison and are ignored as bans
  choice      penalty, then ban, then the lowest index among equal maxima; a NaN never wins; no candidate at all: token 0"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lm_reference as R

SETTINGS = ((1.3, 3), (1.0, 2), (2.0, 0))        # (repetition_penalty, no_repeat_ngram_size)
MODEL_CASES = ("A", "E", "C", "V")
BITE_CASES = ("A", "E", "C")                      # V's wide vocabulary may repeat rarely: held to the margin condition only
LENGTHS = (17, 37)                                # prompts with the image block, given as inputs_embeds with their ids as history
STEPS = 48
# pinned on the CPU: the f64 reference alone meets the margin condition (and A, E, C the bite condition) at every setting; tests/test_lm_logits_cases_cpu.py asserts it
SEEDS = {"A": 1, "E": 1, "C": 2, "V": 7}


# ------------------------------------------------------------------------------------------------ the processors
def banned_tokens(history: Sequence[int], n: int) -> set:
    """The ids (of any size) that would complete an n-gram the history already holds."""
    h = [int(v) for v in history]
    H = len(h)
    if n <= 1 or H < n:
        return set()
    tail = h[H - n + 1:]
    return {h[i + n - 1] for i in range(H - n + 1) if h[i:i + n - 1] == tail}


def process(logits: np.ndarray, history: Sequence[int], r: float, n: int) -> np.ndarray:
    """numpy f32: what the select kernel's arg-max sees."""
    x = np.array(logits, np.float32, copy=True)
    V = x.size
    seen = np.unique(np.asarray([t for t in history if 0 <= int(t) < V], np.int64))
    if seen.size and r != 1.0:
        rr = np.float32(r)
        with np.errstate(all="ignore"):
            v = x[seen]
            x[seen] = np.where(v < 0, v * rr, v / rr).astype(np.float32)
    for t in banned_tokens(history, n):
        if 0 <= t < V:
            x[t] = -np.inf
    return x


def process64(logits: torch.Tensor, history: Sequence[int], r: float, n: int) -> torch.Tensor:
    """the same on an f64 tensor"""
    x = logits.to(torch.float64).clone()
    V = x.numel()
    seen = sorted({int(t) for t in history if 0 <= int(t) < V})
    if seen and r != 1.0:
        idx = torch.as_tensor(seen)
        v = x[idx]
        x[idx] = torch.where(v < 0, v * r, v / r)
    for t in banned_tokens(history, n):
        if 0 <= t < V:
            x[t] = float("-inf")
    return x


def choose(x: np.ndarray) -> int:
    """The lowest index among equal maxima; a NaN never wins; nothing but NaNs: 0."""
    x = np.asarray(x)
    ok = ~np.isnan(x)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (x == x[ok].max()))[0])


# ------------------------------------------------------------------------------------------------ the f64 generate
def generate(ref: R.RefLM, inputs_embeds, position_ids, history, max_new_tokens, r, n, forced_tokens=None, eos_token_id=None):
    """RefLM.generate with the processors.  -> dict: tokens [max_new] (eos from the first eos on), raw [max_new, V] (torch), margin [max_new] (best - second best
    PROCESSED logit), raw_argmax [max_new], ban_hit / demoted [max_new] bool (the raw arg-max is banned / loses to the penalty alone), histories (per step)."""
    x = torch.from_numpy(np.asarray(inputs_embeds, np.float32)).to(ref.dt)
    pos3 = torch.as_tensor(np.asarray(position_ids, np.int64))
    nxt = int(pos3.max()) + 1
    cache = [None] * ref.c.L
    h = ref.forward_chunk(x, pos3, cache)[-1:]
    hist = [int(v) for v in history]
    out = dict(tokens=[], raw=[], margin=[], raw_argmax=[], ban_hit=[], demoted=[], histories=[])
    done = False
    for i in range(max_new_tokens):
        lg = ref.logits_of(h)[0]
        proc = process64(lg, hist, r, n)
        pen = process64(lg, hist, r, 0)
        ra = choose(lg.numpy())
        top = torch.topk(proc, 2).values
        tok = int(eos_token_id) if done else choose(proc.numpy())
        out["tokens"].append(tok); out["raw"].append(lg); out["margin"].append(float(top[0] - top[1])); out["raw_argmax"].append(ra)
        out["ban_hit"].append(ra in banned_tokens(hist, n)); out["demoted"].append(choose(pen.numpy()) != ra); out["histories"].append(list(hist))
        if eos_token_id is not None and tok == eos_token_id:
            done = True
        if i + 1 == max_new_tokens:
            break
        feed = tok
        if forced_tokens is not None and int(forced_tokens[i]) >= 0:
            feed = int(forced_tokens[i])
        hist.append(feed)
        h = ref.forward_chunk(ref.embed([feed]), torch.full((3, 1), nxt + i, dtype=torch.int64), cache)
    out["tokens"] = np.asarray(out["tokens"], np.int64)
    out["raw"] = torch.stack(out["raw"])
    for k in ("margin", "raw_argmax", "ban_hit", "demoted"):
        out[k] = np.asarray(out[k])
    return out


_REFS: dict = {}


def reference_for(name: str, seed: Optional[int] = None):
    """Computed once per process and shared: the case's weights, its prompts (embeds, positions, ids), for every setting and prompt the f64 run of STEPS tokens
    (runs[(r, n)][i]), and noise / tol as DESIGN 4.40 has them (f32 against f64 logits under the f64 run's tokens, over every setting, prompt and step)."""
    seed = SEEDS[name] if seed is None else seed
    key = (name, seed)
    if key not in _REFS:
        case = R.CASES[name]
        weights = R.make_lm(case, seed)
        prompts = [R.make_prompt(case, weights, T, seed) for T in LENGTHS]
        r64, r32 = R.RefLM(case, weights, torch.float64), R.RefLM(case, weights, torch.float32)
        runs, noise = {}, 0.0
        for (r, n) in SETTINGS:
            runs[(r, n)] = []
            for emb, pos, ids in prompts:
                g = generate(r64, emb, pos, ids, STEPS, r, n)
                _, l32 = r32.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=STEPS, forced_tokens=g["tokens"])
                noise = max(noise, float((l32.double() - g["raw"]).abs().max()))
                runs[(r, n)].append(g)
        _REFS[key] = dict(case=case, weights=weights, prompts=prompts, runs=runs, noise=noise, tol=max(16.0 * noise, 2.0 ** -19))
    return _REFS[key]


def conditions(ref) -> dict:
    """Per setting: least margin over 4 r tol (must exceed 1), the fewest steps of a sequence at which the processed token differs from the raw arg-max, and the
    case's counts of steps whose raw arg-max is banned / loses to the penalty alone."""
    out = {}
    for (r, n), runs in ref["runs"].items():
        out[(r, n)] = dict(margin_ratio=min(float(g["margin"].min()) for g in runs) / (4.0 * r * ref["tol"]),
                           least_differing=min(int((g["tokens"] != g["raw_argmax"]).sum()) for g in runs),
                           ban_hits=sum(int(g["ban_hit"].sum()) for g in runs), demoted=sum(int(g["demoted"].sum()) for g in runs))
    return out


# ------------------------------------------------------------------------------------------------ the select kernel's direct cases
KERNEL_VOCABS = (33, 97, 1030, 10007, 103424)
HISTORY_LENGTHS = lambda n: (0, 1, n - 1, n, 255, 256, 257, 1030)   # noqa: E731


def _six_ids(V: int):
    """six ids that sit on the presence bitmap's word borders and in the row's last, partial quad"""
    ids = {0, 1, V - 2, V - 1}
    return sorted(ids | ({31, 32} if 32 < V - 2 else {2, 3}))


def _history(rng, V: int, H: int, n: int, beyond: bool, crafted: bool) -> List[int]:
    ids = _six_ids(V) + ([V, V + 5, (1 << 24) + 3] if beyond else [])
    h = [int(ids[j]) for j in rng.integers(0, len(ids), H)]
    if crafted and n > 1 and H >= 2 * n + 1:
        a, b = ids[2], ids[5]
        h[H - n:] = [a] * n                      # i = H - n: the last n ids are equal, so a is banned
        h[:n - 1] = [a] * (n - 1)                # i = 0: the first n - 1 ids are the tail, the id behind them is banned
        h[n - 1] = b
    return h


def _logits(rng, rows: int, V: int) -> np.ndarray:
    x = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    x[:, rng.integers(0, V, max(V // 16, 2))] = 0.0
    x[:, rng.integers(0, V, max(V // 16, 2))] = -0.0
    for i in range(rows):
        if i % 4 == 1:
            x[i] = -np.abs(x[i]) - np.float32(0.25)          # negative winners: a seen winner moves away from zero
        if i % 4 == 2:
            x[i, rng.integers(0, V, max(V // 8, 3))] = np.nan
    return x


def kernel_cases() -> List[dict]:
    """Every dict: name, logits [rows, V] f32, histories (a list of id lists), r, n."""
    rng = np.random.default_rng(4047)
    cases = []
    for V in KERNEL_VOCABS:
        for n in (2, 3, 5):
            lens = list(HISTORY_LENGTHS(n)) * 2
            hs = [_history(rng, V, H, n, beyond=i >= 8, crafted=i % 2 == 0) for i, H in enumerate(lens)]
            cases.append(dict(name=f"v{V}_n{n}_rows16", logits=_logits(rng, 16, V), histories=hs, r=1.3, n=n))
        hs = [_history(rng, V, H, 3, beyond=True, crafted=True) for H in (257, 0, 40)]
        cases.append(dict(name=f"v{V}_rows3_ban_only", logits=_logits(rng, 3, V), histories=hs, r=1.0, n=3))
        cases.append(dict(name=f"v{V}_rows1_penalty_only", logits=_logits(rng, 1, V), histories=[_history(rng, V, 256, 0, True, False)], r=1.5, n=0))
        cases.append(dict(name=f"v{V}_rows3_n_beyond_history", logits=_logits(rng, 3, V), histories=[_history(rng, V, H, 0, False, False) for H in (1030, 5, 0)], r=1.3, n=2000))
        # rows of NaN alone, of -inf alone, and all tokens banned but one (after every `a` of the history comes every id but k)
        a, k = 1, V // 2
        x = _logits(rng, 3, V)
        x[0] = np.nan
        x[1] = -np.inf
        ban_all = [t for v in range(V) if v != k for t in (a, v)] + [a]
        if len(ban_all) <= 65536:
            cases.append(dict(name=f"v{V}_nan_inf_banned_but_one", logits=x, histories=[[0, 5 % V], [0, 5 % V, 0], ban_all], r=1.3, n=2))
        else:
            cases.append(dict(name=f"v{V}_nan_inf", logits=x[:2], histories=[[0, 5 % V], [0, 5 % V, 0]], r=1.3, n=2))
    # equal maxima d apart: with the lower one seen (r = 1.08) the upper wins, unseen the lower wins
    for V in (1030, 10007, 103424):
        lo, rows, hs = 3, [], []
        for d in (1, 64, 256, 1023):
            for seen in (True, False):
                x = (rng.standard_normal(V) * 2.0).astype(np.float32)
                x[lo] = x[lo + d] = np.float32(20.0)
                rows.append(x)
                hs.append([lo] if seen else [lo + 2])
        cases.append(dict(name=f"v{V}_equal_maxima", logits=np.stack(rows), histories=hs, r=1.08, n=0, equal_maxima=[(lo, d) for d in (1, 64, 256, 1023)]))
    return cases


def kernel_expected(case: dict) -> np.ndarray:
    return np.asarray([choose(process(case["logits"][i], case["histories"][i], case["r"], case["n"])) for i in range(len(case["histories"]))], np.int32)


# ------------------------------------------------------------------------------------------------ composite case PA (vision_reference.composite_reference) with processors
PA_SETTING = (1.3, 3)
_PA: dict = {}


def composite_reference():
    """vision_reference's composite case PA (two images through the vision stage into LM case A) decoded with PA_SETTING, the expanded ids (prefix, one image id per
    image token, suffix) as history: per sequence the f64 run of PA_STEPS tokens as `generate` gives it; tol is the composite case's own."""
    if not _PA:
        from . import vision_reference as vr
        base = vr.composite_reference()
        vc, lc, w = base["vis_case"], base["lm_case"], base["weights"]
        r64 = R.RefLM(lc, w, torch.float64)
        runs = []
        for img, grid, (_, _, ids, pos) in zip(base["images"], vr.PA_GRIDS, base["runs"]):
            px = vr.patchify_ref(img, 2, 1.0 / 255.0, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
            n_img = grid[0] * grid[1] // 4
            _, emb = vr.vision_forward(vc, w, px, "float64", grids=(grid,))
            x = r64.embed(ids).clone()
            x[2:2 + n_img] = torch.from_numpy(emb).to(x.dtype)
            runs.append(_generate_rows(r64, x, pos, ids, vr.PA_STEPS, *PA_SETTING))
        _PA.update(base=base, runs=runs, tol=base["tol"])
    return _PA


def _generate_rows(ref, x, pos, history, steps, r, n):
    """`generate` on embedding rows kept in f64 (its inputs_embeds argument goes through f32)"""
    pos3 = torch.as_tensor(np.asarray(pos, np.int64))
    nxt = int(pos3.max()) + 1
    cache = [None] * ref.c.L
    h = ref.forward_chunk(x, pos3, cache)[-1:]
    hist = [int(v) for v in history]
    toks, margin, raw_argmax = [], [], []
    for i in range(steps):
        lg = ref.logits_of(h)[0]
        proc = process64(lg, hist, r, n)
        top = torch.topk(proc, 2).values
        tok = choose(proc.numpy())
        toks.append(tok); margin.append(float(top[0] - top[1])); raw_argmax.append(choose(lg.numpy()))
        if i + 1 == steps:
            break
        hist.append(tok)
        h = ref.forward_chunk(ref.embed([tok]), torch.full((3, 1), nxt + i, dtype=torch.int64), cache)
    return dict(tokens=np.asarray(toks, np.int64), margin=np.asarray(margin), raw_argmax=np.asarray(raw_argmax))
