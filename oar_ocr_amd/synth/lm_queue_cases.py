"""The workload of queued generation (csrc/lm_queue.h): 40 prompts of case A of synth/lm_reference.py with mixed lengths, 12 tokens asked for and an
eos id at which the f64 greedy runs end at several different lengths, so that cache slots are handed over under way.  Expected tokens are the f64 run cut at its
first eos and filled with eos; the tolerance is the project's rule over the workload's own live rows: noise = max |f32 - f64| of the torch reference, teacher-forced,
tol = max(16 noise, 2^-19).  The module asserts the spread it needs itself; the scheduler's constants come from the header compiled for the host."""
from __future__ import annotations

import numpy as np
import torch

from . import lm_reference as R

CASE = "A"
LENGTHS = (1, 3, 37, 16, 17, 2, 15, 33, 5, 18, 31, 4, 20, 9, 12, 7, 25, 1, 36, 11, 6, 29, 14, 8, 22, 3, 19, 10, 35, 13, 2, 27, 21, 5, 30, 17, 24, 9, 1, 32)
MAX_NEW = 12
EOS = 48
PROMPT_SEED0 = 50            # prompt i is make_prompt(case, weights, LENGTHS[i], PROMPT_SEED0 + i)
MIN_EARLY, MIN_EARLY_LENGTHS, MIN_AT_LIMIT = 8, 4, 8
MIN_MARGIN_TOLS = 2.0        # a greedy choice survives an error of tol on both logits

_WORK: dict = {}


def counts_of(tokens: np.ndarray, eos) -> np.ndarray:
    """Tokens up to and including the first eos of every row, else the row's length."""
    tokens = np.atleast_2d(tokens)
    out = np.full(tokens.shape[0], tokens.shape[1], np.int32)
    if eos is not None:
        for i, row in enumerate(tokens):
            hit = np.flatnonzero(row == eos)
            if len(hit):
                out[i] = hit[0] + 1
    return out


def workload(max_new: int = MAX_NEW, eos: int = EOS) -> dict:
    """Computed once per process and shared (do not write into the arrays): case, weights, prompts [(embeds, position_ids, ids)], tokens [n, max_new] (the f64
    run cut at eos and filled with eos), counts [n], logits64 [n, max_new, V] (teacher-forced with `tokens`; rows >= counts are not to be compared), noise, tol,
    margin (the smallest best - second best over the live rows)."""
    key = (max_new, eos)
    if key in _WORK:
        return _WORK[key]
    ref = R.reference_for(CASE)
    case, weights = ref["case"], ref["weights"]
    prompts = [R.make_prompt(case, weights, T, PROMPT_SEED0 + i) for i, T in enumerate(LENGTHS)]
    r64, r32 = R.RefLM(case, weights, torch.float64), R.RefLM(case, weights, torch.float32)
    n = len(prompts)
    tokens = np.zeros((n, max_new), np.int32)
    logits = np.zeros((n, max_new, case.vocab), np.float64)
    noise, margin = 0.0, np.inf
    for i, (emb, pos, _) in enumerate(prompts):
        t64, l64 = r64.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=max_new)
        c = int(counts_of(t64, eos)[0])
        t64[c:] = eos
        _, l32 = r32.generate(inputs_embeds=emb, position_ids=pos, max_new_tokens=c, forced_tokens=t64)
        noise = max(noise, float((l32.double() - l64[:c]).abs().max()))
        margin = min(margin, float(R.greedy_margins(l64[:c]).min()))
        tokens[i], logits[i] = t64, l64.numpy()
    counts = counts_of(tokens, eos)
    tol = max(16.0 * noise, 2.0 ** -19)
    w = dict(case=case, weights=weights, prompts=prompts, tokens=tokens, counts=counts, logits64=logits, noise=noise, tol=tol, margin=margin, max_new=max_new, eos=eos)
    if key == (MAX_NEW, EOS):   # the spread the tests lean on: slots change hands at different steps, and some sequences run to the limit
        early = counts[counts < max_new]
        assert len(early) >= MIN_EARLY and len(set(early.tolist())) >= MIN_EARLY_LENGTHS and int((counts == max_new).sum()) >= MIN_AT_LIMIT, counts.tolist()
        assert margin >= MIN_MARGIN_TOLS * tol, (margin, tol)
    _WORK[key] = w
    return w


_CONST_PROG = r"""
#include <cstdio>
#include "lm_queue.h"
int main() {
    using namespace oar::k;
    std::printf("{\"stride\": %d, \"lookahead\": %d, \"ring\": %d, \"max_seq\": %d, \"threads\": %d, \"vec_per_thread\": %d, \"max_blocks\": %d, \"rows\": %d, "
                "\"blocks\": [%d, %d, %d, %d, %d]}\n", kLmQueueStride, kLmQueueLookahead, kLmQueueRing, kLmQueueMaxSeq, kLmQueueThreads, kLmQueueVecPerThread, kLmQueueMaxBlocks,
                kLmRows, lm_queue_turnover_blocks(12, 97, false), lm_queue_turnover_blocks(12, 97, true), lm_queue_turnover_blocks(1024, 103424, false),
                lm_queue_turnover_blocks(64, 103424, true), lm_queue_turnover_blocks(4096, 103424, true));
    return 0;
}
"""
_CONST: dict = {}


def queue_constants() -> dict:
    """csrc/lm_queue.h compiled for the host: stride, lookahead, ring, max_seq, the turnover kernel's launch constants and blocks: its workgroups per entry
    at (max_new, V, logits) = (12, 97, no), (12, 97, yes), (1024, 103424, no), (64, 103424, yes), (4096, 103424, yes)."""
    import json
    import shutil
    import subprocess
    import tempfile
    from pathlib import Path
    if not _CONST:
        csrc = Path(__file__).resolve().parents[1] / "csrc"
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        with tempfile.TemporaryDirectory() as d:
            (Path(d) / "const.cc").write_text(_CONST_PROG)
            subprocess.run([cxx, "-std=c++17", f"-I{csrc}", str(Path(d) / "const.cc"), "-o", str(Path(d) / "const")], check=True, capture_output=True, timeout=300)
            _CONST.update(json.loads(subprocess.run([str(Path(d) / "const")], check=True, capture_output=True, text=True, timeout=60).stdout))
    return _CONST
