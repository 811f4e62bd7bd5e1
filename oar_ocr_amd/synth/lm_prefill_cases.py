"""Cases of the GEMM-based prefill (lm_prefill_gemm.hip, lm_prefill_attn.hip): prompt lengths at the edges of the attention kernel's 64-query tiles on
the geometries of lm_reference's cases A and LA, and the f64 / f32 references of the two kernels alone.  Built from lm_reference's make_lm / make_prompt / RefLM; the
tolerance is lm_reference's rule: noise = max |f32 - f64| of the torch reference itself, tol = max(16 noise, 2^-19)."""
from __future__ import annotations

import numpy as np
import torch

from . import lm_reference as R

# (geometry, prompt lengths): the GEMM phase takes T - 1 rows of every prompt -- 63, 64, 65 and 128: one row short of a tile, a full tile, one row into the second
# tile, two full tiles -- and the four prompts are packed into one call, so every tile edge but the first also falls at a different row of the chunk
EDGE_LENGTHS = (64, 65, 66, 129)
EDGE_STEPS = 4
EDGE_CASES = {
    "TA": R.LmCase("TA", 64, 2, 4, 2, 16, 96, 97, (2, 3, 3)),               # case A: head size 16, G = 2
    "TLA": R.LmCase("TLA", 64, 2, 16, 2, 128, 96, 97, (16, 24, 24)),        # case LA: head size 128 (the widest instantiation), G = 8
}
# greedy-safe: the f64 best-to-second margin exceeds 4 tol at every forced step of every prompt (tests/test_lm_prefill_cases_cpu.py)
EDGE_SEEDS = {"TA": 0, "TLA": 0}
EDGE_MARGIN_TOLS = 4.0

_REFS: dict = {}


def edge_reference_for(name: str):
    """As lm_reference.reference_for: weights, the four prompts, EDGE_STEPS greedy f64 tokens and logits per prompt, noise and tol."""
    if name not in _REFS:
        case, seed = EDGE_CASES[name], EDGE_SEEDS[name]
        _REFS[name] = R._reference(case, R.make_lm(case, seed), seed, EDGE_LENGTHS, EDGE_STEPS, EDGE_STEPS)
    return _REFS[name]


def tol_of(ref32: np.ndarray, ref64: np.ndarray):
    """(noise, tol) of one op from its own torch references."""
    noise = float(np.abs(ref32.astype(np.float64) - ref64).max())
    return noise, max(16.0 * noise, 2.0 ** -19)


# ---------------------------------------------------------------------------------------------- the two kernels alone
GEMM_MS = (1, 15, 16, 17, 63, 64, 65, 130)
# a reduced cross of K in {4, 36, 1028} and N in {2, 30, 34, 258}: every K and every N, K = 4 and 36 below and above one 32-column chunk, 1028 ending in a chunk
# of 4; N = 2 and 30 inside one 64-row tile (30: a lane group's four rows half past the end), 34 and 258 past one and four tiles
GEMM_KN = ((4, 2), (4, 258), (36, 30), (36, 34), (1028, 2), (1028, 34), (1028, 258), (36, 258))


def gemm_case(M: int, K: int, N: int, bf16: bool, seed: int = 0):
    """x [M, K] f32, w [N, K] (float32, or uint16 bf16 bits), and y = x w^T in f64 and f32 from the values the kernel sees."""
    rng = np.random.default_rng(4200 + seed + 7 * M + 131 * K + 17 * N)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    wk = R.to_bf16_bits(w) if bf16 else w
    wv = R.bf16_bits_to_f32(wk) if bf16 else w
    y64 = torch.from_numpy(x).double() @ torch.from_numpy(wv).double().T
    y32 = torch.from_numpy(x) @ torch.from_numpy(wv).T
    return x, wk, y64.numpy(), y32.numpy()


ATTN_DHS = (8, 12, 20, 64, 80, 128)
ATTN_SEQS = ((1,), (31, 32, 33), (64, 65), (4, 140))
ATTN_GS = (1, 3, 8)


def attn_case(lens, dh: int, G: int, kvh: int = 2, seed: int = 0, extra: int = 3):
    """Sequences of `lens` positions, all of them queries (start 0): kcache / vcache [n, kvh, max(lens) + extra, dh] (the unused positions hold 1e30: a kernel
    that reads one shows it), q [sum lens, kvh G dh], and o [sum lens, kvh G dh] in f64 and f32."""
    rng = np.random.default_rng(4300 + seed + 3 * dh + 1000 * G + sum(lens))
    n, maxpos, H = len(lens), max(lens) + extra, kvh * G
    kc = np.full((n, kvh, maxpos, dh), 1e30, np.float32)
    vc = np.full((n, kvh, maxpos, dh), 1e30, np.float32)
    qs, o64, o32 = [], [], []
    for i, T in enumerate(lens):
        kc[i, :, :T] = rng.standard_normal((kvh, T, dh)).astype(np.float32)
        vc[i, :, :T] = rng.standard_normal((kvh, T, dh)).astype(np.float32)
        q = rng.standard_normal((T, H, dh)).astype(np.float32)
        qs.append(q.reshape(T, H * dh))
        for dt, out in ((torch.float64, o64), (torch.float32, o32)):
            K = torch.from_numpy(kc[i, :, :T]).to(dt).repeat_interleave(G, dim=0)       # [H, T, dh]: query head h uses kv head h // G
            V = torch.from_numpy(vc[i, :, :T]).to(dt).repeat_interleave(G, dim=0)
            s = torch.einsum("thd,hsd->hts", torch.from_numpy(q).to(dt), K) * dh ** -0.5
            s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool))[None], float("-inf"))
            out.append(torch.einsum("hts,hsd->thd", torch.softmax(s, dim=-1), V).reshape(T, H * dh).numpy())
    return np.concatenate(qs), kc, vc, np.concatenate(o64), np.concatenate(o32)


# ---------------------------------------------------------------------------------------------- the header's arithmetic, compiled for the host
_ARITH_PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "lm_prefill.h"
int main(int argc, char** argv) {
    using namespace oar::k;
    const int heads = std::atoi(argv[1]), chunk = std::atoi(argv[2]);
    std::vector<int32_t> lens;
    for (int i = 3; i < argc; ++i) lens.push_back(std::atoi(argv[i]));
    std::vector<LmPfSpan> spans; std::vector<int> first, rows;
    lm_pf_chunks(lens.data(), (int)lens.size(), chunk, spans, first, rows);
    std::printf("{\"gemm_lds\": %zu, \"attn_lds\": {", lm_gemm_lds_bytes());
    for (int dh = kLmPfMinDh; dh <= kLmPfMaxDh; dh += 4) std::printf("%s\"%d\": %zu", dh > kLmPfMinDh ? ", " : "", dh, lm_pf_attn_lds_bytes(dh));
    std::printf("}, \"default_chunk\": %d, \"max_chunk\": %d, \"chunks\": [", kLmPrefillDefaultChunk, kLmPrefillMaxChunk);
    for (size_t c = 0; c < rows.size(); ++c) {
        std::printf("%s{\"rows\": %d, \"spans\": [", c ? ", " : "", rows[c]);
        for (int i = first[c]; i < first[c + 1]; ++i) std::printf("%s[%d, %d, %d, %d]", i > first[c] ? ", " : "", spans[i].seq, spans[i].start, spans[i].len, spans[i].row0);
        std::vector<LmPfTile> tiles;
        lm_pf_tiles(spans.data() + first[c], first[c + 1] - first[c], heads, tiles);
        std::printf("], \"count\": %lld, \"tiles\": [", (long long)lm_pf_tile_count(spans.data() + first[c], first[c + 1] - first[c], heads));
        for (size_t i = 0; i < tiles.size(); ++i)
            std::printf("%s[%d, %d, %d, %d, %d, %d]", i ? ", " : "", tiles[i].seq, tiles[i].head, tiles[i].qt, tiles[i].lo, tiles[i].hi, tiles[i].row_lo);
        std::printf("]}");
    }
    std::printf("], \"launches\": %d}\n", lm_pf_launches((int)rows.size(), 3));
    return 0;
}
"""
_ARITH: dict = {}


def prefill_arithmetic(lengths, heads: int = 1, chunk_rows: int = 2048) -> dict:
    """csrc/lm_prefill.h compiled for the host: LDS bytes of the two kernels, and for prompts of `lengths` positions cut into chunks of chunk_rows packed rows the
    chunks' rows, spans [seq, start, len, row0] and attention tiles [seq, head, qt, lo, hi, row_lo]; `launches` is the GEMM phase's launch count at 3 layers."""
    import json
    import shutil
    import subprocess
    import tempfile
    from pathlib import Path
    key = (tuple(int(n) for n in lengths), int(heads), int(chunk_rows))
    if key not in _ARITH:
        csrc = Path(__file__).resolve().parents[1] / "csrc"
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        with tempfile.TemporaryDirectory() as d:
            (Path(d) / "arith.cc").write_text(_ARITH_PROG)
            subprocess.run([cxx, "-std=c++17", f"-I{csrc}", str(Path(d) / "arith.cc"), "-o", str(Path(d) / "arith")], check=True, capture_output=True, timeout=300)
            out = subprocess.run([str(Path(d) / "arith"), str(heads), str(chunk_rows)] + [str(n) for n in key[0]], check=True, capture_output=True, text=True, timeout=60).stdout
        g = json.loads(out)
        g["attn_lds"] = {int(k): v for k, v in g["attn_lds"].items()}
        _ARITH[key] = g
    return _ARITH[key]
