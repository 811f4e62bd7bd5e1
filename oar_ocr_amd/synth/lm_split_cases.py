"""Cases of the split-key decode attention (lm_decode_split.hip): rows of one step at the edges of 64-key spans and tiles, their f64 / f32 references,
the header's arithmetic compiled for the host, and the sensitivity of the cases to one key too few.  Built on lm_prefill_cases.attn_case (whose caches hold 1e30 at
every unused position); the tolerance is the project's rule: noise = max |f32 - f64| of the torch reference itself, tol = max(16 noise, 2^-19)."""
from __future__ import annotations

import numpy as np

from . import lm_prefill_cases as P

SPLIT_LENS = (1, 193, 130)            # sequences 0, 1, 2
SPLIT_KEYS = 64
# rows of sequence 1 that see p + 1 = 63 .. 193 keys: one short of a span, a span, one past it, the same at two spans, three spans and one key into the fourth
EDGE_KEYS = (63, 64, 65, 127, 128, 129, 192, 193)
# the 11-row call: those, the one-position sequence, and positions 129 and 64 of the third sequence
ROWS = tuple((1, n - 1) for n in EDGE_KEYS) + ((0, 0), (2, 129), (2, 64))
DHS = P.ATTN_DHS                      # 8, 12, 20, 64, 80, 128
GS = (1, 3, 7, 8, 12)                 # workgroups of 1 head, 4 with one idle, 4 + 3, 8, 8 + 4
WIDE_DHS = (20, 128)                  # the head sizes that also run with split_keys 128
SENSITIVITY_TOLS = 4.0
SEED = 0

_CASES: dict = {}


def split_case(dh: int, G: int, kvh: int = 2, seed: int = SEED) -> dict:
    """The 11-row call at this head size and group size, computed once per process and shared: q [11, kvh G dh], kc / vc [3, kvh, 196, dh], row_seq / row_pos,
    o64 / o32 [11, kvh G dh], noise and tol (tol_all: over every query row of attn_case).  Do not write into the arrays."""
    key = (dh, G, kvh, seed)
    if key not in _CASES:
        q, kc, vc, o64, o32 = P.attn_case(SPLIT_LENS, dh, G, kvh, seed)
        off = np.concatenate([[0], np.cumsum(SPLIT_LENS)])
        idx = [int(off[s]) + p for s, p in ROWS]
        noise, tol = P.tol_of(o32[idx], o64[idx])                # of the call's own 11 rows: what the kernels are held to
        noise_all, tol_all = P.tol_of(o32, o64)                  # of all 324 causal query rows of attn_case (never smaller): what the sensitivity is measured in
        _CASES[key] = dict(q=np.ascontiguousarray(q[idx]), kc=kc, vc=vc, row_seq=np.array([s for s, _ in ROWS], np.int32), row_pos=np.array([p for _, p in ROWS], np.int32),
                           o64=o64[idx], o32=o32[idx], noise=noise, tol=tol, noise_all=noise_all, tol_all=tol_all, dh=dh, G=G, kvh=kvh, heads=kvh * G)
    return _CASES[key]


def attend64(case: dict, row: int, drop=None) -> np.ndarray:
    """f64 output [heads, dh] of row `row` of the case over keys 0 .. p of its sequence, without key `drop` when given."""
    s, p = int(case["row_seq"][row]), int(case["row_pos"][row])
    dh, G, kvh = case["dh"], case["G"], case["kvh"]
    keep = np.array([j for j in range(p + 1) if j != drop])
    q = case["q"][row].astype(np.float64).reshape(kvh, G, dh)
    K = case["kc"][s, :, keep].astype(np.float64).transpose(1, 0, 2)       # [kvh, keys, dh] (the key index leads after fancy indexing)
    V = case["vc"][s, :, keep].astype(np.float64).transpose(1, 0, 2)
    sc = np.einsum("kgd,ksd->kgs", q, K) * dh ** -0.5
    w = np.exp(sc - sc.max(-1, keepdims=True))
    w /= w.sum(-1, keepdims=True)
    return np.einsum("kgs,ksd->kgd", w, V).reshape(kvh * G, dh)


def sensitive_keys(p: int):
    """The keys whose loss the cases must show for a row at position p: the first, those around every span edge, the last two of the sequence and of the row."""
    return sorted({j for j in (0, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, p - 1, p) if 0 <= j <= p})


def least_movement(case: dict) -> float:
    """min over the rows of sequence 1, the sensitive keys of each and every head of max_d |o without the key - o|: what one key too few changes at least."""
    least = np.inf
    for row, n in enumerate(EDGE_KEYS):
        full = attend64(case, row)
        for j in sensitive_keys(n - 1):
            least = min(least, float(np.abs(attend64(case, row, drop=j) - full).max(axis=1).min()))
    return least


# ---------------------------------------------------------------------------------------------- the header's arithmetic, compiled for the host
_ARITH_PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "lm_decode.h"
int main(int argc, char** argv) {
    using namespace oar::k;
    const int S = std::atoi(argv[1]), H = std::atoi(argv[2]), dh = std::atoi(argv[3]), maxpos = std::atoi(argv[4]), L = std::atoi(argv[5]);
    std::printf("{\"threads\": %d, \"tile\": %d, \"min\": %d, \"max\": %d, \"default\": %d, \"merge_threads\": %d, \"stop_stride\": %d, \"stop_lookahead\": %d, \"stop_ring\": %d, ",
                kLmSplitThreads, kLmSplitTile, kLmSplitMin, kLmSplitMax, kLmSplitDefault, kLmMergeThreads, kLmStopStride, kLmStopLookahead, kLmStopRing);
    std::printf("\"supported\": %d, \"ws_bytes\": %zu, \"launches\": %d, \"launches_serial\": %d, \"gt\": {", (int)lm_split_keys_supported(S), lm_split_keys_supported(S) ? lm_split_ws_floats(H, dh, maxpos, S) * 4 : (size_t)0,
                lm_launches_per_step_split(L), lm_launches_per_step(L));
    for (int G = 1; G <= 16; ++G) std::printf("%s\"%d\": %d", G > 1 ? ", " : "", G, lm_split_gt(G));
    std::printf("}, \"ldk\": {");
    for (int d = kLmMinDh; d <= kLmMaxDh; d += 4) std::printf("%s\"%d\": %d", d > kLmMinDh ? ", " : "", d, lm_split_ldk(d));
    std::printf("}, \"lds\": {");
    for (int d = kLmMinDh; d <= kLmMaxDh; d += 4)
        for (int gt = 1; gt <= 8; gt *= 2) std::printf("%s\"%d,%d\": %zu", (d > kLmMinDh || gt > 1) ? ", " : "", d, gt, lm_split_lds_bytes(d, gt));
    std::printf("}, \"spans\": {");
    for (int i = 6; i < argc; ++i) std::printf("%s\"%d\": %d", i > 6 ? ", " : "", std::atoi(argv[i]), lm_split_keys_supported(S) ? lm_split_spans(std::atoi(argv[i]), S) : 0);
    std::printf("}}\n");
    return 0;
}
"""
_ARITH: dict = {}


def split_arithmetic(S: int = SPLIT_KEYS, heads: int = 16, dh: int = 128, maxpos: int = 4096, layers: int = 18, n_keys=()) -> dict:
    """csrc/lm_decode.h compiled for the host: the constants of the split mode, whether S is a valid split_keys, the workspace bytes of a model, the launches of a step,
    heads per workgroup gt[G], a staged key row's floats ldk[dh], the dynamic LDS lds[(dh, gt)] and, for every count of n_keys, the spans of a row that sees so many keys."""
    import json
    import shutil
    import subprocess
    import tempfile
    from pathlib import Path
    key = (int(S), int(heads), int(dh), int(maxpos), int(layers), tuple(int(n) for n in n_keys))
    if key not in _ARITH:
        csrc = Path(__file__).resolve().parents[1] / "csrc"
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        with tempfile.TemporaryDirectory() as d:
            (Path(d) / "arith.cc").write_text(_ARITH_PROG)
            subprocess.run([cxx, "-std=c++17", f"-I{csrc}", str(Path(d) / "arith.cc"), "-o", str(Path(d) / "arith")], check=True, capture_output=True, timeout=300)
            out = subprocess.run([str(Path(d) / "arith")] + [str(v) for v in key[:5]] + [str(n) for n in key[5]], check=True, capture_output=True, text=True, timeout=60).stdout
        g = json.loads(out)
        g["gt"] = {int(k): v for k, v in g["gt"].items()}
        g["ldk"] = {int(k): v for k, v in g["ldk"].items()}
        g["lds"] = {tuple(int(x) for x in k.split(",")): v for k, v in g["lds"].items()}
        g["spans"] = {int(k): v for k, v in g["spans"].items()}
        _ARITH[key] = g
    return _ARITH[key]
