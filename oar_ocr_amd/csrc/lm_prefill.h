// lm_prefill.h -- the GEMM-based prefill of the decoder-only language model (lm_prefill_gemm.hip, lm_prefill_attn.hip): the tile and chunk
// arithmetic, the row and tile tables and the launchers.  Plain C++ (no HIP header): the host-only tests compile the inline functions below.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct ihipStream_t;

namespace oar {
namespace k {

constexpr int kLmPrefillDefaultChunk = 2048, kLmPrefillMaxChunk = 65536;
// lm_gemm: a workgroup of 4 waves owns kLmGemmTN weight rows x kLmGemmTM tokens (a wave 32 x 32 as 2 x 2 MFMA tiles); K streams through LDS in chunks of
// kLmGemmKC columns, two stages, rows padded to kLmGemmLd floats (9 float4 groups: odd, so the 16 fragment reads of a lane group fall on 16 different 16-byte slots)
constexpr int kLmGemmThreads = 256, kLmGemmTN = 64, kLmGemmTM = 64, kLmGemmKC = 32, kLmGemmLd = kLmGemmKC + 4;
inline size_t lm_gemm_lds_bytes() { return (size_t)2 * (kLmGemmTN + kLmGemmTM) * kLmGemmLd * 4 + kLmGemmTM * 4; }   // the two stages of W and X, 1 / rms per token
inline int lm_gemm_k_chunks(int Kp) { return (Kp + kLmGemmKC - 1) / kLmGemmKC; }
inline int64_t lm_gemm_workgroups(int64_t M, int64_t N) { return ((M + kLmGemmTM - 1) / kLmGemmTM) * ((N + kLmGemmTN - 1) / kLmGemmTN); }

// lm_prefill_attn: the layout of flash_f32_dev.h (64 queries, 32-key blocks, 256 threads) with LDS rows of 16 DH16 + 4 floats
constexpr int kLmPfQueries = 64, kLmPfKeys = 32, kLmPfThreads = 256, kLmPfMaxDh = 128, kLmPfMinDh = 8;
inline int lm_pf_dh16(int dh) { return (dh + 15) / 16; }
inline int lm_pf_ld(int dh) { return 16 * lm_pf_dh16(dh) + 4; }
inline size_t lm_pf_attn_lds_bytes(int dh) { return (size_t)2 * 2 * kLmPfKeys * lm_pf_ld(dh) * 4; }   // K and V, two stages each
inline bool lm_pf_head_dim_supported(int dh) { return dh >= kLmPfMinDh && dh <= kLmPfMaxDh && dh % 4 == 0; }

// One GEMM row: prompt position `pos` of sequence `seq`, its three rotary positions, its hidden vector's row in the arena.
struct LmPfRow { int32_t seq, pos, rp[3], xrow, pad[2]; };
// One attention workgroup: query head `head` of sequence `seq`, the queries at positions [lo, hi) of tile qt (positions 64 qt .. 64 qt + 63 of the sequence's
// own numbering, whatever the chunk); position lo is row `row_lo` of the launch's q buffer.  Keys 0 .. hi - 1 are in the cache.
struct LmPfTile { int32_t seq, head, qt, lo, hi, row_lo, pad[2]; };

// A run of query rows of one sequence inside one launch: positions [start, start + len), the first being row `row0` of the q buffer.
struct LmPfSpan { int32_t seq, start, len, row0; };

// tiles of one launch in the order (span, head, tile): tile qt of a span covers positions max(start, 64 qt) .. min(start + len, 64 qt + 64) - 1
inline int64_t lm_pf_tile_count(const LmPfSpan* spans, int n, int heads) {
    int64_t t = 0;
    for (int i = 0; i < n; ++i) {
        if (spans[i].len <= 0) continue;
        const int64_t first = spans[i].start / kLmPfQueries, last = ((int64_t)spans[i].start + spans[i].len - 1) / kLmPfQueries;
        t += (int64_t)heads * (last - first + 1);
    }
    return t;
}
inline void lm_pf_tiles(const LmPfSpan* spans, int n, int heads, std::vector<LmPfTile>& out) {
    for (int i = 0; i < n; ++i) {
        const LmPfSpan& s = spans[i];
        if (s.len <= 0) continue;
        const int end = s.start + s.len, first = s.start / kLmPfQueries, last = (end - 1) / kLmPfQueries;
        for (int h = 0; h < heads; ++h)
            for (int qt = first; qt <= last; ++qt) {
                const int lo = qt * kLmPfQueries > s.start ? qt * kLmPfQueries : s.start;
                const int hi = (qt + 1) * kLmPfQueries < end ? (qt + 1) * kLmPfQueries : end;
                out.push_back(LmPfTile{s.seq, h, qt, lo, hi, s.row0 + (lo - s.start), {0, 0}});
            }
    }
}

// The GEMM rows of a call: positions 0 .. T_i - 2 of every sequence, packed in order, cut into chunks of chunk_rows.  spans: the runs of every chunk,
// chunk_first[c] .. chunk_first[c + 1] being chunk c's; row0 counts from the chunk's first row.
inline void lm_pf_chunks(const int32_t* lengths, int n_seq, int chunk_rows, std::vector<LmPfSpan>& spans, std::vector<int>& chunk_first, std::vector<int>& chunk_rows_out) {
    spans.clear(); chunk_first.clear(); chunk_rows_out.clear();
    int fill = 0;
    bool open = false;
    for (int s = 0; s < n_seq; ++s) {
        int t = 0;
        const int n = lengths[s] - 1;
        while (t < n) {
            if (!open) { chunk_first.push_back((int)spans.size()); open = true; fill = 0; }
            const int take = n - t < chunk_rows - fill ? n - t : chunk_rows - fill;
            spans.push_back(LmPfSpan{s, t, take, fill});
            t += take; fill += take;
            if (fill == chunk_rows) { chunk_rows_out.push_back(fill); open = false; }
        }
    }
    if (open) chunk_rows_out.push_back(fill);
    chunk_first.push_back((int)spans.size());
}
inline int lm_pf_launches(int n_chunks, int L) { return n_chunks * (5 * (L - 1) + 1); }   // the last layer stops after its q/k/v launch

enum : int { LM_GEMM_PLAIN = 0, LM_GEMM_RESID = 1, LM_GEMM_QKV = 2, LM_GEMM_GATE = 3 };

struct LmGemmP {
    int mode, bf16;
    int M, N, K, Kp;                  // Y[M][N] = X[M][K] W[N][Kp]^T; K % 4 == 0
    const float* x; int x_ld;         // row m: x + (rows ? rows[m].xrow : m) * x_ld   (x_gather)
    int x_gather, y_scatter;
    const LmPfRow* rows;
    const void* w;
    const float* bias;                // QKV: [N] or null
    const float* rms_g; float eps;    // RMSNorm in front when rms_g != null
    float* y; int y_ld;               // PLAIN: y[m][n] = v; RESID: y[row][n] += v (row = rows[m].xrow when y_scatter); GATE: y[m][n / 2]
    float *q, *kc, *vc; int q_ld, nq, nk, dh, kvh, maxpos, sec0, sec1;
    const float* inv_freq;
};
void lm_gemm(ihipStream_t* s, const LmGemmP& p);

struct LmPfAttnP {
    const float* q; int q_ld;         // [rows][>= H dh]
    const float *kc, *vc;             // [sequences][KVH][maxpos][dh]
    int H, KVH, dh, maxpos;
    float scale;
    float* o; int o_ld;               // [rows][>= H dh]
    const LmPfTile* tiles; int n_tiles;
};
void lm_prefill_attention(ihipStream_t* s, const LmPfAttnP& p, double bytes, double flops);
// what one launch reads and computes: every tile streams keys 0 .. hi - 1 of its kv head
inline void lm_pf_attn_cost(const LmPfTile* tiles, int64_t n, int dh, double* bytes, double* flops) {
    double b = 0, f = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double q = tiles[i].hi - tiles[i].lo, keys = tiles[i].hi;
        b += 4.0 * (2.0 * keys * dh + 2.0 * q * dh);
        f += 4.0 * q * keys * dh;
    }
    *bytes = b; *flops = f;
}

}  // namespace k
}  // namespace oar
