// lm_decode.h -- the decoder-only language-model chain (lm_decode.hip): shapes, the per-step row table and the launchers.
// Plain C++ (no HIP header): the LDS sizes below are also compiled by the host-only resource test.
#pragma once
#include <cstddef>
#include <cstdint>

struct ihipStream_t;

namespace oar {
namespace k {

constexpr int kLmRows = 16;          // rows ((sequence, position) pairs) of one step
constexpr int kLmThreads = 256;      // rows / lm-head / combine kernels
constexpr int kLmKC = 1024;          // columns of the row inputs staged in LDS at a time
constexpr int kLmAttnThreads = 512;  // attention: 8 waves, each takes every 8th group of keys
constexpr int kLmAttnWaves = kLmAttnThreads / 64;
constexpr int kLmAttnUnroll = 4;     // attention: turns of a wave whose keys and values are loaded before the first is used
constexpr int kLmWaves = kLmThreads / 64;
constexpr int kLmR = 2;              // matrix rows a wave of the rows kernels owns at a time (a rotary or gate / up pair)
constexpr int kLmTargetWgs = 512;    // rows kernels: a workgroup takes as many row groups (kLmWaves x kLmR rows each) as keep the grid at about this size
constexpr int kLmMaxDh = 128, kLmMinDh = 8;
constexpr int kLmMaxGT = 8;          // query heads of one kv head that a workgroup serves at once (a larger group takes several workgroups)

// One row of a step.  xrow: the row's hidden vector in the arena ([arena rows][D]); gen >= 0: the row's logits give generated token `gen` of its sequence.
struct LmRow { int32_t seq, pos, rp[3], xrow, gen, pad; };
struct LmStep { int32_t nrows, nhead, pad[2]; LmRow rows[kLmRows]; int32_t head[kLmRows]; };   // head[i]: slot of the i-th row that needs a token
struct LmState { int32_t done[kLmRows]; int32_t alive; int32_t pad[3]; };

struct LmLayerW { const void *w_qkv, *w_o, *w_gu, *w_down; const float *b_qkv, *ln1, *ln2; };

struct LmDecodeP {
    int D, L, H, KVH, dh, F, V, maxpos, sec0, sec1, bf16;   // sec0 / sec1: frequencies below sec0 take axis 0, below sec0 + sec1 axis 1, the rest axis 2
    float eps;
    const LmLayerW* layers;      // host array [L] of device pointers
    const float* lnf;
    const void *w_lm, *embed;    // [V][pad4(D)] each (the same table when tied)
    const float* inv_freq;       // [dh / 2]
    float *kcache, *vcache;      // [L][sequences][KVH][maxpos][dh] each
    size_t cache_layer;          // floats of one layer's K (or V) cache
    float* arena;                // [arena rows][D]: prompt rows, then one decode row per sequence from xdec0 on
    int xdec0;
    float *q, *o, *h;            // [16][H dh], [16][H dh], [16][F]
    void* part;                  // float2 [16][lm workgroups]
    LmState* state;
    int32_t* tokens;             // [sequences][max_new]
    const int32_t* forced;       // [sequences][max_new] or null; < 0: not forced
    float* logits;               // [sequences][max_new][V] or null
    int max_new, eos;
    float* split_ws;             // split-key attention: partials [16][H][ceil(maxpos / split_keys)][dh + 2], or null
    int split_keys;              // keys of one span (a multiple of 64 in 64..4096); read in split mode only
    // logits processors (lm_logits.hip): select != 0 runs the lm-head that also fills step_logits, then lm_select, and lm_combine on its one candidate
    int select;
    float* step_logits;          // [16][pad4(V)], row = the head row's slot in the step
    void* part1;                 // float2 [16]
    int32_t* hist; int hist_cap; // [16][hist_cap]: the prompt ids, then every token fed back
    const int32_t* hlen;         // [16]: ids of the prompt part
    uint32_t* seen;              // [16][ceil(V / 32)]: bit t = id t is in the history
    float penalty; int ngram;
};

// Split-key decode attention (lm_decode_split.hip): a row's keys are cut into spans of split_keys keys, one workgroup per (row, kv head, chunk of
// query heads, span) writes one partial (maximum, sum, weighted value sum [dh]) per head, and a second launch merges a row's partials in span order.
constexpr int kLmSplitThreads = 256;   // 4 waves: all stage a tile of keys and values, wave w scores and accumulates the heads w HPW .. of the chunk
constexpr int kLmSplitWaves = kLmSplitThreads / 64;
constexpr int kLmSplitTile = 64;       // keys staged in LDS at a time: lane j scores key j
constexpr int kLmSplitMin = 64, kLmSplitMax = 4096;
constexpr int kLmSplitDefault = 64;    // what split_keys 0 means (the measurement: DESIGN 4.43)
constexpr int kLmMergeThreads = 128;   // one workgroup per (row, head), thread d
enum : int { LM_ATTN_SERIAL = 0, LM_ATTN_SPLIT = 1 };
// Stop at eos: every kLmStopStride steps the host copies state.alive (4 bytes) into a pinned ring behind the step and records an event; before it enqueues step i
// it waits for the newest copy taken kLmStopLookahead or more steps back (long finished in the steady state: the device keeps a lookahead of queued steps) and
// stops once that word is 0.  With t_stop the index, over all steps of the call, of the step whose lm_combine ended the last sequence:
//     steps_enqueued <= t_stop + 1 + kLmStopLookahead + kLmStopStride.
constexpr int kLmStopStride = 8, kLmStopLookahead = 16, kLmStopRing = 8;

inline bool lm_split_keys_supported(int S) { return S >= kLmSplitMin && S <= kLmSplitMax && S % kLmSplitTile == 0; }
inline int lm_split_spans(int n_keys, int S) { return (n_keys + S - 1) / S; }   // spans of a row that sees n_keys = p + 1 keys (of a cache: n_keys = maxpos)
constexpr int lm_split_gt(int G) { return G >= 8 ? 8 : G > 2 ? 4 : G; }           // query heads per workgroup, as the serial kernel: 1, 2, 4 or 8
constexpr int lm_split_ldk(int dh) { return 4 * ((dh / 4) | 1); }                 // floats of a staged key row: an odd number of float4s, so that 16 lanes reading 16 rows 16 bytes at a time cover all 64 banks
inline size_t lm_split_lds_bytes(int dh, int gt) { return 4 * ((size_t)gt * dh + (size_t)kLmSplitTile * lm_split_ldk(dh) + (size_t)kLmSplitTile * dh + (size_t)gt * kLmSplitTile); }   // q | K tile | V tile | weights
inline size_t lm_split_ws_floats(int H, int dh, int maxpos, int S) { return (size_t)kLmRows * H * lm_split_spans(maxpos, S) * (dh + 2); }
inline int lm_launches_per_step_split(int L) { return 6 * L + 2; }

struct LmAttnArgs {
    const LmStep* st;
    const float* q; int q_ld;
    const float *kc, *vc;        // one layer's caches
    int H, KVH, dh, maxpos;
    float* o; int o_ld;
    const int* alive;
    float* ws; int split_keys;   // LM_ATTN_SPLIT only
};

inline int lm_pad4(int n) { return (n + 3) & ~3; }
inline int lm_nb(int rows) { int nb = 1; while (nb < rows) nb <<= 1; return nb; }
// dynamic LDS of a rows / lm-head launch with `rows` rows over K input columns; static LDS of the attention kernel at its widest instantiation
inline size_t lm_rows_lds_bytes(int rows, int K) { const int kp = lm_pad4(K); return (size_t)lm_nb(rows) * (size_t)(kp < kLmKC ? kp : kLmKC) * 4; }
inline size_t lm_rows_static_lds_bytes() { return 16 * 4 + 4 * 16 * 4 * 2; }
inline size_t lm_attn_lds_bytes() { return (size_t)kLmAttnWaves * kLmMaxGT * (kLmMaxDh + 2) * 4; }
inline bool lm_head_dim_supported(int dh) { return dh >= kLmMinDh && dh <= kLmMaxDh && dh % 4 == 0; }
inline int lm_launches_per_step(int L) { return 5 * L + 2; }
// rows kernels over an [N][K] matrix: row groups per workgroup, and workgroups
inline int lm_groups_for(int N) { const int per = kLmWaves * kLmR; const int g = (N + per * kLmTargetWgs - 1) / (per * kLmTargetWgs); return g > 1 ? g : 1; }
inline int lm_wgs_for(int N) { const int rows = lm_groups_for(N) * kLmWaves * kLmR; return (N + rows - 1) / rows; }
// attention: lanes that hold one key (the power of two >= dh / 4, at least 2), and keys a wave takes per turn
constexpr int lm_attn_lanes_per_key(int dh) { int lpk = 2; while (lpk * 4 < dh) lpk <<= 1; return lpk; }   // (constexpr: the kernel calls it too)
constexpr int lm_attn_keys_per_wave(int dh) { return 64 / lm_attn_lanes_per_key(dh); }
int lm_head_workgroups(int V);

void lm_embed(ihipStream_t* s, const LmDecodeP& p, const int32_t* ids, const int32_t* xrows, int n);   // arena[xrows[i]] = E[ids[i]]
void lm_step(ihipStream_t* s, const LmDecodeP& p, const LmStep* dev_step, int nrows, int nhead, int max_pos_in_step, int attention = LM_ATTN_SERIAL);
// the attention block of a step: lm_attn_kernel (one launch), or lm_attn_split + lm_attn_merge (two); prefill chooses the profiler classes
void lm_attention(ihipStream_t* s, const LmAttnArgs& a, int attention, int nrows, bool prefill, int max_pos_in_step);
void lm_attention_split(ihipStream_t* s, const LmAttnArgs& a, int nrows, bool prefill, int max_pos_in_step);   // lm_decode_split.hip

}  // namespace k
}  // namespace oar
