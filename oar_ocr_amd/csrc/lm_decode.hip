// lm_decode.hip -- a decoder-only transformer (RMSNorm, multi-axis rotary positions "M-RoPE", grouped-query attention over a key / value cache, SwiGLU MLP:
// the Qwen2 / ERNIE-4.5 text decoder of the VL models) as a fixed chain of short weight-streaming launches.  A sibling of formula_decode.hip with its own code.
//
// The unit of work is a ROW: one (sequence, position) pair with its hidden vector [D].  A step processes up to 16 rows, described by an LmStep table in
// device memory (per row: sequence, cache position p, the three rotary positions, where its hidden vector lives, whether its logits are wanted).  In decode the
// rows are the current tokens of up to 16 sequences, in prefill up to 16 consecutive prompt positions of one sequence or of several: the same code.
// Per step 5 L + 2 launches, nothing ever waits on another workgroup:
//   per layer  1 lm_rows      RMSNorm -> [Wq ; Wk ; Wv] (+ bias), M-RoPE on q and k in the epilogue; q to its row buffer, k / v into the cache at (sequence, kv head, p)
//              2 lm_attn      row r attends cache positions 0 .. p_r of its sequence (launch 1 has stored the chunk's keys: prefill is causal without a mask);
//                             one workgroup per (row, kv head) serves the H / KVH query heads of the group, running maximum and sum, no score row anywhere
//              3 lm_rows      Wo + residual
//              4 lm_rows      RMSNorm -> [Wgate ; Wup] interleaved row by row, epilogue silu(g) u on the pair in registers
//              5 lm_rows      Wdown + residual
//   then       6 lm_head      final RMSNorm -> lm-head for the rows that need a token: logits (when asked for) and one (value, index) partial per workgroup and row
//              7 lm_combine   lowest index among equal maxima -> the token; eos bookkeeping; the sequence's next input row = E[token] (or the forced token)
// With a logits processor on (LmDecodeP.select) launch 6 is lm_logits.hip's lm_head_step, lm_select follows it, and lm_combine reads one candidate per row.
// The rows / lm-head body itself lives in lm_rows_dev.h, which lm_logits.hip instantiates too.
// Opt-in (lm_step's `attention`): launch 2 as lm_attn_split + lm_attn_merge of lm_decode_split.hip, the keys of a row cut into spans: 6 L + 2 launches.
// The rotary pair (d, d + dh / 2) of a head and the (gate, up) pair of an MLP column are ADJACENT rows of the stacked matrices (the host permutes them at upload),
// so the wave that owns two rows holds both halves of a pair after its reduction.
//
// Row independence: every dot product is reduced in an order fixed by K alone (lane q takes the float4 q, q + 64, ... of each 1024-column chunk, chunks in order,
// then a butterfly over the wave; the RMSNorm's sum of squares likewise); an attention sum in an order fixed by p and dh alone.  Neither the number of rows of a step nor a row's slot enters.  No float
// atomics: two runs give the same bytes.  Weights are f32 or bf16 (widened in registers: the same arithmetic on the same values); activations, q and the cache f32.
#include <algorithm>

#include "common.h"
#include "lm_decode.h"
#include "lm_logits.h"
#include "lm_rows_dev.h"

namespace oar {
namespace k {

namespace {

template <int NB, typename WT>
__global__ __launch_bounds__(kLmThreads) void lm_rows_kernel(LmRowsP p) { lm_rows_body<NB, LM_PLAIN, WT>(p); }
template <int NB, typename WT>
__global__ __launch_bounds__(kLmThreads) void lm_qkv_rows_kernel(LmRowsP p) { lm_rows_body<NB, LM_QKV, WT>(p); }
template <int NB, typename WT>
__global__ __launch_bounds__(kLmThreads) void lm_gate_rows_kernel(LmRowsP p) { lm_rows_body<NB, LM_GATE, WT>(p); }
template <int NB, typename WT>
__global__ __launch_bounds__(kLmThreads) void lm_head_kernel(LmRowsP p) { lm_rows_body<NB, LM_HEAD, WT>(p); }

// Attention of one (row, kv head, chunk of <= GT query heads of its group).  LPK = the power of two >= dh / 4 lanes hold one key (a float4 each), so a wave takes
// 64 / LPK keys per turn and wave w the turns w, w + 8, ...; every lane group keeps a running (maximum, sum, weighted value sum) per head.  The groups of a wave
// are merged by a butterfly, the 8 waves through LDS in wave order: the order depends on p and dh only.
struct LmAttnP {
    const LmStep* st;
    const float* q; int q_ld;
    const float *kc, *vc;
    int H, KVH, dh, maxpos;
    float scale;
    float* o; int o_ld;
    const int* alive;
};

template <int GT>
__global__ __launch_bounds__(kLmAttnThreads) void lm_attn_kernel(LmAttnP p) {
    __shared__ float sm[kLmAttnWaves][GT], sl[kLmAttnWaves][GT];
    __shared__ float4 sacc[kLmAttnWaves][GT][kLmMaxDh / 4];
    if (*p.alive == 0) return;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kvh = (int)blockIdx.x, b = (int)blockIdx.y, g0 = (int)blockIdx.z * GT;
    const LmRow& R = p.st->rows[b];
    const int dh = p.dh, G = p.H / p.KVH, n = R.pos + 1;
    const int lpk = lm_attn_lanes_per_key(dh);
    const int kpw = 64 / lpk, d4 = lane & (lpk - 1), grp = lane / lpk;
    const bool din = d4 * 4 < dh;
    float4 qv[GT], acc[GT];
    float m[GT], l[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        const int head = kvh * G + g0 + g;
        qv[g] = (din && g0 + g < G) ? *reinterpret_cast<const float4*>(p.q + (size_t)b * p.q_ld + head * dh + d4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        m[g] = -INFINITY; l[g] = 0.0f;
    }
    const size_t base = ((size_t)R.seq * p.KVH + kvh) * p.maxpos * dh;
    const float* kb = p.kc + base;
    const float* vb = p.vc + base;
    constexpr int U = kLmAttnUnroll;   // turns whose keys and values are loaded before the first is used (the same order of keys as one turn at a time)
    const int turn = kLmAttnWaves * kpw;
    for (int j0 = wave * kpw; j0 < n; j0 += U * turn) {   // (uniform over the wave)
        float4 kk[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * turn + grp;
            kk[u] = make_float4(0.f, 0.f, 0.f, 0.f); vv[u] = kk[u];
            if (j < n && din) {
                kk[u] = *reinterpret_cast<const float4*>(kb + (size_t)j * dh + d4 * 4);
                vv[u] = *reinterpret_cast<const float4*>(vb + (size_t)j * dh + d4 * 4);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (j0 + u * turn >= n) break;   // (uniform over the wave)
            const bool ok = j0 + u * turn + grp < n;
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                float s = 0.0f;
                s = fmaf(qv[g].x, kk[u].x, s); s = fmaf(qv[g].y, kk[u].y, s); s = fmaf(qv[g].z, kk[u].z, s); s = fmaf(qv[g].w, kk[u].w, s);
                for (int o = 1; o < lpk; o <<= 1) s += __shfl_xor(s, o, 64);
                s = s * p.scale;
                if (ok) {
                    const float mn = fmaxf(m[g], s);
                    const float c = expf(m[g] - mn), e = expf(s - mn);   // (m = -inf at the group's first key: c = 0)
                    l[g] = l[g] * c + e;
                    acc[g].x = acc[g].x * c + e * vv[u].x; acc[g].y = acc[g].y * c + e * vv[u].y; acc[g].z = acc[g].z * c + e * vv[u].z; acc[g].w = acc[g].w * c + e * vv[u].w;
                    m[g] = mn;
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        for (int o = lpk; o < 64; o <<= 1) {
            const float om = __shfl_xor(m[g], o, 64), ol = __shfl_xor(l[g], o, 64);
            const float ox = __shfl_xor(acc[g].x, o, 64), oy = __shfl_xor(acc[g].y, o, 64), oz = __shfl_xor(acc[g].z, o, 64), ow = __shfl_xor(acc[g].w, o, 64);
            const float mn = fmaxf(m[g], om);
            if (mn != -INFINITY) {   // (a group that saw no key has weight 0)
                const float c1 = m[g] == -INFINITY ? 0.0f : expf(m[g] - mn), c2 = om == -INFINITY ? 0.0f : expf(om - mn);
                // the lower lane group's term first on both sides: both lanes of a pair compute the same sums
                const bool lo = (lane & o) == 0;
                const float ca = lo ? c1 : c2, cb = lo ? c2 : c1;
                const float la = lo ? l[g] : ol, lb = lo ? ol : l[g];
                l[g] = la * ca + lb * cb;
                acc[g].x = (lo ? acc[g].x : ox) * ca + (lo ? ox : acc[g].x) * cb;
                acc[g].y = (lo ? acc[g].y : oy) * ca + (lo ? oy : acc[g].y) * cb;
                acc[g].z = (lo ? acc[g].z : oz) * ca + (lo ? oz : acc[g].z) * cb;
                acc[g].w = (lo ? acc[g].w : ow) * ca + (lo ? ow : acc[g].w) * cb;
                m[g] = mn;
            }
        }
        if (grp == 0 && din) sacc[wave][g][d4] = acc[g];
        if (lane == 0) { sm[wave][g] = m[g]; sl[wave][g] = l[g]; }
    }
    __syncthreads();
    for (int idx = tid; idx < GT * dh; idx += kLmAttnThreads) {
        const int g = idx / dh, d = idx - g * dh;
        if (g0 + g >= G) continue;
        float M = sm[0][g];
        for (int w = 1; w < kLmAttnWaves; ++w) M = fmaxf(M, sm[w][g]);
        float L = 0.0f, O = 0.0f;
        for (int w = 0; w < kLmAttnWaves; ++w) {
            const float mw = sm[w][g];
            if (mw == -INFINITY) continue;   // (a wave without keys)
            const float c = expf(mw - M);
            L = L + sl[w][g] * c;
            O = O + reinterpret_cast<const float*>(&sacc[w][g][0])[d] * c;
        }
        p.o[(size_t)b * p.o_ld + (kvh * G + g0 + g) * dh + d] = O / L;
    }
}

struct LmCombineP {
    const LmStep* st;
    const float2* part; int nwg;
    int V, D, Kp, bf16;
    const void* embed;
    float* arena; int xdec0;
    LmState* state;
    int32_t* tokens; const int32_t* forced; int max_new, eos;
};

__device__ __forceinline__ float embed_at(const void* e, int bf16, size_t i) {
    return bf16 ? __uint_as_float((unsigned)reinterpret_cast<const uint16_t*>(e)[i] << 16) : reinterpret_cast<const float*>(e)[i];
}

__global__ __launch_bounds__(kLmThreads) void lm_combine_kernel(LmCombineP p) {
    __shared__ float red_v[kLmWaves];
    __shared__ int red_i[kLmWaves];
    __shared__ int tok_s, skip_s, done_s;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, b = (int)blockIdx.x;
    const LmRow& R = p.st->rows[p.st->head[b]];
    LmState* st = p.state;
    if (tid == 0) {
        done_s = st->done[R.seq];   // (only this workgroup touches done[seq] in this launch)
        // 0 here means every sequence has finished, this one included (it has not left `alive` in this launch before this read)
        skip_s = __atomic_load_n(&st->alive, __ATOMIC_RELAXED) == 0;
        if (skip_s || done_s) { tok_s = p.eos; p.tokens[(size_t)R.seq * p.max_new + R.gen] = p.eos; }
    }
    __syncthreads();
    if (skip_s) return;
    if (!done_s) {
        float v = -INFINITY;
        int ix = 0x7fffffff;
        for (int i = tid; i < p.nwg; i += kLmThreads) {
            const float2 e = p.part[(size_t)b * p.nwg + i];
            const int oi = __float_as_int(e.y);
            if (better(e.x, oi, v, ix)) { v = e.x; ix = oi; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(ix, o, 64);
            if (better(ov, oi, v, ix)) { v = ov; ix = oi; }
        }
        if (lane == 0) { red_v[wave] = v; red_i[wave] = ix; }
        __syncthreads();
        if (tid == 0) {
            v = red_v[0]; ix = red_i[0];
            for (int w = 1; w < kLmWaves; ++w)
                if (better(red_v[w], red_i[w], v, ix)) { v = red_v[w]; ix = red_i[w]; }
            if (ix < 0 || ix >= p.V) ix = 0;   // (all logits NaN: no candidate ever won)
            tok_s = ix;
            p.tokens[(size_t)R.seq * p.max_new + R.gen] = ix;
            if (p.eos >= 0 && ix == p.eos) {
                st->done[R.seq] = 1;
                atomicSub(&st->alive, 1);
            }
        }
    }
    __syncthreads();
    if (R.gen + 1 >= p.max_new) return;   // the last token is not fed back
    int tok = tok_s;
    if (p.forced) {
        const int f = p.forced[(size_t)R.seq * p.max_new + R.gen];
        if (f >= 0 && f < p.V) tok = f;
    }
    float* x = p.arena + (size_t)(p.xdec0 + R.seq) * p.D;
    for (int i = tid; i < p.D; i += kLmThreads) x[i] = embed_at(p.embed, p.bf16, (size_t)tok * p.Kp + i);
}

__global__ __launch_bounds__(kLmThreads) void lm_embed_kernel(const void* embed, int bf16, int V, int D, int Kp, const int32_t* ids, const int32_t* xrows, float* arena) {
    const int r = (int)blockIdx.x;
    int tok = ids[r];
    tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;   // (the host has refused ids outside the vocabulary)
    float* x = arena + (size_t)xrows[r] * D;
    for (int i = (int)threadIdx.x; i < D; i += kLmThreads) x[i] = embed_at(embed, bf16, (size_t)tok * Kp + i);
}

int groups_for(int N) { return lm_groups_for(N); }   // row groups per workgroup: about kLmTargetWgs workgroups
int wgs_for(int N) { return lm_wgs_for(N); }

template <int MODE, typename WT, int NB>
void launch_rows_nb(hipStream_t s, const LmRowsP& p, int wgs, size_t lds) {
    if (MODE == LM_PLAIN) {
        OAR_MAX_LDS_ONCE((lm_rows_kernel<NB, WT>), 64 * 1024);
        hipLaunchKernelGGL((lm_rows_kernel<NB, WT>), dim3((unsigned)wgs), dim3(kLmThreads), lds, s, p);
    } else if (MODE == LM_QKV) {
        OAR_MAX_LDS_ONCE((lm_qkv_rows_kernel<NB, WT>), 64 * 1024);
        hipLaunchKernelGGL((lm_qkv_rows_kernel<NB, WT>), dim3((unsigned)wgs), dim3(kLmThreads), lds, s, p);
    } else if (MODE == LM_GATE) {
        OAR_MAX_LDS_ONCE((lm_gate_rows_kernel<NB, WT>), 64 * 1024);
        hipLaunchKernelGGL((lm_gate_rows_kernel<NB, WT>), dim3((unsigned)wgs), dim3(kLmThreads), lds, s, p);
    } else {
        OAR_MAX_LDS_ONCE((lm_head_kernel<NB, WT>), 64 * 1024);
        hipLaunchKernelGGL((lm_head_kernel<NB, WT>), dim3((unsigned)wgs), dim3(kLmThreads), lds, s, p);
    }
}

template <int MODE, typename WT>
void launch_rows_t(hipStream_t s, LmRowsP p, int B, bool prefill) {
    p.Kp = lm_pad4(p.K);
    p.groups = groups_for(p.N);
    const int wgs = wgs_for(p.N);
    if (MODE == LM_HEAD) p.nwg = wgs;
    const size_t lds = lm_rows_lds_bytes(B, p.K);
    const double wbytes = sizeof(WT) * (double)p.N * p.Kp;
    ProfScope ps(s, MODE == LM_HEAD ? (prefill ? "lm_prefill_head" : "lm_head") : (prefill ? "lm_prefill_rows" : "lm_rows"), wbytes + 4.0 * B * ((double)p.K + p.N), 2.0 * (double)p.N * p.K * B);
    switch (lm_nb(B)) {
        case 1: launch_rows_nb<MODE, WT, 1>(s, p, wgs, lds); break;
        case 2: launch_rows_nb<MODE, WT, 2>(s, p, wgs, lds); break;
        case 4: launch_rows_nb<MODE, WT, 4>(s, p, wgs, lds); break;
        case 8: launch_rows_nb<MODE, WT, 8>(s, p, wgs, lds); break;
        default: launch_rows_nb<MODE, WT, 16>(s, p, wgs, lds); break;
    }
}

template <int MODE>
void launch_rows(hipStream_t s, const LmRowsP& p, int B, int bf16, bool prefill) {
    if (bf16) launch_rows_t<MODE, uint16_t>(s, p, B, prefill);
    else launch_rows_t<MODE, float>(s, p, B, prefill);
}

}  // namespace

int lm_head_workgroups(int V) { return wgs_for(V); }

void lm_embed(hipStream_t s, const LmDecodeP& p, const int32_t* ids, const int32_t* xrows, int n) {
    if (n <= 0) return;
    ProfScope ps(s, "lm_embed", 4.0 * 2 * n * p.D, 0);
    hipLaunchKernelGGL(lm_embed_kernel, dim3((unsigned)n), dim3(kLmThreads), 0, s, p.embed, p.bf16, p.V, p.D, lm_pad4(p.D), ids, xrows, p.arena);
}

void lm_attention(hipStream_t s, const LmAttnArgs& g, int attention, int nrows, bool prefill, int max_pos_in_step) {
    if (attention == LM_ATTN_SPLIT) { lm_attention_split(s, g, nrows, prefill, max_pos_in_step); return; }
    const int Hd = g.H * g.dh, Kd = g.KVH * g.dh, G = g.H / g.KVH;
    const int gt = G >= 8 ? 8 : G > 2 ? 4 : G;   // 1, 2, 4 or 8 query heads per workgroup
    const int gchunks = (G + gt - 1) / gt;
    LmAttnP a{};
    a.st = g.st; a.alive = g.alive; a.q = g.q; a.q_ld = g.q_ld; a.kc = g.kc; a.vc = g.vc; a.H = g.H; a.KVH = g.KVH; a.dh = g.dh; a.maxpos = g.maxpos;
    a.scale = 1.0f / sqrtf((float)g.dh); a.o = g.o; a.o_ld = g.o_ld;
    const double keys = (double)nrows * (max_pos_in_step + 1);
    ProfScope ps(s, prefill ? "lm_prefill_attn" : "lm_attn", 4.0 * (2.0 * keys * Kd + 2.0 * nrows * Hd), 4.0 * keys * Hd);
    const dim3 grid((unsigned)g.KVH, (unsigned)nrows, (unsigned)gchunks);
    if (gt == 8) hipLaunchKernelGGL(lm_attn_kernel<8>, grid, dim3(kLmAttnThreads), 0, s, a);
    else if (gt == 4) hipLaunchKernelGGL(lm_attn_kernel<4>, grid, dim3(kLmAttnThreads), 0, s, a);
    else if (gt == 2) hipLaunchKernelGGL(lm_attn_kernel<2>, grid, dim3(kLmAttnThreads), 0, s, a);
    else hipLaunchKernelGGL(lm_attn_kernel<1>, grid, dim3(kLmAttnThreads), 0, s, a);
}

void lm_step(hipStream_t s, const LmDecodeP& p, const LmStep* st, int nrows, int nhead, int max_pos_in_step, int attention) {
    OAR_CHECK(nrows >= 1 && nrows <= kLmRows && nhead >= 0 && nhead <= nrows && lm_head_dim_supported(p.dh) && p.KVH >= 1 && p.H % p.KVH == 0, OAR_INTERNAL,
              "lm_step: rows or head size outside the kernels' limits");
    OAR_CHECK(attention == LM_ATTN_SERIAL || (attention == LM_ATTN_SPLIT && p.split_ws && lm_split_keys_supported(p.split_keys)), OAR_INTERNAL,
              "lm_step: split attention without its workspace or span");
    const int D = p.D, Hd = p.H * p.dh, Kd = p.KVH * p.dh;
    // profiler classes: a step all of whose rows give a token (a decode step; a one-position prompt's prefill is one too) is lm_rows / lm_attn / lm_head / lm_combine,
    // a step with prompt positions that give none is lm_prefill_*: the two can be timed apart
    const bool prefill = nhead < nrows;
    const int* alive = &p.state->alive;
    for (int l = 0; l < p.L; ++l) {
        const LmLayerW& Lw = p.layers[l];
        float* kc = p.kcache + (size_t)l * p.cache_layer;
        float* vc = p.vcache + (size_t)l * p.cache_layer;
        LmRowsP r{};
        r.st = st; r.alive = alive; r.xin = p.arena; r.xin_ld = D; r.xin_arena = 1; r.K = D; r.N = Hd + 2 * Kd; r.W = Lw.w_qkv; r.bias = Lw.b_qkv; r.rms_g = Lw.ln1; r.eps = p.eps;
        r.q = p.q; r.q_ld = Hd; r.kc = kc; r.vc = vc; r.nq = Hd; r.nk = Kd; r.dh = p.dh; r.kvh = p.KVH; r.maxpos = p.maxpos; r.sec0 = p.sec0; r.sec1 = p.sec1; r.inv_freq = p.inv_freq;
        launch_rows<LM_QKV>(s, r, nrows, p.bf16, prefill);
        LmAttnArgs a{};
        a.st = st; a.alive = alive; a.q = p.q; a.q_ld = Hd; a.kc = kc; a.vc = vc; a.H = p.H; a.KVH = p.KVH; a.dh = p.dh; a.maxpos = p.maxpos; a.o = p.o; a.o_ld = Hd;
        a.ws = p.split_ws; a.split_keys = p.split_keys;
        lm_attention(s, a, attention, nrows, prefill, max_pos_in_step);
        r = LmRowsP{};
        r.st = st; r.alive = alive; r.xin = p.o; r.xin_ld = Hd; r.K = Hd; r.N = D; r.W = Lw.w_o; r.y = p.arena; r.y_ld = D;
        launch_rows<LM_PLAIN>(s, r, nrows, p.bf16, prefill);
        r = LmRowsP{};
        r.st = st; r.alive = alive; r.xin = p.arena; r.xin_ld = D; r.xin_arena = 1; r.K = D; r.N = 2 * p.F; r.W = Lw.w_gu; r.rms_g = Lw.ln2; r.eps = p.eps; r.y = p.h; r.y_ld = p.F;
        launch_rows<LM_GATE>(s, r, nrows, p.bf16, prefill);
        r = LmRowsP{};
        r.st = st; r.alive = alive; r.xin = p.h; r.xin_ld = p.F; r.K = p.F; r.N = D; r.W = Lw.w_down; r.y = p.arena; r.y_ld = D;
        launch_rows<LM_PLAIN>(s, r, nrows, p.bf16, prefill);
    }
    if (nhead == 0) return;   // a prefill step that ends no prompt
    LmRowsP r{};
    r.st = st; r.alive = alive; r.xin = p.arena; r.xin_ld = D; r.xin_arena = 1; r.K = D; r.N = p.V; r.W = p.w_lm; r.rms_g = p.lnf; r.eps = p.eps;
    r.logits = p.logits; r.max_new = p.max_new; r.part = reinterpret_cast<float2*>(p.part);
    if (p.select) {   // logits processors: the lm-head also fills the step buffer, lm_select leaves one candidate per row
        lm_head_step(s, p, st, nhead, prefill);
        LmSelectP q{};
        q.st = st; q.state = p.state; q.logits = p.step_logits; q.ld = lm_select_ld(p.V); q.V = p.V; q.words = lm_select_words(p.V); q.hist = p.hist; q.cap = p.hist_cap;
        q.hlen = p.hlen; q.seen = p.seen; q.tokens = p.tokens; q.forced = p.forced; q.max_new = p.max_new; q.penalty = p.penalty; q.ngram = p.ngram; q.part = p.part1;
        lm_select(s, q, nhead, prefill);
    } else {
        launch_rows<LM_HEAD>(s, r, nhead, p.bf16, prefill);
    }
    LmCombineP c{};
    c.st = st; c.part = reinterpret_cast<const float2*>(p.select ? p.part1 : p.part); c.nwg = p.select ? 1 : wgs_for(p.V); c.V = p.V; c.D = D; c.Kp = lm_pad4(D); c.bf16 = p.bf16; c.embed = p.embed;
    c.arena = p.arena; c.xdec0 = p.xdec0; c.state = p.state; c.tokens = p.tokens; c.forced = p.forced; c.max_new = p.max_new; c.eos = p.eos;
    {
        ProfScope ps(s, prefill ? "lm_prefill_combine" : "lm_combine", 4.0 * nhead * (2.0 * c.nwg + 2.0 * D), 0);
        hipLaunchKernelGGL(lm_combine_kernel, dim3((unsigned)nhead), dim3(kLmThreads), 0, s, c);
    }
}

}  // namespace k
}  // namespace oar
