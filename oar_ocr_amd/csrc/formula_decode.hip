// formula_decode.hip -- the greedy autoregressive decode of a PP-FormulaNet-style head (an MBart-order, pre-norm transformer decoder with a
// key / value cache) as a fixed chain of short launches per step.  The engine's Loop rewrite (engine_loops.cc, match_formula_loop) emits it.
//
// A decode step at batch <= 16 is weight streaming: every matrix is read once per step for the whole batch, across all CUs, and a kernel
// boundary is the all-to-all seam each LayerNorm / GEMV pair needs.  There is no grid-wide barrier and no flag in global memory: nothing here
// ever waits on another workgroup.  Per step (t = 0 .. M-1) and chunk of <= 16 images, 8 Ld + 2 launches:
//   per layer   1 fd_rows        LN1 -> [Wq ; Wk ; Wv] (one stacked matrix): q to its row buffer, k / v straight into the cache at position t
//                                (squeeze attention: Wq / Wk have Dq = nh dq rows, 1 <= dq <= 128 whatever dh is, the key cache is dq wide per head, the value cache dh)
//               2 fd_self_attn   softmax(q K'^T) V' over the t + 1 cached positions, one workgroup per (image, head)
//               3 fd_rows        Wo + bias + residual
//               4 fd_rows        LN2 -> Wcq (the query scale where the graph had it)
//               5 fd_cross_attn  softmax(qc KmT) Vm over the S memory positions
//               6 fd_rows        Wco + bias + residual
//               7 fd_rows        LN3 -> W1 + bias -> GELU (erf form of ACT_GELU_ERF)
//               8 fd_rows        W2 + bias + residual
//   then        9 fd_lm_head     LN_f -> W_lm (+ bias): logits (when declared) and one (value, index) partial per workgroup and image
//              10 fd_combine     lowest index among equal values -> the token (scan output + state) and the NEXT step's input row
//                                LN_emb(E_tok[tok] * s_emb + E_pos[t + 1 + c_pos]): the embedding costs no launch of its own
// One more fd_combine launch per chunk embeds the start token before step 0 (profiler class formula_embed).
//
// Stop token (opt-in, FormulaDecodeP::stop; off = every pointer below is null and nothing here differs from the chain above).  Per chunk the engine keeps
// FdStopState in device memory of its own: done[b] (0 while image b decodes, f + 1 once it emitted the stop token at step f), alive (images still decoding)
// and a 64-bit count of executed steps.  fd_combine is the only writer: it forces the stop token for a finished image (as scan output AND as the next input),
// marks an image that has just emitted it and takes it off `alive` with one atomicSub.  Every other kernel of the chain reads `alive` before it touches
// anything and returns when it is 0 -- the kernel boundary after fd_combine orders the write.  The workgroup that brings `alive` to 0 also stores the
// chunk's generation number into a word of mapped host memory; the host, which waits on the event recorded kFdLookahead steps back before it enqueues
// a step (so at most t_stop + kFdLookahead steps of a chunk are enqueued), stops enqueuing once it reads its own generation there, and fd_fill_tail writes the stop token into the rows that were never enqueued.  While a
// hipGraph is captured the host reads nothing: all M steps are enqueued and the guards alone skip the work.
//
// fd_rows: y[B][N] = epi(LN?(x[B][K]) W^T + b).  A workgroup of 4 waves owns a slice of W's rows; it stages the B input rows in LDS in chunks of
// 768 columns (48 KB at 16 rows: two workgroups per CU), applying the LayerNorm itself (the row statistics come from a two-pass prologue over the
// B x K inputs, L2 resident), and streams its weight rows once with 16-byte loads: a wave takes two rows at a time, every lane multiplies its float4
// of each row with the matching float4 of all B staged inputs, and the 2 B sums are reduced across the wave with shuffles.  Weight rows are padded to
// a multiple of four floats at rewrite time.  f32 throughout; fmaf only inside the dot products.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "kernels_dev.h"

namespace oar {
namespace k {

namespace {

constexpr int kFdThreads = 256, kFdWaves = kFdThreads / 64, kFdR = 2, kFdKC = 768, kFdTargetWgs = 512;
constexpr int kFdAttnThreads = 256;

enum : int { FD_PLAIN = 0, FD_QKV = 1, FD_LM = 2 };

struct FdRowsP {
    const float* x; int x_ld;            // [B][K] inputs, row stride x_ld
    int B, K, N, Kp;                     // Kp: weight row stride (K rounded up to 4)
    const float* W; const float* bias;   // [N][Kp], [N] or null
    const float *ln_g, *ln_b; float eps; // LayerNorm prologue over K when ln_g != null
    int groups;                          // row groups (of kFdWaves * kFdR rows) per workgroup
    float* y; int y_ld;                  // FD_PLAIN / FD_QKV (rows < D): y[b][n]
    const float* res;                    // residual [B][y_ld] or null (may alias y)
    int gelu;
    int scale_mode; float scale; int scale_rows;   // rows < scale_rows: 1 = (v + b) * s, 2 = v * s + b
    float *kc, *vc; int Dq, dq, dh, nh, M, t;   // FD_QKV: rows [Dq, 2Dq) -> kc[b][head][t][dq], [2Dq, 2Dq + D) -> vc[b][head][t][dh]
    float* logits;                       // FD_LM: [B][N] or null
    float2* part; int nwg;               // FD_LM: part[b][workgroup] = (value, index)
    const int* alive;                    // stop token on: images of the chunk still decoding (0: return at once); null: off
};

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ bool better(float ov, int oi, float v, int ix) { return ov > v || (ov == v && oi < ix); }

template <int NB, int MODE>
__device__ __forceinline__ void fd_rows_body(const FdRowsP& p) {
    extern __shared__ float4 fd_lds4[];
    __shared__ float mean_s[16], rstd_s[16];
    __shared__ float red_v[kFdWaves][16];
    __shared__ int red_i[kFdWaves][16];
    float* xs = reinterpret_cast<float*>(fd_lds4);
    if (p.alive && *p.alive == 0) return;   // (uniform over the grid: only fd_combine writes it)
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int KCs = p.Kp < kFdKC ? p.Kp : kFdKC;
    const bool ln = p.ln_g != nullptr;
    if (ln) {
        for (int b = wave; b < NB; b += kFdWaves) {
            if (b < p.B) {
                const float* xr = p.x + (size_t)b * p.x_ld;
                float s = 0.0f;
                for (int i = lane; i < p.K; i += 64) s += xr[i];
                const float mean = wave_sum(s) / (float)p.K;
                float v = 0.0f;
                for (int i = lane; i < p.K; i += 64) { const float d = xr[i] - mean; v += d * d; }
                const float var = wave_sum(v) / (float)p.K;
                if (lane == 0) { mean_s[b] = mean; rstd_s[b] = 1.0f / sqrtf(var + p.eps); }
            }
        }
    }
    const int nchunks = (p.Kp + kFdKC - 1) / kFdKC;
    const int row0 = (int)blockIdx.x * p.groups * kFdWaves * kFdR;
    float bv[NB];
    int bi[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { bv[b] = -INFINITY; bi[b] = 0x7fffffff; }
    for (int rg = 0; rg < p.groups; ++rg) {
        const int rbase = row0 + (rg * kFdWaves + wave) * kFdR;
        float acc[kFdR][NB];
#pragma unroll
        for (int r = 0; r < kFdR; ++r)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[r][b] = 0.0f;
        for (int c = 0; c < nchunks; ++c) {
            const int k0 = c * kFdKC, kc = (p.Kp - k0) < kFdKC ? (p.Kp - k0) : kFdKC;
            if (nchunks > 1 || rg == 0) {
                __syncthreads();   // (the statistics are written / the previous chunk has been read)
                for (int i = tid; i < NB * kc; i += kFdThreads) {
                    const int b = i / kc, kk = i - b * kc, gk = k0 + kk;
                    float v = 0.0f;
                    if (b < p.B && gk < p.K) {
                        v = p.x[(size_t)b * p.x_ld + gk];
                        if (ln) v = (v - mean_s[b]) * rstd_s[b] * p.ln_g[gk] + p.ln_b[gk];
                    }
                    xs[b * KCs + kk] = v;
                }
                __syncthreads();
            }
            const float4* xv = reinterpret_cast<const float4*>(xs);
            const int kc4 = kc >> 2, ks4 = KCs >> 2;
            for (int q = lane; q < kc4; q += 64) {
                float4 w[kFdR];
#pragma unroll
                for (int r = 0; r < kFdR; ++r) {
                    const int row = rbase + r;
                    w[r] = row < p.N ? reinterpret_cast<const float4*>(p.W + (size_t)row * p.Kp + k0)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float4 v = xv[b * ks4 + q];
#pragma unroll
                    for (int r = 0; r < kFdR; ++r) {
                        float a = acc[r][b];
                        a = fmaf(w[r].x, v.x, a); a = fmaf(w[r].y, v.y, a); a = fmaf(w[r].z, v.z, a); a = fmaf(w[r].w, v.w, a);
                        acc[r][b] = a;
                    }
                }
            }
        }
        // every lane ends up with all sums; lane r * NB + b finishes output (row rbase + r, image b)
        float mine = 0.0f;
#pragma unroll
        for (int r = 0; r < kFdR; ++r)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float s = wave_sum(acc[r][b]);
                if (lane == r * NB + b) mine = s;
                acc[r][b] = s;
            }
        const int er = lane / NB, eb = lane - er * NB, row = rbase + er;
        const bool live = lane < kFdR * NB && eb < p.B && row < p.N;
        if (MODE == FD_LM) {
#pragma unroll
            for (int r = 0; r < kFdR; ++r) {
                const int rr = rbase + r;
                if (rr < p.N) {
                    const float bias = p.bias ? p.bias[rr] : 0.0f;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const float v = p.bias ? acc[r][b] + bias : acc[r][b];
                        if (v > bv[b]) { bv[b] = v; bi[b] = rr; }   // a wave's rows only grow: the first maximum stays
                    }
                }
            }
            if (live && p.logits) p.logits[(size_t)eb * p.N + row] = p.bias ? mine + p.bias[row] : mine;
        } else if (live) {
            float v = mine;
            const float bias = p.bias ? p.bias[row] : 0.0f;
            const int sm = row < p.scale_rows ? p.scale_mode : 0;
            if (sm == 2) v = v * p.scale;
            if (p.bias) v = v + bias;
            if (sm == 1) v = v * p.scale;
            if (p.gelu) v = apply_act(v, ACT_GELU_ERF, 0.f, 0.f);
            if (MODE == FD_QKV && row >= p.Dq) {
                const int which = row >= 2 * p.Dq, n = row - (which ? 2 : 1) * p.Dq, w = which ? p.dh : p.dq, head = n / w, d = n - head * w;
                float* cache = which ? p.vc : p.kc;
                cache[(((size_t)eb * p.nh + head) * p.M + p.t) * w + d] = v;
            } else {
                if (p.res) v = p.res[(size_t)eb * p.y_ld + row] + v;
                p.y[(size_t)eb * p.y_ld + row] = v;
            }
        }
    }
    if (MODE == FD_LM) {
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) { red_v[wave][b] = bv[b]; red_i[wave][b] = bi[b]; }
        }
        __syncthreads();
        if (tid < NB && tid < p.B) {
            float v = red_v[0][tid];
            int ix = red_i[0][tid];
            for (int w = 1; w < kFdWaves; ++w)
                if (better(red_v[w][tid], red_i[w][tid], v, ix)) { v = red_v[w][tid]; ix = red_i[w][tid]; }
            p.part[(size_t)tid * p.nwg + blockIdx.x] = make_float2(v, __int_as_float(ix));
        }
    }
}

template <int NB>
__global__ __launch_bounds__(kFdThreads) void fd_rows_kernel(FdRowsP p) { fd_rows_body<NB, FD_PLAIN>(p); }
template <int NB>
__global__ __launch_bounds__(kFdThreads) void fd_qkv_rows_kernel(FdRowsP p) { fd_rows_body<NB, FD_QKV>(p); }
template <int NB>
__global__ __launch_bounds__(kFdThreads) void fd_lm_head_kernel(FdRowsP p) { fd_rows_body<NB, FD_LM>(p); }

// softmax(q K^T) V of one (image, head): key element (j, d) at kb[j * ks_j + d * ks_d], d < dq (the q . k width); value row j at vb + j * dh; n positions.
// q is [B][nh dq] within rows of q_ld floats, o is [B][nh dh].  Both widths are run-time fields: squeeze attention (dq < dh) runs the same code object
struct FdAttnP {
    const float* q; int q_ld;            // [B][D]
    const float *kb, *vb;                // image 0, head 0
    size_t k_img, k_head, v_img, v_head; // strides in floats
    int ks_j, ks_d, n, dq, dh;
    float* o; int o_ld;                  // [B][D]
    const int* alive;                    // as FdRowsP::alive
};

__device__ __forceinline__ void fd_attn_body(const FdAttnP& p) {
    __shared__ float qs[kFdMaxDh];
    __shared__ float sc[kFdMaxS];
    __shared__ float part[kFdAttnThreads];
    __shared__ float red[kFdAttnThreads / 64];
    if (p.alive && *p.alive == 0) return;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, head = (int)blockIdx.x, b = (int)blockIdx.y;
    const int n = p.n, dq = p.dq, dh = p.dh;
    const float* kb = p.kb + (size_t)b * p.k_img + (size_t)head * p.k_head;
    const float* vb = p.vb + (size_t)b * p.v_img + (size_t)head * p.v_head;
    if (tid < dq) qs[tid] = p.q[(size_t)b * p.q_ld + head * dq + tid];
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < n; j += kFdAttnThreads) {
        float a = 0.0f;
        const float* kr = kb + (size_t)j * p.ks_j;
        for (int d = 0; d < dq; ++d) a = fmaf(qs[d], kr[(size_t)d * p.ks_d], a);
        sc[j] = a;
        m = fmaxf(m, a);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < kFdAttnThreads / 64; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    float s = 0.0f;
    for (int j = tid; j < n; j += kFdAttnThreads) { const float e = expf(sc[j] - m); sc[j] = e; s += e; }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = red[0];
    for (int w = 1; w < kFdAttnThreads / 64; ++w) s += red[w];
    for (int j = tid; j < n; j += kFdAttnThreads) sc[j] = sc[j] / s;
    __syncthreads();
    // weighted sum of the value rows: G groups of dhp threads take every G-th position, summed in group order
    int dhp = 1;
    while (dhp < dh) dhp <<= 1;
    const int G = kFdAttnThreads / dhp, g = tid / dhp, d = tid & (dhp - 1);
    float a = 0.0f;
    if (d < dh)
        for (int j = g; j < n; j += G) a = fmaf(sc[j], vb[(size_t)j * dh + d], a);
    part[tid] = a;
    __syncthreads();
    if (tid < dh) {
        float r = part[tid];
        for (int w = 1; w < G; ++w) r += part[w * dhp + tid];
        p.o[(size_t)b * p.o_ld + head * dh + tid] = r;
    }
}
__global__ __launch_bounds__(kFdAttnThreads) void fd_self_attn_kernel(FdAttnP p) { fd_attn_body(p); }
__global__ __launch_bounds__(kFdAttnThreads) void fd_cross_attn_kernel(FdAttnP p) { fd_attn_body(p); }

struct FdCombineP {
    const float2* part; int nwg;         // null: the token comes from tok_in (the start token)
    const float* tok_in;                 // [B] f32-coded
    float* tok_out;                      // scan output row of this step, [B] f32-coded (null for the start token)
    int V, D, pos;                       // pos >= 0: also write x = LN_emb(E_tok[tok] * s_emb + E_pos[pos])
    const float *e_tok, *e_pos, *ln_g, *ln_b;
    float s_emb, eps;
    float* x;                            // [B][D]
    FdStopState* st;                     // stop token on (null: off).  Start-token launch: reset the chunk's state; step launch: see the header
    int stop_tok, t;                     // the stop token; this launch's step
    int reset_count;                     // start-token launch of a run's first chunk: steps_executed = 0
    unsigned* fin_host; unsigned gen;    // mapped host word that receives `gen` once the chunk has finished (null while capturing)
};

__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = (int)threadIdx.x;
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < kFdThreads / 64; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(kFdThreads) void fd_combine_kernel(FdCombineP p) {
    __shared__ float red_v[kFdWaves];
    __shared__ int red_i[kFdWaves];
    __shared__ float red[kFdWaves];
    __shared__ int tok_s;
    __shared__ int skip_s, done_s;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, b = (int)blockIdx.x;
    FdStopState* st = p.st;
    if (st && !p.part) {   // start token: a new chunk
        if (tid == 0) {
            __atomic_store_n(&st->done[b], 0, __ATOMIC_RELAXED);
            if (b == 0) {
                st->alive = (int)gridDim.x;
                if (p.reset_count) st->steps_executed = 0;
            }
        }
    } else if (st) {
        if (tid == 0) {
            // done[] holds f + 1, so an image that finishes in this very launch (another workgroup may already have said so) still counts as decoding on
            // entry: the step is counted exactly when at least one image entered it alive, whatever the order of the workgroups
            if (b == 0) {
                bool any = false;
                for (int j = 0; j < (int)gridDim.x; ++j) {
                    const int d = __atomic_load_n(&st->done[j], __ATOMIC_RELAXED);
                    any = any || d == 0 || d == p.t + 1;
                }
                if (any) st->steps_executed = st->steps_executed + 1;
            }
            done_s = __atomic_load_n(&st->done[b], __ATOMIC_RELAXED);   // (only this workgroup writes done[b]; workgroup 0 may read it meanwhile)
            // 0 here means every image has finished, this one included (it has not left `alive` in this launch before this read): nothing is left to do
            skip_s = __atomic_load_n(&st->alive, __ATOMIC_RELAXED) == 0;
        }
        __syncthreads();
        if (skip_s || done_s) {
            if (tid == 0) { tok_s = p.stop_tok; p.tok_out[b] = (float)p.stop_tok; }
            if (skip_s) return;
        }
    }
    if (p.part && !(st && done_s)) {
        float v = -INFINITY;
        int ix = 0x7fffffff;
        for (int i = tid; i < p.nwg; i += kFdThreads) {
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
            for (int w = 1; w < kFdWaves; ++w)
                if (better(red_v[w], red_i[w], v, ix)) { v = red_v[w]; ix = red_i[w]; }
            if (ix < 0 || ix >= p.V) ix = 0;   // (all logits NaN: no candidate ever won)
            tok_s = ix;
            p.tok_out[b] = (float)ix;
            if (st && ix == p.stop_tok) {
                __atomic_store_n(&st->done[b], p.t + 1, __ATOMIC_RELAXED);
                if (atomicSub(&st->alive, 1) == 1 && p.fin_host) {   // the chunk's last image: tell the host (visible at the latest when this launch ends)
                    __atomic_store_n(p.fin_host, p.gen, __ATOMIC_RELAXED);
                    __threadfence_system();
                }
            }
        }
    } else if (!p.part && tid == 0) {
        int ix = (int)p.tok_in[b];
        tok_s = ix < 0 ? 0 : ix >= p.V ? p.V - 1 : ix;
    }
    __syncthreads();
    if (p.pos < 0) return;
    const int tok = tok_s, D = p.D;
    const float* et = p.e_tok + (size_t)tok * D;
    const float* ep = p.e_pos + (size_t)p.pos * D;
    float e[kFdMaxD / kFdThreads];
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < kFdMaxD / kFdThreads; ++q) {
        const int i = tid + q * kFdThreads;
        e[q] = i < D ? et[i] * p.s_emb + ep[i] : 0.0f;
        s += e[q];
    }
    const float mean = block_sum(s, red) / (float)D;
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < kFdMaxD / kFdThreads; ++q) {
        const int i = tid + q * kFdThreads;
        const float d = i < D ? e[q] - mean : 0.0f;
        v += d * d;
    }
    const float rstd = 1.0f / sqrtf(block_sum(v, red) / (float)D + p.eps);
#pragma unroll
    for (int q = 0; q < kFdMaxD / kFdThreads; ++q) {
        const int i = tid + q * kFdThreads;
        if (i < D) p.x[(size_t)b * D + i] = (e[q] - mean) * rstd * p.ln_g[i] + p.ln_b[i];
    }
}

// rows [t0, M) of a chunk's token columns: the steps the host never enqueued read the stop token
__global__ __launch_bounds__(kFdThreads) void fd_fill_tail_kernel(float* tok, int ld, int bc, int t0, int M, float v) {
    const int n = (M - t0) * bc;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) {
        const int r = i / bc, b = i - r * bc;
        tok[(size_t)(t0 + r) * ld + b] = v;
    }
}

int pad4i(int n) { return (n + 3) & ~3; }
int groups_for(int N) {   // row groups per workgroup: about kFdTargetWgs workgroups
    const int per = kFdWaves * kFdR;
    return std::max(1, (N + per * kFdTargetWgs - 1) / (per * kFdTargetWgs));
}
int wgs_for(int N) { const int rows = groups_for(N) * kFdWaves * kFdR; return (N + rows - 1) / rows; }

template <int MODE>
void launch_rows(hipStream_t s, FdRowsP p) {
    p.Kp = pad4i(p.K);
    p.groups = groups_for(p.N);
    const int wgs = wgs_for(p.N);
    if (MODE == FD_LM) p.nwg = wgs;
    int nb = 1;
    while (nb < p.B) nb <<= 1;
    const size_t lds = (size_t)nb * (size_t)std::min(p.Kp, kFdKC) * 4;
    ProfScope ps(s, "formula_decode", 4.0 * ((double)p.N * p.Kp + (double)p.B * (p.K + p.N)), 2.0 * (double)p.N * p.K * p.B);
#define OAR_FD_LAUNCH(NB)                                                                                                              \
    do {                                                                                                                               \
        if (MODE == FD_PLAIN) hipLaunchKernelGGL(fd_rows_kernel<NB>, dim3((unsigned)wgs), dim3(kFdThreads), lds, s, p);                 \
        else if (MODE == FD_QKV) hipLaunchKernelGGL(fd_qkv_rows_kernel<NB>, dim3((unsigned)wgs), dim3(kFdThreads), lds, s, p);          \
        else hipLaunchKernelGGL(fd_lm_head_kernel<NB>, dim3((unsigned)wgs), dim3(kFdThreads), lds, s, p);                              \
    } while (0)
    switch (nb) {
        case 1: OAR_FD_LAUNCH(1); break;
        case 2: OAR_FD_LAUNCH(2); break;
        case 4: OAR_FD_LAUNCH(4); break;
        case 8: OAR_FD_LAUNCH(8); break;
        default: OAR_FD_LAUNCH(16); break;
    }
#undef OAR_FD_LAUNCH
}

}  // namespace

bool formula_decode_supported(int D, int nh, int F, int V, int Ld, int M, int S, int dq) {
    return nh >= 1 && D >= nh && D % nh == 0 && D <= kFdMaxD && D / nh <= kFdMaxDh && dq >= 1 && dq <= kFdMaxDh && nh * dq <= kFdMaxD && F >= 1 && F <= kFdMaxF && Ld >= 1 && Ld <= kFdMaxLayers && V >= 2 && V < kFdMaxV &&
           M >= 1 && M <= kFdMaxM && S >= 1 && S <= kFdMaxS;
}
int formula_decode_lm_workgroups(int V) { return wgs_for(V); }
int formula_decode_launches_per_step(int Ld) { return 8 * Ld + 2; }

size_t formula_decode_ws_floats(int B, int D, int F, int V, int Ld, int M, int Dq) {
    const size_t bc = (size_t)std::min(B, kFdChunk);
    // caches (keys Dq wide, values D) | x o [bc][D] each, q [bc][max(D, Dq)] | h [bc][F] | tok [bc] | partials [bc][wgs] float2
    return (size_t)Ld * bc * (size_t)M * ((size_t)Dq + D) + 2 * bc * D + bc * (size_t)std::max(D, Dq) + bc * (size_t)F + 16 + 2 * bc * (size_t)wgs_for(V) + 16;
}

void formula_decode(hipStream_t s, const FormulaDecodeP& p) {
    const int D = p.D, nh = p.nh, dh = D / nh, dq = p.dq, Dq = nh * dq, F = p.F, V = p.V, Ld = p.Ld, M = p.M, S = p.S;
    OAR_CHECK(formula_decode_supported(D, nh, F, V, Ld, M, S, dq) && p.c_pos >= 0 && (int64_t)M + p.c_pos <= p.P, OAR_UNSUPPORTED_OP, "FormulaDecode: shape outside the kernels' limits");
    if (p.B <= 0) return;
    const int bc_max = std::min(p.B, kFdChunk);
    const size_t kcache_l = (size_t)bc_max * M * Dq, vcache_l = (size_t)bc_max * M * D;   // one layer's caches: K [bc][nh][M][dq], V [bc][nh][M][dh]
    float* kc0 = p.ws;
    float* x = kc0 + (size_t)Ld * (kcache_l + vcache_l);
    const int q_ld = std::max(D, Dq);   // the row buffer of the self-attention query (Dq wide; dq may exceed dh) and of the cross-attention query (D wide)
    float* q = x + (size_t)bc_max * D;
    float* o = q + (size_t)bc_max * q_ld;
    float* h = o + (size_t)bc_max * D;
    const size_t part_off = ((size_t)(h - p.ws) + (size_t)bc_max * F + 1) & ~(size_t)1;   // 8-byte aligned (ws is)
    float2* part = reinterpret_cast<float2*>(p.ws + part_off);
    FdStop* const stop = p.stop;
    OAR_CHECK(!stop || (stop->token >= 0 && stop->token < V && stop->state), OAR_INTERNAL, "FormulaDecode: stop token without its state");
    const bool poll = stop && !Profiler::capturing;   // (a captured graph reads nothing back: the device guards alone skip the work)
    const int* const alive = stop ? &stop->state->alive : nullptr;
    constexpr int kRing = kFdLookahead + 1;
    for (int c0 = 0; c0 < p.B; c0 += kFdChunk) {
        const int bc = std::min(kFdChunk, p.B - c0);
        FdCombineP cb{};
        cb.V = V; cb.D = D; cb.e_tok = p.e_tok; cb.e_pos = p.e_pos; cb.ln_g = p.lne_g; cb.ln_b = p.lne_b; cb.s_emb = p.s_emb; cb.eps = p.eps_e; cb.x = x;
        if (stop) {
            if (++stop->gen == 0) stop->gen = 1;
            cb.st = stop->state; cb.stop_tok = stop->token; cb.gen = stop->gen; cb.fin_host = poll ? stop->fin_dev : nullptr;
        }
        {
            FdCombineP c = cb;
            c.tok_in = p.tok0 + c0; c.pos = p.c_pos;
            if (stop) { c.reset_count = stop->first_chunk ? 1 : 0; stop->first_chunk = false; }
            ProfScope ps(s, "formula_embed", 4.0 * 3 * bc * D, 0);
            hipLaunchKernelGGL(fd_combine_kernel, dim3((unsigned)bc), dim3(kFdThreads), 0, s, c);
        }
        int t = 0;
        for (; t < M; ++t) {
            if (poll && t >= kFdLookahead) {   // steps 0 .. t - kFdLookahead have ended: did the last image finish in one of them?
                OAR_HIP(hipEventSynchronize(stop->ev[(t - kFdLookahead) % kRing]));
                if (*stop->fin == stop->gen) break;
            }
            for (int l = 0; l < Ld; ++l) {
                const FdLayerP& L = p.layer[l];
                float* kc = kc0 + (size_t)l * (kcache_l + vcache_l);
                float* vc = kc + kcache_l;
                FdRowsP r{};
                r.x = x; r.x_ld = D; r.B = bc; r.K = D; r.N = 2 * Dq + D; r.W = L.w_qkv; r.bias = L.b_qkv; r.ln_g = L.ln1_g; r.ln_b = L.ln1_b; r.eps = L.eps1;
                r.y = q; r.y_ld = q_ld; r.scale_mode = L.q_scale_mode; r.scale = L.q_scale; r.scale_rows = Dq; r.kc = kc; r.vc = vc; r.Dq = Dq; r.dq = dq; r.dh = dh; r.nh = nh; r.M = M; r.t = t;
                r.alive = alive; launch_rows<FD_QKV>(s, r);
                FdAttnP a{};
                a.q = q; a.q_ld = q_ld; a.kb = kc; a.vb = vc; a.k_img = (size_t)M * Dq; a.v_img = (size_t)M * D; a.k_head = (size_t)M * dq; a.v_head = (size_t)M * dh; a.ks_j = dq; a.ks_d = 1; a.n = t + 1;
                a.dq = dq; a.dh = dh;
                a.o = o; a.o_ld = D; a.alive = alive;
                {
                    ProfScope ps(s, "formula_decode", 4.0 * bc * ((double)(t + 1) * (Dq + D) + Dq + D), 2.0 * bc * (double)(t + 1) * (Dq + D));
                    hipLaunchKernelGGL(fd_self_attn_kernel, dim3((unsigned)nh, (unsigned)bc), dim3(kFdAttnThreads), 0, s, a);
                }
                r = FdRowsP{};
                r.x = o; r.x_ld = D; r.B = bc; r.K = D; r.N = D; r.W = L.w_o; r.bias = L.b_o; r.y = x; r.y_ld = D; r.res = x;
                r.alive = alive; launch_rows<FD_PLAIN>(s, r);
                r = FdRowsP{};
                r.x = x; r.x_ld = D; r.B = bc; r.K = D; r.N = D; r.W = L.w_cq; r.bias = L.b_cq; r.ln_g = L.ln2_g; r.ln_b = L.ln2_b; r.eps = L.eps2;
                r.y = q; r.y_ld = q_ld; r.scale_mode = L.cq_scale_mode; r.scale = L.cq_scale; r.scale_rows = D;
                r.alive = alive; launch_rows<FD_PLAIN>(s, r);
                a = FdAttnP{};
                a.q = q; a.q_ld = q_ld; a.kb = L.kmT + (size_t)c0 * D * S; a.vb = L.vm + (size_t)c0 * D * S; a.k_img = a.v_img = (size_t)D * S; a.k_head = a.v_head = (size_t)dh * S;
                a.ks_j = 1; a.ks_d = S; a.n = S; a.dq = dh; a.dh = dh; a.o = o; a.o_ld = D; a.alive = alive;
                {
                    ProfScope ps(s, "formula_decode", 4.0 * bc * (2.0 * S * D + 2 * D), 4.0 * bc * (double)S * D);
                    hipLaunchKernelGGL(fd_cross_attn_kernel, dim3((unsigned)nh, (unsigned)bc), dim3(kFdAttnThreads), 0, s, a);
                }
                r = FdRowsP{};
                r.x = o; r.x_ld = D; r.B = bc; r.K = D; r.N = D; r.W = L.w_co; r.bias = L.b_co; r.y = x; r.y_ld = D; r.res = x;
                r.alive = alive; launch_rows<FD_PLAIN>(s, r);
                r = FdRowsP{};
                r.x = x; r.x_ld = D; r.B = bc; r.K = D; r.N = F; r.W = L.w_1; r.bias = L.b_1; r.ln_g = L.ln3_g; r.ln_b = L.ln3_b; r.eps = L.eps3; r.y = h; r.y_ld = F; r.gelu = 1;
                r.alive = alive; launch_rows<FD_PLAIN>(s, r);
                r = FdRowsP{};
                r.x = h; r.x_ld = F; r.B = bc; r.K = F; r.N = D; r.W = L.w_2; r.bias = L.b_2; r.y = x; r.y_ld = D; r.res = x;
                r.alive = alive; launch_rows<FD_PLAIN>(s, r);
            }
            FdRowsP r{};
            r.x = x; r.x_ld = D; r.B = bc; r.K = D; r.N = V; r.W = p.w_lm; r.bias = p.b_lm; r.ln_g = p.lnf_g; r.ln_b = p.lnf_b; r.eps = p.eps_f;
            r.logits = p.logits ? p.logits + ((size_t)t * p.B + c0) * V : nullptr; r.part = part;
            r.alive = alive; launch_rows<FD_LM>(s, r);
            FdCombineP c = cb;
            c.part = part; c.nwg = wgs_for(V); c.tok_out = p.tokens + (size_t)t * p.B + c0; c.pos = t + 1 < M ? t + 1 + p.c_pos : -1;
            c.t = t;
            {
                ProfScope ps(s, "formula_decode", 4.0 * bc * (2.0 * c.nwg + 3.0 * D), 0);
                hipLaunchKernelGGL(fd_combine_kernel, dim3((unsigned)bc), dim3(kFdThreads), 0, s, c);
            }
            if (poll) OAR_HIP(hipEventRecord(stop->ev[t % kRing], s));
        }
        if (p.stats) { p.stats->steps_limit += M; p.stats->steps_enqueued += t; }
        if (t < M) {   // (only ever with the stop token on)
            const int n = (M - t) * bc;
            ProfScope ps(s, "formula_stop", 4.0 * n, 0);
            hipLaunchKernelGGL(fd_fill_tail_kernel, dim3((unsigned)std::min((n + kFdThreads - 1) / kFdThreads, 64)), dim3(kFdThreads), 0, s, p.tokens + c0, p.B, bc, t, M,
                               (float)stop->token);
        }
    }
}

}  // namespace k
}  // namespace oar
