// lm_rows_dev.h -- the body of the rows / lm-head kernels of the language-model chain, for the translation units that instantiate it: lm_decode.hip (the chain's
// own kernels) and lm_logits.hip (the lm-head that also fills the step logits buffer).  Device code: include it from a .hip file only.
#pragma once
#include "common.h"
#include "lm_decode.h"

namespace oar {
namespace k {

namespace {

enum : int { LM_PLAIN = 0, LM_QKV = 1, LM_GATE = 2, LM_HEAD = 3, LM_HEAD_STEP = 4 };   // LM_HEAD_STEP: LM_HEAD, and row b's logits also go to y[head[b]][n]

struct LmRowsP {
    const LmStep* st;
    const float* xin; int xin_ld; int xin_arena;   // row b's input: xin + (xin_arena ? rows[b].xrow : b) * xin_ld
    int K, N, Kp;
    const void* W; const float* bias;              // [N][Kp] f32 or bf16; [N] or null
    const float* rms_g; float eps;                 // RMSNorm prologue over K when rms_g != null
    int groups;
    float* y; int y_ld;                            // LM_PLAIN: arena (y[xrow][n] += v); LM_GATE: y[b][n / 2]; LM_HEAD_STEP: the step logits buffer
    float *q, *kc, *vc; int q_ld, nq, nk, dh, kvh, maxpos, sec0, sec1;   // LM_QKV: rows < nq -> q, < nq + nk -> kc, the rest -> vc
    const float* inv_freq;
    float* logits; int max_new;                    // LM_HEAD
    float2* part; int nwg;
    const int* alive;
};

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ bool better(float ov, int oi, float v, int ix) { return ov > v || (ov == v && oi < ix); }

__device__ __forceinline__ float4 load_w4(const float* w, int q) { return reinterpret_cast<const float4*>(w)[q]; }
__device__ __forceinline__ float4 load_w4(const uint16_t* w, int q) {   // four bf16 -> f32, exact
    const uint2 u = reinterpret_cast<const uint2*>(w)[q];
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}

template <int NB, int MODE, typename WT>
__device__ __forceinline__ void lm_rows_body(const LmRowsP& p) {
    extern __shared__ float4 lm_lds4[];
    __shared__ float rstd_s[16];
    __shared__ float red_v[kLmWaves][16];
    __shared__ int red_i[kLmWaves][16];
    constexpr bool HEAD = MODE == LM_HEAD || MODE == LM_HEAD_STEP;
    float* xs = reinterpret_cast<float*>(lm_lds4);
    if (*p.alive == 0) return;   // (uniform over the grid: only lm_combine writes it)
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const LmStep* st = p.st;
    const int B = HEAD ? st->nhead : st->nrows;
    const int KCs = p.Kp < kLmKC ? p.Kp : kLmKC;
    const bool rms = p.rms_g != nullptr;
    // RMSNorm: x g is staged, the sum of squares is gathered while staging (thread t always takes the same float4s of a row, whatever the row's slot), and
    // 1 / sqrt(mean + eps), a scalar per row, multiplies the finished dot product
    float ss[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) ss[b] = 0.0f;
    const int nchunks = (p.Kp + kLmKC - 1) / kLmKC;
    const int row0 = (int)blockIdx.x * p.groups * kLmWaves * kLmR;
    const WT* W = reinterpret_cast<const WT*>(p.W);
    float bv[NB];
    int bi[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { bv[b] = -INFINITY; bi[b] = 0x7fffffff; }
    for (int rg = 0; rg < p.groups; ++rg) {
        const int rbase = row0 + (rg * kLmWaves + wave) * kLmR;
        float acc[kLmR][NB];
#pragma unroll
        for (int r = 0; r < kLmR; ++r)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[r][b] = 0.0f;
        for (int c = 0; c < nchunks; ++c) {
            const int k0 = c * kLmKC, kc = (p.Kp - k0) < kLmKC ? (p.Kp - k0) : kLmKC;
            if (nchunks > 1 || rg == 0) {
                __syncthreads();   // (the statistics are written / the previous chunk has been read)
                const int kc4s = kc >> 2, ks4s = KCs >> 2;
                for (int q = tid; q < kc4s; q += kLmThreads) {
                    const float4 g4 = rms ? reinterpret_cast<const float4*>(p.rms_g + k0)[q] : make_float4(1.f, 1.f, 1.f, 1.f);
                    constexpr int SB = NB < 4 ? NB : 4;   // rows whose loads are in flight together
#pragma unroll
                    for (int b0 = 0; b0 < NB; b0 += SB) {
                        float4 x4[SB];
#pragma unroll
                        for (int bb = 0; bb < SB; ++bb) {
                            const int b = b0 + bb;
                            x4[bb] = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (b < B) {
                                const int slot = HEAD ? st->head[b] : b;
                                x4[bb] = reinterpret_cast<const float4*>(p.xin + (size_t)(p.xin_arena ? st->rows[slot].xrow : slot) * p.xin_ld + k0)[q];
                            }
                        }
#pragma unroll
                        for (int bb = 0; bb < SB; ++bb) {
                            const int b = b0 + bb;
                            float4 v = x4[bb];
                            if (rms) {
                                if (rg == 0) { float t = ss[b]; t = fmaf(v.x, v.x, t); t = fmaf(v.y, v.y, t); t = fmaf(v.z, v.z, t); t = fmaf(v.w, v.w, t); ss[b] = t; }
                                v.x = v.x * g4.x; v.y = v.y * g4.y; v.z = v.z * g4.z; v.w = v.w * g4.w;
                            }
                            reinterpret_cast<float4*>(xs)[b * ks4s + q] = v;
                        }
                    }
                }
                __syncthreads();
            }
            const float4* xv = reinterpret_cast<const float4*>(xs);
            const int kc4 = kc >> 2, ks4 = KCs >> 2;
#pragma unroll 2
            for (int q = lane; q < kc4; q += 64) {
                float4 w[kLmR];
#pragma unroll
                for (int r = 0; r < kLmR; ++r) {
                    const int row = rbase + r;
                    w[r] = row < p.N ? load_w4(W + (size_t)row * p.Kp + k0, q) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float4 v = xv[b * ks4 + q];
#pragma unroll
                    for (int r = 0; r < kLmR; ++r) {
                        float a = acc[r][b];
                        a = fmaf(w[r].x, v.x, a); a = fmaf(w[r].y, v.y, a); a = fmaf(w[r].z, v.z, a); a = fmaf(w[r].w, v.w, a);
                        acc[r][b] = a;
                    }
                }
            }
        }
        if (rms && rg == 0) {   // (all chunks have been staged once)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float t = wave_sum(ss[b]);
                if (lane == 0) red_v[wave][b] = t;
            }
            __syncthreads();
            if (tid < NB) {
                float t = red_v[0][tid];
                for (int w = 1; w < kLmWaves; ++w) t += red_v[w][tid];
                rstd_s[tid] = 1.0f / sqrtf(t / (float)p.K + p.eps);
            }
            __syncthreads();
        }
        // every lane ends up with all sums; lane r * NB + b finishes output (row rbase + r, row slot b) and also holds the other row of the pair
        float mine = 0.0f, other = 0.0f;
#pragma unroll
        for (int r = 0; r < kLmR; ++r)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float s = wave_sum(acc[r][b]);
                if (lane == r * NB + b) mine = s;
                if (lane == (1 - r) * NB + b) other = s;
                acc[r][b] = s;
            }
        const int er = lane / NB, eb = lane - er * NB, row = rbase + er;
        const bool live = lane < kLmR * NB && eb < B && row < p.N;
        if (rms && lane < kLmR * NB) { mine = mine * rstd_s[eb]; other = other * rstd_s[eb]; }
        if (HEAD) {
#pragma unroll
            for (int r = 0; r < kLmR; ++r) {
                const int rr = rbase + r;
                if (rr < p.N) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const float v = acc[r][b] * rstd_s[b];   // (the value the logits row holds)
                        if (v > bv[b]) { bv[b] = v; bi[b] = rr; }   // a wave's rows only grow: the first maximum stays
                    }
                }
            }
            if (live && p.logits) {
                const LmRow& R = st->rows[st->head[eb]];
                p.logits[((size_t)R.seq * p.max_new + R.gen) * p.N + row] = mine;
            }
            if (MODE == LM_HEAD_STEP && live) p.y[(size_t)st->head[eb] * p.y_ld + row] = mine;   // the same value, at the row's slot
        } else if (MODE == LM_GATE) {
            if (live && er == 0) {   // (N is even: the pair's second row exists)
                const float g = mine, u = other;
                p.y[(size_t)eb * p.y_ld + (row >> 1)] = g / (1.0f + expf(-g)) * u;
            }
        } else if (MODE == LM_QKV) {
            if (live) {
                const LmRow& R = st->rows[eb];
                float v = mine, w = other;
                if (p.bias) { v = v + p.bias[row]; w = w + p.bias[row ^ 1]; }   // (rows of a pair are 2 i and 2 i + 1)
                if (row < p.nq + p.nk) {
                    const int n = row < p.nq ? row : row - p.nq, head = n / p.dh, i = (n - head * p.dh) >> 1, half = p.dh >> 1;
                    const int axis = i < p.sec0 ? 0 : i < p.sec0 + p.sec1 ? 1 : 2;
                    const float ang = (float)R.rp[axis] * p.inv_freq[i];
                    const float cs = cosf(ang), sn = sinf(ang);
                    // rotate_half: out[d] = x[d] cos - x[d + half] sin, out[d + half] = x[d + half] cos + x[d] sin
                    const float out = er == 0 ? v * cs - w * sn : v * cs + w * sn;
                    const int d = i + er * half;
                    if (row < p.nq) p.q[(size_t)eb * p.q_ld + head * p.dh + d] = out;
                    else p.kc[(((size_t)R.seq * p.kvh + head) * p.maxpos + R.pos) * p.dh + d] = out;
                } else {
                    const int n = row - p.nq - p.nk, head = n / p.dh, d = n - head * p.dh;
                    p.vc[(((size_t)R.seq * p.kvh + head) * p.maxpos + R.pos) * p.dh + d] = v;
                }
            }
        } else if (live) {
            float* yr = p.y + (size_t)st->rows[eb].xrow * p.y_ld;
            yr[row] = yr[row] + mine;
        }
    }
    if (HEAD) {
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) { red_v[wave][b] = bv[b]; red_i[wave][b] = bi[b]; }
        }
        __syncthreads();
        if (tid < NB && tid < B) {
            float v = red_v[0][tid];
            int ix = red_i[0][tid];
            for (int w = 1; w < kLmWaves; ++w)
                if (better(red_v[w][tid], red_i[w][tid], v, ix)) { v = red_v[w][tid]; ix = red_i[w][tid]; }
            p.part[(size_t)tid * p.nwg + blockIdx.x] = make_float2(v, __int_as_float(ix));
        }
    }
}

}  // namespace

}  // namespace k
}  // namespace oar
