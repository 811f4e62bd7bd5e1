// lm_prefill_gemm.hip -- lm_gemm: the token-major GEMM of the language model's GEMM-based prefill.  Y[M][N] = X[M][K] W[N][Kp]^T on
// v_mfma_f32_16x16x4_f32 (exact f32: bitwise an fmaf chain), W being the very tables lm_host.cc uploads for the rows kernels: row-major, f32 or bf16 (widened
// with u << 16 on the way into LDS: the same arithmetic on the same values), rotary pairs and gate / up pairs as ADJACENT rows.
//
// The tile is computed as W X^T: the MFMA's M dimension runs over weight rows, so accumulator lane (tok = lane & 15, g = lane >> 4) holds weight rows
// 4 g .. 4 g + 3 of token tok -- both rows of two pairs.  Rotation and gating are register arithmetic with the expressions of lm_decode.hip.
//   * a workgroup (4 waves) owns 64 weight rows x 64 tokens, wave w the 32 x 32 corner (w & 1, w >> 1) as 2 x 2 MFMA tiles;
//   * both operands are K-contiguous and stream through LDS in chunks of 32 columns, two stages, every global load unconditional (a row past the end reads the
//     last row and is not stored; a column past K is staged as zero); rows padded to 36 floats;
//   * lane (i, g) reads the float4 at columns 16 c + 4 g of its row: MFMA j of group c contracts column 16 c + 4 g + j on both sides.  An output element's sum
//     runs over the chunks in order and, inside a chunk, over (c, j, g) in the matrix unit's order: fixed by K alone.  No split-K, no atomics;
//   * RMSNorm in front: x g is staged, the 8 threads that stage a token's row gather its sum of squares on the way (thread f always the columns 32 c + 4 f ..),
//     a butterfly over the 8 finishes it, and 1 / sqrt(mean + eps) multiplies the finished dot product: no launch of its own.
#include "common.h"
#include "kernels_dev.h"
#include "lm_prefill.h"

namespace oar {
namespace k {

namespace {

__device__ __forceinline__ float4 gemm_load4(const float* row, int col) { return *reinterpret_cast<const float4*>(row + col); }
__device__ __forceinline__ float4 gemm_load4(const uint16_t* row, int col) {   // four bf16 -> f32, exact
    const uint2 u = *reinterpret_cast<const uint2*>(row + col);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}

template <int MODE, typename WT>
__global__ __launch_bounds__(kLmGemmThreads) void lm_gemm_kernel(LmGemmP p) {
    constexpr int LD = kLmGemmLd, TN = kLmGemmTN, TM = kLmGemmTM, KC = kLmGemmKC;
    __shared__ float4 Ws4[2 * TN * LD / 4];
    __shared__ float4 Xs4[2 * TM * LD / 4];
    __shared__ float rstd_s[TM];
    float* Ws = reinterpret_cast<float*>(Ws4);
    float* Xs = reinterpret_cast<float*>(Xs4);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int n0 = (int)blockIdx.x * TN, m0 = (int)blockIdx.y * TM;
    const int wr = (wave & 1) * 32, wt = (wave >> 1) * 32;
    const bool rms = p.rms_g != nullptr;

    // ---- staging: thread (r = tid >> 3, f = tid & 7) takes the float4 group f of rows r and r + 32, of W and of X
    const int sr = tid >> 3, sf = tid & 7;
    const WT* wrow[2];
    const float* xrow[2];
#pragma clang loop unroll(full)
    for (int i = 0; i < 2; ++i) {
        const int n = min(n0 + sr + 32 * i, p.N - 1), m = min(m0 + sr + 32 * i, p.M - 1);
        wrow[i] = reinterpret_cast<const WT*>(p.w) + (size_t)n * p.Kp;
        xrow[i] = p.x + (size_t)(p.x_gather ? p.rows[m].xrow : m) * p.x_ld;
    }
    float4 wreg[2], xreg[2];
    float ss[2] = {0.f, 0.f};
    auto stage_load = [&](int c) {
        const int col = c * KC + 4 * sf;
        const bool in = col < p.K;
        const int cc = min(col, p.K - 4);
        const float4 g4 = rms ? *reinterpret_cast<const float4*>(p.rms_g + cc) : make_float4(1.f, 1.f, 1.f, 1.f);
#pragma clang loop unroll(full)
        for (int i = 0; i < 2; ++i) {
            float4 w = gemm_load4(wrow[i], cc), x = gemm_load4(xrow[i], cc);
            if (!in) { w = make_float4(0.f, 0.f, 0.f, 0.f); x = w; }
            if (rms) {
                float t = ss[i];
                t = fmaf(x.x, x.x, t); t = fmaf(x.y, x.y, t); t = fmaf(x.z, x.z, t); t = fmaf(x.w, x.w, t);
                ss[i] = t;
                x.x = x.x * g4.x; x.y = x.y * g4.y; x.z = x.z * g4.z; x.w = x.w * g4.w;
            }
            wreg[i] = w; xreg[i] = x;
        }
    };
    auto stage_commit = [&](int st) {
#pragma clang loop unroll(full)
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<float4*>(Ws + (st * TN + sr + 32 * i) * LD + 4 * sf) = wreg[i];
            *reinterpret_cast<float4*>(Xs + (st * TM + sr + 32 * i) * LD + 4 * sf) = xreg[i];
        }
    };

    f32x4 acc[2][2];
#pragma clang loop unroll(full)
    for (int i = 0; i < 2; ++i)
#pragma clang loop unroll(full)
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nchunks = (p.K + KC - 1) / KC;
    stage_load(0);
    stage_commit(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int st = c & 1;
        const bool more = c + 1 < nchunks;
        if (more) stage_load(c + 1);
#pragma clang loop unroll(full)
        for (int cg = 0; cg < KC / 16; ++cg) {
            float4 a[2], b[2];
#pragma clang loop unroll(full)
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const float4*>(Ws + (st * TN + wr + 16 * i + l15) * LD + 16 * cg + 4 * g);
                b[i] = *reinterpret_cast<const float4*>(Xs + (st * TM + wt + 16 * i + l15) * LD + 16 * cg + 4 * g);
            }
#pragma clang loop unroll(full)
            for (int i = 0; i < 2; ++i)
#pragma clang loop unroll(full)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
#pragma clang loop unroll(full)
            for (int i = 0; i < 2; ++i)
#pragma clang loop unroll(full)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
#pragma clang loop unroll(full)
            for (int i = 0; i < 2; ++i)
#pragma clang loop unroll(full)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
#pragma clang loop unroll(full)
            for (int i = 0; i < 2; ++i)
#pragma clang loop unroll(full)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
        }
        if (more) {
            stage_commit(st ^ 1);
            __syncthreads();
        }
    }
    if (rms) {   // (uniform over the grid)
#pragma clang loop unroll(full)
        for (int i = 0; i < 2; ++i) {
            float t = ss[i];
            t += __shfl_xor(t, 1, 64); t += __shfl_xor(t, 2, 64); t += __shfl_xor(t, 4, 64);
            if (sf == 0) rstd_s[sr + 32 * i] = 1.0f / sqrtf(t / (float)p.K + p.eps);
        }
        __syncthreads();
    }

    // ---- epilogue: lane (tok, g) holds rows nb + r, r = 0 .. 3, of its token in acc[i][j]
#pragma clang loop unroll(full)
    for (int j = 0; j < 2; ++j) {
        const int tl = wt + 16 * j + l15, m = m0 + tl;
        if (m >= p.M) continue;
        const float rs = rms ? rstd_s[tl] : 1.0f;
#pragma clang loop unroll(full)
        for (int i = 0; i < 2; ++i) {
            const int nb = n0 + wr + 16 * i + 4 * g;
            if (nb >= p.N) continue;
            float v[4];
#pragma clang loop unroll(full)
            for (int r = 0; r < 4; ++r) v[r] = rms ? acc[i][j][r] * rs : acc[i][j][r];
            if (MODE == LM_GEMM_PLAIN || MODE == LM_GEMM_RESID) {
                float* yr = p.y + (size_t)(p.y_scatter ? p.rows[m].xrow : m) * p.y_ld;
#pragma clang loop unroll(full)
                for (int r = 0; r < 4; ++r)
                    if (nb + r < p.N) yr[nb + r] = MODE == LM_GEMM_RESID ? yr[nb + r] + v[r] : v[r];
            } else if (MODE == LM_GEMM_GATE) {   // (N is even: rows nb + 1 and nb + 3 exist with nb and nb + 2)
#pragma clang loop unroll(full)
                for (int h = 0; h < 2; ++h)
                    if (nb + 2 * h < p.N) {
                        const float gt = v[2 * h], u = v[2 * h + 1];
                        p.y[(size_t)m * p.y_ld + ((nb + 2 * h) >> 1)] = gt / (1.0f + expf(-gt)) * u;
                    }
            } else {
                const LmPfRow& R = p.rows[m];
                const int rp0 = R.rp[0], rp1 = R.rp[1], rp2 = R.rp[2], seq = R.seq, pos = R.pos;   // (scalars: a run-time index into a copy would be scratch)
#pragma clang loop unroll(full)
                for (int h = 0; h < 2; ++h) {
                    const int row = nb + 2 * h;   // the pair (row, row + 1)
                    if (row >= p.N) continue;
                    float a = v[2 * h], b = v[2 * h + 1];
                    if (p.bias) { a = a + p.bias[row]; b = b + p.bias[row + 1]; }
                    if (row < p.nq + p.nk) {
                        const int n = row < p.nq ? row : row - p.nq, head = n / p.dh, fi = (n - head * p.dh) >> 1, half = p.dh >> 1;
                        const int rp = fi < p.sec0 ? rp0 : fi < p.sec0 + p.sec1 ? rp1 : rp2;
                        const float ang = (float)rp * p.inv_freq[fi];
                        const float cs = cosf(ang), sn = sinf(ang);
                        // rotate_half: out[d] = x[d] cos - x[d + half] sin, out[d + half] = x[d + half] cos + x[d] sin
                        const float lo = a * cs - b * sn, hi = b * cs + a * sn;
                        float* dst = row < p.nq ? p.q + (size_t)m * p.q_ld + head * p.dh
                                                : p.kc + (((size_t)seq * p.kvh + head) * p.maxpos + pos) * p.dh;
                        dst[fi] = lo; dst[fi + half] = hi;
                    } else {
                        const int n = row - p.nq - p.nk, head = n / p.dh, d = n - head * p.dh;   // (dh is even: both rows lie in one head)
                        float* dst = p.vc + (((size_t)seq * p.kvh + head) * p.maxpos + pos) * p.dh;
                        dst[d] = a; dst[d + 1] = b;
                    }
                }
            }
        }
    }
}

template <int MODE>
void launch_gemm(hipStream_t s, const LmGemmP& p, dim3 grid) {
    if (p.bf16) hipLaunchKernelGGL((lm_gemm_kernel<MODE, uint16_t>), grid, dim3(kLmGemmThreads), 0, s, p);
    else hipLaunchKernelGGL((lm_gemm_kernel<MODE, float>), grid, dim3(kLmGemmThreads), 0, s, p);
}

}  // namespace

void lm_gemm(hipStream_t s, const LmGemmP& p) {
    OAR_CHECK(p.M >= 1 && p.N >= 1 && p.K >= 4 && p.K % 4 == 0 && p.Kp >= p.K && p.Kp % 4 == 0 && p.x && p.w && p.x_ld >= p.K && p.x_ld % 4 == 0 &&
                  (((uintptr_t)p.x | (uintptr_t)p.w) & 15) == 0,
              OAR_INTERNAL, "lm_gemm: bad or misaligned arguments");
    OAR_CHECK(p.mode >= LM_GEMM_PLAIN && p.mode <= LM_GEMM_GATE && (p.mode == LM_GEMM_PLAIN || p.mode == LM_GEMM_RESID || p.N % 2 == 0) &&
                  (!(p.x_gather || p.y_scatter || p.mode == LM_GEMM_QKV) || p.rows) && (p.mode == LM_GEMM_QKV ? (p.q && p.kc && p.vc && p.inv_freq && p.dh % 2 == 0) : p.y != nullptr),
              OAR_INTERNAL, "lm_gemm: an epilogue without its arguments");
    const int64_t gx = (p.N + kLmGemmTN - 1) / kLmGemmTN, gy = (p.M + kLmGemmTM - 1) / kLmGemmTM;
    OAR_CHECK(gy <= 65535, OAR_INTERNAL, "lm_gemm: more than 65535 token tiles");
    const double wb = (p.bf16 ? 2.0 : 4.0) * (double)p.N * p.Kp;
    ProfScope ps(s, "lm_gemm_linear", wb + 4.0 * (double)p.M * ((double)p.K + p.N), 2.0 * (double)p.M * p.N * p.K);
    const dim3 grid((unsigned)gx, (unsigned)gy);
    switch (p.mode) {
        case LM_GEMM_PLAIN: launch_gemm<LM_GEMM_PLAIN>(s, p, grid); break;
        case LM_GEMM_RESID: launch_gemm<LM_GEMM_RESID>(s, p, grid); break;
        case LM_GEMM_QKV: launch_gemm<LM_GEMM_QKV>(s, p, grid); break;
        default: launch_gemm<LM_GEMM_GATE>(s, p, grid); break;
    }
}

}  // namespace k
}  // namespace oar
