// flash_f32_dev.h -- the flash-attention core of relpos_attention.hip and mha_attention.hip: exact f32 on the matrix pipe
// (v_mfma_f32_16x16x4_f32 is bitwise an fmaf chain), one layout (k::kFlash* in kernels.h).  __device__ __forceinline__ templates on DH16 = ceil(head_dim /
// 16), and the host's switch over the four instantiations: the head size is rounded up to DH16 * 16 components with zeros, so registers stay statically indexed (no scratch).  A kernel supplies three things:
// where a query or key row comes from, what is added to a raw score and how the tail is masked, and where the output row goes.
//   * a workgroup (4 waves) owns kFlashQueries = 64 queries, a wave 16 of them: lane (ql = lane & 15, g = lane >> 4) holds components 16 c + 4 g + j of
//     query ql (B operand of S^T = K Q^T; MFMA j of chunk c contracts component 16 c + 4 g + j of both sides);
//   * K and V stream through LDS in blocks of kFlashKeys = 32 keys, double-buffered, every global load unconditional (a key past the end reads the last
//     key and the kernel's score functor makes it -inf; a query past the end reads the last query and is not stored), rows padded to kFlashLd = 68 floats:
//     the K fragment is one 16-byte read per 4 MFMAs, the V fragment reads (key 4 g + r, component i) hit 64 different banks;
//   * the accumulator lane (ql, g) of a 16-key tile holds the scores of query ql against keys 4 g + r: the score functor finishes them (scale, bias terms,
//     mask), then the running maximum (two cross-lane maxima per block) and expf;
//   * these 4 probabilities ARE the lane's B operands of O^T = V^T P^T when MFMA r contracts key 4 g + r, so P never crosses lanes; the running sum stays
//     per lane and is reduced once, in the epilogue, in a fixed order: run-to-run identical.
// The key loop of a kernel is
//     flash_stage_load(0); flash_stage_commit(0); barrier;
//     for kb: if (more) flash_stage_load(kb + 1);  flash_block(kb & 1, score);  if (more) { flash_stage_commit((kb & 1) ^ 1); barrier; }
// (stage st ^ 1 was last read in iteration kb - 1, before that iteration's barrier).
#pragma once
#include <type_traits>

#include "kernels_dev.h"

namespace oar {
namespace k {

// a lane's DH16 float4 groups of the query row `qrow` (components 16 c + 4 g ..), zero beyond dh, times `scale` where the graph scales q
template <int DH16>
__device__ __forceinline__ void flash_load_q(float4 (&qf)[DH16], const float* qrow, int g, int dh, int scale_pre, float scale) {
#pragma clang loop unroll(full)
    for (int c = 0; c < DH16; ++c) {
        const int col = 16 * c + 4 * g;
        float4 v = *reinterpret_cast<const float4*>(qrow + min(col, dh - 4));
        if (col >= dh) v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (scale_pre) { v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale; }
        qf[c] = v;
    }
}

// the running state of a lane: o holds components 16 dt + 4 g + r of query ql
template <int DH16>
struct FlashAcc {
    f32x4 o[DH16];
    float m_run, l_run;
    __device__ __forceinline__ void init() {
#pragma clang loop unroll(full)
        for (int dt = 0; dt < DH16; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        m_run = -INFINITY; l_run = 0.f;
    }
};

// staging: waves 0, 1 take K and waves 2, 3 take V; thread slot = tid & 127 takes float4 group (idx % F4) of key (idx / F4), idx = slot + 128 i.
// row(n, zero) gives the source row of key n < n_keys (always a valid address: the load is unconditional) and whether it is staged as zeros.
template <int DH16, class Row>
__device__ __forceinline__ void flash_stage_load(float4 (&stg)[DH16], int slot, int kb, int n_keys, int dh, Row&& row) {
    constexpr int F4 = 4 * DH16;                       // float4 groups per staged row
#pragma clang loop unroll(full)
    for (int i = 0; i < DH16; ++i) {
        const int idx = slot + 128 * i, kl = idx / F4, f = idx - kl * F4;
        bool zero = false;
        const float* src = row(min(kb * kFlashKeys + kl, n_keys - 1), zero);
        float4 v = *reinterpret_cast<const float4*>(src + min(4 * f, dh - 4));
        if (4 * f >= dh || zero) v = make_float4(0.f, 0.f, 0.f, 0.f);
        stg[i] = v;
    }
}
// LD: the row stride of Ks / Vs in floats, kFlashLd unless a kernel with a larger head says otherwise (vis_attention.hip: 84 at DH16 = 5)
template <int DH16, int LD = kFlashLd>
__device__ __forceinline__ void flash_stage_commit(const float4 (&stg)[DH16], float* dst, int slot, int st) {   // dst: Ks or Vs, as the thread's half has it
    constexpr int F4 = 4 * DH16;
#pragma clang loop unroll(full)
    for (int i = 0; i < DH16; ++i) {
        const int idx = slot + 128 * i, kl = idx / F4, f = idx - kl * F4;
        *reinterpret_cast<float4*>(dst + (st * kFlashKeys + kl) * LD + 4 * f) = stg[i];
    }
}

// one block of kFlashKeys keys from stage st of Ks / Vs ([2][kFlashKeys][LD] each).  score(s, sc): the two raw accumulators (tile t, s[t][r]: key
// 16 t + 4 g + r of the block) -> the eight finished scores sc[4 t + r], -inf for a key that does not exist.
template <int DH16, int LD = kFlashLd, class Score>
__device__ __forceinline__ void flash_block(const float* Ks, const float* Vs, int st, int ql, int g, const float4 (&qf)[DH16], FlashAcc<DH16>& a, Score&& score) {
    // ---- S^T = K Q^T: two 16-key tiles, two independent accumulators
    f32x4 s[2];
    s[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; s[1] = s[0];
#pragma clang loop unroll(full)
    for (int c = 0; c < DH16; ++c) {
        float4 ka[2];
#pragma clang loop unroll(full)
        for (int t = 0; t < 2; ++t) ka[t] = *reinterpret_cast<const float4*>(Ks + (st * kFlashKeys + 16 * t + ql) * LD + 16 * c + 4 * g);
#pragma clang loop unroll(full)
        for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].x, qf[c].x, s[t], 0, 0, 0);
#pragma clang loop unroll(full)
        for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].y, qf[c].y, s[t], 0, 0, 0);
#pragma clang loop unroll(full)
        for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].z, qf[c].z, s[t], 0, 0, 0);
#pragma clang loop unroll(full)
        for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].w, qf[c].w, s[t], 0, 0, 0);
    }
    float sc[8];
    score(s, sc);
    // ---- online soft-max (the first block holds key 0, so the maximum is finite from there on)
    float mx = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), fmaxf(fmaxf(sc[4], sc[5]), fmaxf(sc[6], sc[7])));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(a.m_run, mx);
    const float alpha = expf(a.m_run - m_new);         // first block: expf(-inf) = 0
    a.m_run = m_new;
    float ls = 0.f;
#pragma clang loop unroll(full)
    for (int j = 0; j < 8; ++j) { sc[j] = expf(sc[j] - m_new); ls += sc[j]; }
    a.l_run = a.l_run * alpha + ls;
#pragma clang loop unroll(full)
    for (int dt = 0; dt < DH16; ++dt)
#pragma clang loop unroll(full)
        for (int r = 0; r < 4; ++r) a.o[dt][r] *= alpha;
    // ---- O^T += V^T P^T: MFMA (t, r) contracts key 16 t + 4 g + r
#pragma clang loop unroll(full)
    for (int t = 0; t < 2; ++t)
#pragma clang loop unroll(full)
        for (int r = 0; r < 4; ++r) {
            const float* vr = Vs + (st * kFlashKeys + 16 * t + 4 * g + r) * LD + ql;
#pragma clang loop unroll(full)
            for (int dt = 0; dt < DH16; ++dt) a.o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[16 * dt], sc[4 * t + r], a.o[dt], 0, 0, 0);
        }
}

// epilogue: the sum over the four lane groups in a fixed order (every lane calls this), then one float4 store per (query, 16-component tile).
// y: component 4 g of the query's output row; the kernel forms it inside its own guard.
template <int DH16>
__device__ __forceinline__ float flash_sum(const FlashAcc<DH16>& a) {
    float l = a.l_run;
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    return l;
}
template <int DH16>
__device__ __forceinline__ void flash_store(const FlashAcc<DH16>& a, float l, float* y, int g, int dh) {
#pragma clang loop unroll(full)
    for (int dt = 0; dt < DH16; ++dt)
        if (16 * dt + 4 * g < dh) *reinterpret_cast<float4*>(y + 16 * dt) = make_float4(a.o[dt][0] / l, a.o[dt][1] / l, a.o[dt][2] / l, a.o[dt][3] / l);
}

// host: f(std::integral_constant<int, DH16>) for head_dim, so that a launcher names its kernel template once
template <class F>
inline void flash_dispatch(int head_dim, F&& f) {
    switch ((head_dim + 15) / 16) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

}  // namespace k
}  // namespace oar
