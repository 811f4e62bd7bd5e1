// mha_attention.hip -- ordinary multi-head attention with separate q / k / v sources as ONE launch: the self-attention of an RT-DETR decoder
// layer and the AIFI layer of its hybrid encoder, where q and k are projections of x + pos and v of x.  The engine's rewrite pass 3e (engine.cc) emits it for
// the spelling  heads(q) heads(k)^T, scaled on either side -> Softmax -> heads(v) -> merge:  q, k, v are three pointers, each viewed as [N][T][nh][dh] with a
// row stride of its own, so the head split and merge are address arithmetic and o [N][Tq][nh dh] is written in token order.
//
// The key loop is relpos_attention.hip's without the token grid and the rel terms -- flash-style, exact f32 on the matrix pipe
// (v_mfma_f32_16x16x4_f32 is bitwise an fmaf chain):
//   * a workgroup (4 waves) owns kMhaQueries = 64 queries of one (image, head), a wave 16 of them: lane (ql = lane & 15, g = lane >> 4) holds components
//     16 c + 4 g + j of query ql (B operand of S^T = K Q^T; MFMA j of chunk c contracts component 16 c + 4 g + j of both sides);
//   * K and V stream through LDS in blocks of kMhaKeys = 32 keys, double-buffered, every global load unconditional (a key past Tk reads the last key and its
//     score becomes -inf; a query past Tq reads the last query and is not stored), rows padded to kMhaLd = 68 floats: the K fragment is one 16-byte read per
//     4 MFMAs, the V fragment reads (key 4 g + r, component i) hit 64 different banks;
//   * the accumulator lane (ql, g) of a 16-key tile holds the scores of query ql against keys 4 g + r: each gets the scale where the graph has it, the tail
//     mask, then the running maximum (two cross-lane maxima per block) and expf;
//   * these 4 probabilities ARE the lane's B operands of O^T = V^T P^T when MFMA r contracts key 4 g + r, so P never crosses lanes; the running sum stays
//     per lane and is reduced once, in the epilogue, in a fixed order: run-to-run identical.
// The head size is rounded up to DH16 * 16 components with zeros (template: registers stay statically indexed, no scratch).
// LDS (dynamic, k::mha_attention_lds_bytes): 34,816 bytes whatever the shape -- four workgroups fit a CU's 160 KB, so one wave's soft-max overlaps
// another's MFMAs.
#include "common.h"
#include "kernels.h"
#include "kernels_dev.h"

namespace oar {
namespace k {

namespace {

template <int DH16>
__global__ __launch_bounds__(kMhaThreads) void mha_attention_kernel(MhaAttnP p, int q_tiles) {
    extern __shared__ float4 mha_lds4[];
    constexpr int F4 = 4 * DH16;                       // float4 groups per staged row
    float* Ks = reinterpret_cast<float*>(mha_lds4);    // [2][kMhaKeys][kMhaLd]
    float* Vs = Ks + 2 * kMhaKeys * kMhaLd;            // [2][kMhaKeys][kMhaLd]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    unsigned bid = blockIdx.x;
    const int qt = (int)(bid % (unsigned)q_tiles); bid /= (unsigned)q_tiles;
    const int head = (int)(bid % (unsigned)p.nh), b = (int)(bid / (unsigned)p.nh);
    const int dh = p.dh, Tq = p.Tq, Tk = p.Tk;
    const float* qimg = p.q + (size_t)b * Tq * p.ldq + head * dh;   // component 0 of this head in the image's token 0
    const float* kimg = p.k + (size_t)b * Tk * p.ldk + head * dh;
    const float* vimg = p.v + (size_t)b * Tk * p.ldv + head * dh;

    // ---- this wave's 16 queries as B-operand fragments
    const int qn = qt * kMhaQueries + wave * 16 + ql;
    const float* qrow = qimg + (size_t)min(qn, Tq - 1) * p.ldq;
    float4 qf[DH16];
#pragma clang loop unroll(full)
    for (int c = 0; c < DH16; ++c) {
        const int col = 16 * c + 4 * g;
        float4 v = *reinterpret_cast<const float4*>(qrow + min(col, dh - 4));
        if (col >= dh) v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.scale_pre) { v.x *= p.scale; v.y *= p.scale; v.z *= p.scale; v.w *= p.scale; }
        qf[c] = v;
    }
    const float post = p.scale_pre ? 1.0f : p.scale;   // (x * 1.0f is exact)

    // ---- staging: waves 0, 1 take K and waves 2, 3 take V; thread slot = tid & 127 takes float4 group (idx % F4) of key (idx / F4), idx = slot + 128 i
    float4 stg[DH16];
    const bool is_v = tid >= 128;
    const int slot = tid & 127;
    const float* src0 = is_v ? vimg : kimg;
    const size_t lds_ = is_v ? (size_t)p.ldv : (size_t)p.ldk;
    float* dst = is_v ? Vs : Ks;
    auto stage_load = [&](int kb) {
#pragma clang loop unroll(full)
        for (int i = 0; i < DH16; ++i) {
            const int idx = slot + 128 * i, kl = idx / F4, f = idx - kl * F4;
            const int row = min(kb * kMhaKeys + kl, Tk - 1);          // (always a valid address: the load is unconditional)
            float4 v = *reinterpret_cast<const float4*>(src0 + (size_t)row * lds_ + min(4 * f, dh - 4));
            if (4 * f >= dh) v = make_float4(0.f, 0.f, 0.f, 0.f);
            stg[i] = v;
        }
    };
    auto stage_commit = [&](int st) {
#pragma clang loop unroll(full)
        for (int i = 0; i < DH16; ++i) {
            const int idx = slot + 128 * i, kl = idx / F4, f = idx - kl * F4;
            *reinterpret_cast<float4*>(dst + (st * kMhaKeys + kl) * kMhaLd + 4 * f) = stg[i];
        }
    };

    f32x4 o[DH16];                                     // lane (ql, g): components 16 dt + 4 g + r of query ql
#pragma clang loop unroll(full)
    for (int dt = 0; dt < DH16; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    const int n_blocks = (Tk + kMhaKeys - 1) / kMhaKeys;
    stage_load(0);
    stage_commit(0);
    __syncthreads();
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int st = kb & 1;
        const bool more = kb + 1 < n_blocks;
        if (more) stage_load(kb + 1);
        // ---- S^T = K Q^T: two 16-key tiles, two independent accumulators
        f32x4 s[2];
        s[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; s[1] = s[0];
#pragma clang loop unroll(full)
        for (int c = 0; c < DH16; ++c) {
            float4 ka[2];
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t) ka[t] = *reinterpret_cast<const float4*>(Ks + (st * kMhaKeys + 16 * t + ql) * kMhaLd + 16 * c + 4 * g);
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].x, qf[c].x, s[t], 0, 0, 0);
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].y, qf[c].y, s[t], 0, 0, 0);
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].z, qf[c].z, s[t], 0, 0, 0);
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].w, qf[c].w, s[t], 0, 0, 0);
        }
        // ---- scale, tail mask
        float sc[8];
        const int key0 = kb * kMhaKeys + 4 * g;
#pragma clang loop unroll(full)
        for (int t = 0; t < 2; ++t)
#pragma clang loop unroll(full)
            for (int r = 0; r < 4; ++r) sc[4 * t + r] = key0 + 16 * t + r < Tk ? s[t][r] * post : -INFINITY;
        // ---- online soft-max (the first block holds key 0, so the maximum is finite from there on)
        float mx = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), fmaxf(fmaxf(sc[4], sc[5]), fmaxf(sc[6], sc[7])));
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = expf(m_run - m_new);       // first block: expf(-inf) = 0
        m_run = m_new;
        float ls = 0.f;
#pragma clang loop unroll(full)
        for (int j = 0; j < 8; ++j) { sc[j] = expf(sc[j] - m_new); ls += sc[j]; }
        l_run = l_run * alpha + ls;
#pragma clang loop unroll(full)
        for (int dt = 0; dt < DH16; ++dt)
#pragma clang loop unroll(full)
            for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        // ---- O^T += V^T P^T: MFMA (t, r) contracts key 16 t + 4 g + r
#pragma clang loop unroll(full)
        for (int t = 0; t < 2; ++t)
#pragma clang loop unroll(full)
            for (int r = 0; r < 4; ++r) {
                const float* vr = Vs + (st * kMhaKeys + 16 * t + 4 * g + r) * kMhaLd + ql;
#pragma clang loop unroll(full)
                for (int dt = 0; dt < DH16; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[16 * dt], sc[4 * t + r], o[dt], 0, 0, 0);
            }
        if (more) {
            stage_commit(st ^ 1);                      // (stage st ^ 1 was last read in iteration kb - 1, before that iteration's barrier)
            __syncthreads();
        }
    }
    // ---- epilogue: the sum over the four lane groups in a fixed order, one float4 store per (query, 16-component tile): the head merge is this address
    float l = l_run;
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (qn < Tq) {
        float* y = p.o + ((size_t)b * Tq + qn) * ((size_t)p.nh * dh) + head * dh + 4 * g;
#pragma clang loop unroll(full)
        for (int dt = 0; dt < DH16; ++dt)
            if (16 * dt + 4 * g < dh) *reinterpret_cast<float4*>(y + 16 * dt) = make_float4(o[dt][0] / l, o[dt][1] / l, o[dt][2] / l, o[dt][3] / l);
    }
}

}  // namespace

bool mha_attention_supported(int64_t N, int64_t Tq, int64_t Tk, int64_t heads, int64_t head_dim) {
    if (N < 1 || Tq < 1 || Tk < 1 || heads < 1 || head_dim < 4 || head_dim > kMhaMaxDh || head_dim % 4) return false;
    const int64_t lim = (int64_t)1 << 31;
    if (N >= lim || Tq >= lim || Tk >= lim || heads >= lim) return false;                                 // (each product below: two factors below 2^31)
    if (N * Tq >= lim || N * Tk >= lim || N * heads >= lim || heads * head_dim >= lim) return false;      // token counts, the row length
    return N * heads * ((Tq + kMhaQueries - 1) / kMhaQueries) < lim;                                      // one workgroup per (image, head, query tile)
}

void mha_attention(hipStream_t s, const MhaAttnP& p) {
    OAR_CHECK(mha_attention_supported(p.N, p.Tq, p.Tk, p.nh, p.dh), OAR_UNSUPPORTED_OP, "MultiHeadAttention: shape outside the kernel's limits");
    const int D = p.nh * p.dh;
    OAR_CHECK(p.q && p.k && p.v && p.o && (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.o) & 15) == 0 && p.ldq >= D && p.ldk >= D && p.ldv >= D &&
                  ((p.ldq | p.ldk | p.ldv) & 3) == 0,
              OAR_INTERNAL, "MultiHeadAttention: bad or misaligned arguments");
    const int q_tiles = (p.Tq + kMhaQueries - 1) / kMhaQueries;
    const int64_t grid = (int64_t)p.N * p.nh * q_tiles;
    const size_t lds = mha_attention_lds_bytes(p.dh);
    const int dh16 = (p.dh + 15) / 16;
    auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kMhaThreads), lds, s, p, q_tiles); };
    const double sets = (double)p.N * p.nh;
    ProfScope ps(s, "mha_attention", 4.0 * (2.0 * p.N * p.Tq * D + sets * q_tiles * 2.0 * p.Tk * p.dh), sets * 4.0 * p.Tq * p.Tk * p.dh);
    switch (dh16) {
        case 1: launch(mha_attention_kernel<1>); break;
        case 2: launch(mha_attention_kernel<2>); break;
        case 3: launch(mha_attention_kernel<3>); break;
        default: launch(mha_attention_kernel<4>); break;
    }
}

}  // namespace k
}  // namespace oar
