// mha_attention.hip -- ordinary multi-head attention with separate q / k / v sources as ONE launch: the self-attention of an RT-DETR decoder
// layer and the AIFI layer of its hybrid encoder, where q and k are projections of x + pos and v of x.  The engine's rewrite pass 3e (engine_rewrite.cc) emits it for
// the spelling  heads(q) heads(k)^T, scaled on either side -> Softmax -> heads(v) -> merge:  q, k, v are three pointers, each viewed as [N][T][nh][dh] with a
// row stride of its own, so the head split and merge are address arithmetic and o [N][Tq][nh dh] is written in token order.
//
// The key loop is the shared flash core (flash_f32_dev.h, where the lane layout is described): a workgroup owns kFlashQueries queries of one (image,
// head); a key past Tk reads the last key and its score becomes -inf, a query past Tq reads the last query and is not stored.
// LDS (dynamic, k::mha_attention_lds_bytes): 34,816 bytes whatever the shape -- four workgroups fit a CU's 160 KB, so one wave's soft-max overlaps
// another's MFMAs.
#include "common.h"
#include "kernels.h"
#include "flash_f32_dev.h"

namespace oar {
namespace k {

namespace {

template <int DH16>
__global__ __launch_bounds__(kFlashThreads) void mha_attention_kernel(MhaAttnP p, int q_tiles) {
    extern __shared__ float4 mha_lds4[];
    float* Ks = reinterpret_cast<float*>(mha_lds4);    // [2][kFlashKeys][kFlashLd]
    float* Vs = Ks + 2 * kFlashKeys * kFlashLd;        // [2][kFlashKeys][kFlashLd]
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
    const int qn = qt * kFlashQueries + wave * 16 + ql;
    float4 qf[DH16];
    flash_load_q<DH16>(qf, qimg + (size_t)min(qn, Tq - 1) * p.ldq, g, dh, p.scale_pre, p.scale);
    const float post = p.scale_pre ? 1.0f : p.scale;   // (x * 1.0f is exact)

    // ---- staging: waves 0, 1 take K and waves 2, 3 take V
    float4 stg[DH16];
    const bool is_v = tid >= 128;
    const int slot = tid & 127;
    const float* src0 = is_v ? vimg : kimg;
    const size_t lds_ = is_v ? (size_t)p.ldv : (size_t)p.ldk;
    float* dst = is_v ? Vs : Ks;
    auto stage_load = [&](int kb) { flash_stage_load<DH16>(stg, slot, kb, Tk, dh, [&](int row, bool&) { return src0 + (size_t)row * lds_; }); };

    FlashAcc<DH16> acc;
    acc.init();
    const int n_blocks = (Tk + kFlashKeys - 1) / kFlashKeys;
    stage_load(0);
    flash_stage_commit<DH16>(stg, dst, slot, 0);
    __syncthreads();
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int st = kb & 1;
        const bool more = kb + 1 < n_blocks;
        if (more) stage_load(kb + 1);
        flash_block<DH16>(Ks, Vs, st, ql, g, qf, acc, [&](const f32x4 (&s)[2], float (&sc)[8]) {   // scale, tail mask
            const int key0 = kb * kFlashKeys + 4 * g;
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t)
#pragma clang loop unroll(full)
                for (int r = 0; r < 4; ++r) sc[4 * t + r] = key0 + 16 * t + r < Tk ? s[t][r] * post : -INFINITY;
        });
        if (more) {
            flash_stage_commit<DH16>(stg, dst, slot, st ^ 1);
            __syncthreads();
        }
    }
    // ---- one float4 store per (query, 16-component tile): the head merge is this address
    const float l = flash_sum(acc);
    if (qn < Tq) flash_store(acc, l, p.o + ((size_t)b * Tq + qn) * ((size_t)p.nh * dh) + head * dh + 4 * g, g, dh);
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
    const double sets = (double)p.N * p.nh;
    ProfScope ps(s, "mha_attention", 4.0 * (2.0 * p.N * p.Tq * D + sets * q_tiles * 2.0 * p.Tk * p.dh), sets * 4.0 * p.Tq * p.Tk * p.dh);
    flash_dispatch(p.dh, [&](auto n) { hipLaunchKernelGGL(mha_attention_kernel<decltype(n)::value>, dim3((unsigned)grid), dim3(kFlashThreads), lds, s, p, q_tiles); });
}

}  // namespace k
}  // namespace oar
