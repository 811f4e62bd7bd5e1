// lm_prefill_attn.hip -- the causal grouped-query attention of the language model's GEMM-based prefill as ONE launch per layer.
//
// The key loop is the shared flash core (flash_f32_dev.h, where the lane layout is described).  What this kernel supplies:
//   * a workgroup is one entry (sequence, query head, tile of 64 query positions) of a host-built tile table; tiles are aligned to the SEQUENCE's own positions
//     (tile i = positions 64 i .. 64 i + 63), and an entry names the positions [lo, hi) of its tile that this launch holds: a chunk of the prefill may cut a tile;
//   * the keys are positions 0 .. p of the query's own sequence in the key / value cache, already rotated (the layer's q / k / v launch has stored the chunk's
//     keys): no mask tensor exists, the score functor applies `key <= p`.  A key past hi - 1 reads key hi - 1 and is masked for every query of the entry;
//   * key 0 is visible to every query, so the running maximum is finite after block 0, and a block that is wholly masked for a query is an exact no-op
//     (alpha = expf(0) = 1, every probability expf(-inf) = 0): a query's output does not depend on how many blocks its workgroup walks, so not on where a
//     chunk cuts its tile.  A wave whose 16 queries all precede a block skips it (the same no-op, left out);
//   * head sizes 8 .. 128: instantiations DH16 = 1 .. 8, LDS rows of 16 DH16 + 4 floats (an odd number of float4 groups: the 16 K-fragment reads of a lane
//     group fall on 16 different 16-byte slots), 67,584 bytes at head size 128: two workgroups per CU.
#include "common.h"
#include "kernels.h"
#include "flash_f32_dev.h"
#include "lm_prefill.h"

namespace oar {
namespace k {

namespace {

template <int DH16>
__global__ __launch_bounds__(kFlashThreads) void lm_prefill_attn_kernel(LmPfAttnP p) {
    constexpr int LD = 16 * DH16 + 4;
    extern __shared__ float4 lmpf_lds4[];
    float* Ks = reinterpret_cast<float*>(lmpf_lds4);   // [2][kFlashKeys][LD]
    float* Vs = Ks + 2 * kFlashKeys * LD;              // [2][kFlashKeys][LD]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    const LmPfTile tile = p.tiles[blockIdx.x];
    const int dh = p.dh, G = p.H / p.KVH, kvh = tile.head / G;
    const int n_keys = tile.hi;                        // keys 0 .. hi - 1 are in the cache
    const size_t base = ((size_t)tile.seq * p.KVH + kvh) * p.maxpos * dh;

    // ---- this wave's 16 queries as B-operand fragments; a position outside [lo, hi) reads the nearest one inside and is not stored
    const int qn = tile.qt * kFlashQueries + wave * 16 + ql;
    const int qc = min(max(qn, tile.lo), tile.hi - 1);
    float4 qf[DH16];
    flash_load_q<DH16>(qf, p.q + (size_t)(tile.row_lo + (qc - tile.lo)) * p.q_ld + tile.head * dh, g, dh, 0, 1.0f);
    const float scale = p.scale;

    // ---- staging: waves 0, 1 take K and waves 2, 3 take V
    float4 stg[DH16];
    const bool is_v = tid >= 128;
    const int slot = tid & 127;
    const float* src0 = (is_v ? p.vc : p.kc) + base;
    float* dst = is_v ? Vs : Ks;
    auto stage_load = [&](int kb) { flash_stage_load<DH16>(stg, slot, kb, n_keys, dh, [&](int row, bool&) { return src0 + (size_t)row * dh; }); };

    FlashAcc<DH16> acc;
    acc.init();
    const int n_blocks = (n_keys + kFlashKeys - 1) / kFlashKeys;
    const int wave_last = tile.qt * kFlashQueries + wave * 16 + 15;   // the last position of this wave's queries
    stage_load(0);
    flash_stage_commit<DH16, LD>(stg, dst, slot, 0);
    __syncthreads();
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int st = kb & 1;
        const bool more = kb + 1 < n_blocks;
        if (more) stage_load(kb + 1);
        if (kb * kFlashKeys <= wave_last)              // (uniform over the wave)
            flash_block<DH16, LD>(Ks, Vs, st, ql, g, qf, acc, [&](const f32x4 (&s)[2], float (&sc)[8]) {   // scale after the product, causal bound
                const int key0 = kb * kFlashKeys + 4 * g;
#pragma clang loop unroll(full)
                for (int t = 0; t < 2; ++t)
#pragma clang loop unroll(full)
                    for (int r = 0; r < 4; ++r) sc[4 * t + r] = key0 + 16 * t + r <= qc ? s[t][r] * scale : -INFINITY;
            });
        if (more) {
            flash_stage_commit<DH16, LD>(stg, dst, slot, st ^ 1);
            __syncthreads();
        }
    }
    const float l = flash_sum(acc);
    if (qn >= tile.lo && qn < tile.hi) flash_store(acc, l, p.o + (size_t)(tile.row_lo + (qn - tile.lo)) * p.o_ld + tile.head * dh + 4 * g, g, dh);
}

template <int DH16>
void launch_attn(hipStream_t s, const LmPfAttnP& p, size_t lds) {
    OAR_MAX_LDS_ONCE((lm_prefill_attn_kernel<DH16>), 80 * 1024);
    hipLaunchKernelGGL((lm_prefill_attn_kernel<DH16>), dim3((unsigned)p.n_tiles), dim3(kFlashThreads), lds, s, p);
}

}  // namespace

void lm_prefill_attention(hipStream_t s, const LmPfAttnP& p, double bytes, double flops) {
    OAR_CHECK(lm_pf_head_dim_supported(p.dh) && p.H >= 1 && p.KVH >= 1 && p.H % p.KVH == 0 && p.maxpos >= 1, OAR_UNSUPPORTED_OP, "lm_prefill_attention: head size outside 8..128 in steps of 4");
    const int Hd = p.H * p.dh;
    OAR_CHECK(p.q && p.kc && p.vc && p.o && p.tiles && p.n_tiles > 0 && (((uintptr_t)p.q | (uintptr_t)p.kc | (uintptr_t)p.vc | (uintptr_t)p.o) & 15) == 0 && p.q_ld >= Hd &&
                  p.o_ld >= Hd && ((p.q_ld | p.o_ld) & 3) == 0,
              OAR_INTERNAL, "lm_prefill_attention: bad or misaligned arguments");
    static_assert(kFlashQueries == kLmPfQueries && kFlashKeys == kLmPfKeys && kFlashThreads == kLmPfThreads, "lm_prefill.h repeats the flash core's layout");
    const size_t lds = lm_pf_attn_lds_bytes(p.dh);
    ProfScope ps(s, "lm_gemm_attn", bytes, flops);
    switch (lm_pf_dh16(p.dh)) {
        case 1: launch_attn<1>(s, p, lds); break;
        case 2: launch_attn<2>(s, p, lds); break;
        case 3: launch_attn<3>(s, p, lds); break;
        case 4: launch_attn<4>(s, p, lds); break;
        case 5: launch_attn<5>(s, p, lds); break;
        case 6: launch_attn<6>(s, p, lds); break;
        case 7: launch_attn<7>(s, p, lds); break;
        default: launch_attn<8>(s, p, lds); break;
    }
}

}  // namespace k
}  // namespace oar
