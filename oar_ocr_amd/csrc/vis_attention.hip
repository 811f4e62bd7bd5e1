// vis_attention.hip -- the attention of one layer of the PaddleOCR-VL vision encoder as ONE launch: the patches of several images packed back
// to back, every image a segment [start, start + len) of the rows, 2-D rotary embedding on q and k, full (non-causal) soft-max inside a segment.
//
// The key loop is the shared flash core (flash_f32_dev.h, where the lane layout is described).  What this kernel supplies:
//   * a workgroup is one entry (segment, head, query tile) of a host-built tile table, so the grid is flat over segments of different lengths;
//   * a key past the segment's end reads the segment's last row and its score becomes -inf, a query past the end reads the last row and is not stored: no
//     row outside [start, start + len) is ever read, of qkv or of the cos / sin tables;
//   * the rotation x'[c] = x[c] cos[c] - x[c + dh/2] sin[c], x'[c + dh/2] = x[c + dh/2] cos[c] + x[c] sin[c] happens in registers, on q when its fragments are
//     loaded and on k between a key block's global loads and its LDS commit: the partner of float4 group f is group f +- dh/8 of the same row (dh % 8 == 0), no
//     rotated copy of q or k exists in memory, v is staged as it is;
//   * head sizes up to 80: a fifth instantiation DH16 = 5, whose LDS rows are kVisLd5 = 84 floats (80 + 4: like 68, an odd number of float4 groups, so the 16
//     K-fragment reads of a lane group fall on 16 different 16-byte slots and the V reads of keys 4 g + r on different banks).
// LDS (dynamic, k::vis_attention_lds_bytes): 34,816 bytes up to head size 64, 43,008 above -- three workgroups fit a CU's 160 KB.
#include "common.h"
#include "kernels.h"
#include "flash_f32_dev.h"

namespace oar {
namespace k {

namespace {

// one float4 group of a row, rotated: col (a multiple of 4, < dh) names the group, h2 = dh / 2; cs / sn: the row's tables [h2]
struct VisRot {
    float4 x, y, cs, sn;   // the group, its partner group, cos and sin of the pair's angle
    bool low;              // the group lies in the first half
    __device__ __forceinline__ void load(const float* row, const float* cs_row, const float* sn_row, int col, int h2) {
        low = col < h2;
        const int tc = low ? col : col - h2;
        x = *reinterpret_cast<const float4*>(row + col);
        y = *reinterpret_cast<const float4*>(row + (low ? col + h2 : tc));
        cs = *reinterpret_cast<const float4*>(cs_row + tc);
        sn = *reinterpret_cast<const float4*>(sn_row + tc);
    }
    __device__ __forceinline__ float4 value() const {
        const float4 a = make_float4(x.x * cs.x, x.y * cs.y, x.z * cs.z, x.w * cs.w), b = make_float4(y.x * sn.x, y.y * sn.y, y.z * sn.z, y.w * sn.w);
        return low ? make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w) : make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
};

template <int DH16, int LD>
__global__ __launch_bounds__(kFlashThreads) void vis_attention_kernel(VisAttnP p) {
    extern __shared__ float4 vis_lds4[];
    float* Ks = reinterpret_cast<float*>(vis_lds4);    // [2][kFlashKeys][LD]
    float* Vs = Ks + 2 * kFlashKeys * LD;              // [2][kFlashKeys][LD]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    const VisTile tile = p.tiles[blockIdx.x];
    const VisSeg seg = p.segs[tile.seg];
    const int dh = p.dh, h2 = dh >> 1, T = seg.len, head = tile.head;
    const int D = p.nh * dh;
    const float* qseg = p.qkv + (size_t)seg.start * p.ld + head * dh;   // component 0 of this head's q in the segment's row 0; k at + D, v at + 2 D
    const float* cseg = p.cos + (size_t)seg.start * h2;
    const float* sseg = p.sin + (size_t)seg.start * h2;

    // ---- this wave's 16 queries as B-operand fragments, rotated
    const int qn = tile.qt * kFlashQueries + wave * 16 + ql;
    float4 qf[DH16];
    {
        const int qr = min(qn, T - 1);
        const float* qrow = qseg + (size_t)qr * p.ld;
#pragma clang loop unroll(full)
        for (int c = 0; c < DH16; ++c) {
            const int col = 16 * c + 4 * g;
            VisRot r;
            r.load(qrow, cseg + (size_t)qr * h2, sseg + (size_t)qr * h2, min(col, dh - 4), h2);
            float4 v = r.value();
            if (col >= dh) v = make_float4(0.f, 0.f, 0.f, 0.f);
            qf[c] = v;
        }
    }

    // ---- staging: waves 0, 1 take K (rotated at the commit) and waves 2, 3 take V
    constexpr int F4 = 4 * DH16;
    const bool is_v = tid >= 128;
    const int slot = tid & 127;
    const float* src0 = qseg + (is_v ? 2 * D : D);
    float* dst = is_v ? Vs : Ks;
    VisRot rk[DH16];       // a V thread uses x alone
    float4 stg[DH16];
    auto stage_load = [&](int kb) {
#pragma clang loop unroll(full)
        for (int i = 0; i < DH16; ++i) {
            const int idx = slot + 128 * i, kl = idx / F4, f = idx - kl * F4;
            const int row = min(kb * kFlashKeys + kl, T - 1), col = min(4 * f, dh - 4);
            const float* src = src0 + (size_t)row * p.ld;
            if (is_v) rk[i].x = *reinterpret_cast<const float4*>(src + col);
            else rk[i].load(src, cseg + (size_t)row * h2, sseg + (size_t)row * h2, col, h2);
        }
    };
    auto stage_commit = [&](int st) {
#pragma clang loop unroll(full)
        for (int i = 0; i < DH16; ++i) {
            const int idx = slot + 128 * i, kl = idx / F4, f = idx - kl * F4;
            float4 v = is_v ? rk[i].x : rk[i].value();
            if (4 * f >= dh) v = make_float4(0.f, 0.f, 0.f, 0.f);
            stg[i] = v;
        }
        flash_stage_commit<DH16, LD>(stg, dst, slot, st);
    };

    FlashAcc<DH16> acc;
    acc.init();
    const int n_blocks = (T + kFlashKeys - 1) / kFlashKeys;
    const float scale = p.scale;
    stage_load(0);
    stage_commit(0);
    __syncthreads();
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int st = kb & 1;
        const bool more = kb + 1 < n_blocks;
        if (more) stage_load(kb + 1);
        flash_block<DH16, LD>(Ks, Vs, st, ql, g, qf, acc, [&](const f32x4 (&s)[2], float (&sc)[8]) {   // scale after the product, tail mask
            const int key0 = kb * kFlashKeys + 4 * g;
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t)
#pragma clang loop unroll(full)
                for (int r = 0; r < 4; ++r) sc[4 * t + r] = key0 + 16 * t + r < T ? s[t][r] * scale : -INFINITY;
        });
        if (more) {
            stage_commit(st ^ 1);
            __syncthreads();
        }
    }
    // ---- one float4 store per (query, 16-component tile), in token order
    const float l = flash_sum(acc);
    if (qn < T) flash_store(acc, l, p.o + (size_t)(seg.start + qn) * D + head * dh + 4 * g, g, dh);
}

}  // namespace

void vis_attention(hipStream_t s, const VisAttnP& p, double bytes, double flops) {
    OAR_CHECK(vis_attention_supported(p.nh, p.dh), OAR_UNSUPPORTED_OP, "vis_attention: head size outside 8..80 in steps of 8");
    const int D = p.nh * p.dh;
    OAR_CHECK(p.qkv && p.cos && p.sin && p.o && p.segs && p.tiles && p.n_tiles > 0 &&
                  (((uintptr_t)p.qkv | (uintptr_t)p.cos | (uintptr_t)p.sin | (uintptr_t)p.o) & 15) == 0 && p.ld >= 3 * D && (p.ld & 3) == 0,
              OAR_INTERNAL, "vis_attention: bad or misaligned arguments");
    const size_t lds = vis_attention_lds_bytes(p.dh);
    ProfScope ps(s, "vis_attention", bytes, flops);   // (k::vis_attention_cost: the segment lengths are the caller's)
    const dim3 grid((unsigned)p.n_tiles), block(kFlashThreads);
    switch ((p.dh + 15) / 16) {                    // flash_dispatch stops at 4: this kernel's own list
        case 1: hipLaunchKernelGGL((vis_attention_kernel<1, kFlashLd>), grid, block, lds, s, p); break;
        case 2: hipLaunchKernelGGL((vis_attention_kernel<2, kFlashLd>), grid, block, lds, s, p); break;
        case 3: hipLaunchKernelGGL((vis_attention_kernel<3, kFlashLd>), grid, block, lds, s, p); break;
        case 4: hipLaunchKernelGGL((vis_attention_kernel<4, kFlashLd>), grid, block, lds, s, p); break;
        default: hipLaunchKernelGGL((vis_attention_kernel<5, kVisLd5>), grid, block, lds, s, p); break;
    }
}

}  // namespace k
}  // namespace oar
