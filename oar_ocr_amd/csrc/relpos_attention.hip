// relpos_attention.hip -- the attention of one SAM / Vary ViT block (the encoder of the larger PP-FormulaNet files) as ONE launch, windowed or
// global, with the decomposed relative-position bias  q . Rh[qy, ky] + q . Rw[qx, kx]  that depends on the query.  The engine's rewrite pass 3d (engine_rewrite.cc)
// emits it for the spelling  [pad -> window partition ->] fused qkv Linear -> heads -> scores + rel terms -> Softmax -> values -> projection [-> window reverse
// -> crop]:  a Linear is per token, so the fused projection reads the unpadded tokens in image order and this kernel gathers a key set's rows by address
// (a window, or the whole grid); a padding token is a key carrying bqkv's k / v rows and is skipped as a query.
//
// The key loop is the shared flash core (flash_f32_dev.h, where the lane layout is described); a workgroup owns kFlashQueries queries of one (image,
// window, head).  What is this kernel's own:
//   * before the key loop the workgroup stages its queries in LDS once and computes rh[q][ky] = q . Rh[qy][:][ky] and rw[q][kx] from the UNSCALED q
//     ((gh + gw) dh fmas per query, ascending d), kept in LDS for the whole loop;
//   * a key past the end reads the last key and is masked with -inf; a padding key reads bqkv;
//   * each score gets the scale where the graph has it, then + rh[q][ky] + rw[q][kx]: the key's coordinates come from a table the staging threads write
//     next to the block.
// LDS (dynamic, k::relpos_attention_lds_bytes): 34,816 + 256 + 256 ((gh | 1) + (gw | 1)) bytes, 68,352 at gh = gw = 64: two workgroups per CU, so one wave's
// soft-max overlaps the other's MFMAs.
#include "common.h"
#include "kernels.h"
#include "flash_f32_dev.h"

namespace oar {
namespace k {

namespace {

template <int DH16>
__global__ __launch_bounds__(kFlashThreads) void relpos_attention_kernel(RelPosAttnP p, int q_tiles) {
    extern __shared__ float4 rp_lds4[];
    constexpr int F4 = 4 * DH16;                       // float4 groups per staged row
    const int gw = p.ws ? p.ws : p.W, gh = p.ws ? p.ws : p.H, N = gh * gw;
    const int ghs = gh | 1, gws = gw | 1;
    float* Ks = reinterpret_cast<float*>(rp_lds4);     // [2][kFlashKeys][kFlashLd]; before the key loop: the workgroup's queries [kFlashQueries][kFlashLd]
    float* Vs = Ks + 2 * kFlashKeys * kFlashLd;        // [2][kFlashKeys][kFlashLd]
    int* tab = reinterpret_cast<int*>(Vs + 2 * kFlashKeys * kFlashLd);   // [2][kFlashKeys]: ky << 8 | kx, negative past the key set's end
    float* rhs = reinterpret_cast<float*>(tab + 2 * kFlashKeys);        // [kFlashQueries][ghs]
    float* rws = rhs + kFlashQueries * ghs;            // [kFlashQueries][gws]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 15, g = lane >> 4;
    const int wbn = p.ws ? (p.W + p.ws - 1) / p.ws : 1, hbn = p.ws ? (p.H + p.ws - 1) / p.ws : 1, nW = hbn * wbn;
    unsigned bid = blockIdx.x;
    const int qt = (int)(bid % (unsigned)q_tiles); bid /= (unsigned)q_tiles;
    const int head = (int)(bid % (unsigned)p.nh); bid /= (unsigned)p.nh;
    const int wi = (int)(bid % (unsigned)nW), b = (int)(bid / (unsigned)nW);
    const int oy = (wi / wbn) * gh, ox = (wi % wbn) * gw;          // the key set's origin in the (padded) grid; global: (0, 0)
    const int C = p.nh * p.dh, dh = p.dh;
    const size_t ld = (size_t)3 * C;
    const float* img = p.qkv + (size_t)b * p.H * p.W * ld + head * dh;   // q of the image's token (0, 0); k at + C, v at + 2 C
    auto token = [&](int n) {                          // the row of the key set's n-th token within the image, -1: padding
        const int r = n / gw, c = n - r * gw, y = oy + r, x = ox + c;
        return y < p.H && x < p.W ? y * p.W + x : -1;
    };
    const int q0 = qt * kFlashQueries;

    // ---- the workgroup's queries -> LDS (unscaled), then rh / rw
    for (int i = 0; i < DH16; ++i) {
        const int idx = tid + kFlashThreads * i, qi = idx / F4, f = idx - qi * F4;
        const int row = max(token(min(q0 + qi, N - 1)), 0);        // (a padding query and a query past the end compute values nobody stores)
        float4 v = *reinterpret_cast<const float4*>(img + (size_t)row * ld + min(4 * f, dh - 4));
        if (4 * f >= dh) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(Ks + qi * kFlashLd + 4 * f) = v;
    }
    __syncthreads();
    for (int idx = tid; idx < kFlashQueries * gh; idx += kFlashThreads) {
        const int qi = idx / gh, ky = idx - qi * gh, qy = min(q0 + qi, N - 1) / gw;
        const float* r = p.rh + (size_t)qy * dh * gh + ky;
        float a = 0.f;
        for (int d = 0; d < dh; ++d) a = fmaf(Ks[qi * kFlashLd + d], r[(size_t)d * gh], a);
        rhs[qi * ghs + ky] = a;
    }
    for (int idx = tid; idx < kFlashQueries * gw; idx += kFlashThreads) {
        const int qi = idx / gw, kx = idx - qi * gw, n = min(q0 + qi, N - 1), qx = n - (n / gw) * gw;
        const float* r = p.rw + (size_t)qx * dh * gw + kx;
        float a = 0.f;
        for (int d = 0; d < dh; ++d) a = fmaf(Ks[qi * kFlashLd + d], r[(size_t)d * gw], a);
        rws[qi * gws + kx] = a;
    }

    // ---- this wave's 16 queries as B-operand fragments
    const int qn = q0 + wave * 16 + ql;
    const int qrow = token(min(qn, N - 1));
    float4 qf[DH16];
    flash_load_q<DH16>(qf, img + (size_t)max(qrow, 0) * ld, g, dh, p.scale_pre, p.scale);
    const float post = p.scale_pre ? 1.0f : p.scale;   // (x * 1.0f is exact)

    // ---- staging: waves 0, 1 take K and waves 2, 3 take V; threads 0 .. kFlashKeys - 1 also take the block's key coordinates
    float4 stg[DH16];
    int tst = 0;
    const bool is_v = tid >= 128;
    const int slot = tid & 127, part = is_v ? 2 * C : C;
    const float* bpad = p.bqkv ? p.bqkv + part + head * dh : nullptr;   // what a padding token is behind the Linear
    float* dst = is_v ? Vs : Ks;
    auto stage_load = [&](int kb) {
        flash_stage_load<DH16>(stg, slot, kb, N, dh, [&](int n, bool& zero) {
            const int row = token(n);
            zero = row < 0 && !bpad;
            return row >= 0 ? img + (size_t)row * ld + part : bpad ? bpad : img + part;
        });
        if (tid < kFlashKeys) {
            const int n = kb * kFlashKeys + tid, r = n / gw;
            tst = n < N ? (r << 8) | (n - r * gw) : (int)0x80000000;
        }
    };
    auto stage_commit = [&](int st) {
        flash_stage_commit<DH16>(stg, dst, slot, st);
        if (tid < kFlashKeys) tab[st * kFlashKeys + tid] = tst;
    };

    FlashAcc<DH16> acc;
    acc.init();
    const float* rhq = rhs + (wave * 16 + ql) * ghs;
    const float* rwq = rws + (wave * 16 + ql) * gws;

    const int n_blocks = (N + kFlashKeys - 1) / kFlashKeys;
    stage_load(0);
    __syncthreads();                                   // rh / rw are written and the staged queries read: the K buffer may be overwritten
    stage_commit(0);
    __syncthreads();
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int st = kb & 1;
        const bool more = kb + 1 < n_blocks;
        if (more) stage_load(kb + 1);
        flash_block<DH16>(Ks, Vs, st, ql, g, qf, acc, [&](const f32x4 (&s)[2], float (&sc)[8]) {   // scale, rel terms, tail mask
#pragma clang loop unroll(full)
            for (int t = 0; t < 2; ++t) {
                const int4 tv = *reinterpret_cast<const int4*>(tab + st * kFlashKeys + 16 * t + 4 * g);
                const int tk[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma clang loop unroll(full)
                for (int r = 0; r < 4; ++r) {
                    const int ky = (tk[r] >> 8) & 0xff, kx = tk[r] & 0xff;
                    float x = s[t][r] * post;
                    x = x + rhq[ky];
                    x = x + rwq[kx];
                    sc[4 * t + r] = tk[r] < 0 ? -INFINITY : x;
                }
            }
        });
        if (more) {
            stage_commit(st ^ 1);                      // (stage st ^ 1 was last read in iteration kb - 1, before that iteration's barrier)
            __syncthreads();
        }
    }
    // ---- one float4 store per (query, 16-component tile)
    const float l = flash_sum(acc);
    if (qn < N && qrow >= 0) flash_store(acc, l, p.o + ((size_t)b * p.H * p.W + qrow) * C + head * dh + 4 * g, g, dh);
}

}  // namespace

bool relpos_attention_supported(int64_t B, int64_t H, int64_t W, int64_t ws, int64_t heads, int64_t head_dim) {
    if (B < 1 || H < 1 || W < 1 || ws < 0 || heads < 1 || head_dim < 4 || head_dim > kRpMaxDh || head_dim % 4) return false;
    if (ws ? ws > kRpMaxGrid : (H > kRpMaxGrid || W > kRpMaxGrid)) return false;
    const int64_t lim = (int64_t)1 << 31;
    if (B >= lim || H >= lim || W >= lim || heads >= lim || H * W >= lim || B * H * W >= lim) return false;   // (each product of two factors below 2^31)
    const int64_t N = ws ? ws * ws : H * W, nW = ws ? ((H + ws - 1) / ws) * ((W + ws - 1) / ws) : 1, q_tiles = (N + kFlashQueries - 1) / kFlashQueries;
    if (B * nW >= lim || B * nW * heads >= lim) return false;
    return B * nW * heads * q_tiles < lim;               // one workgroup per (image, key set, head, query tile)
}

void relpos_attention(hipStream_t s, const RelPosAttnP& p) {
    OAR_CHECK(relpos_attention_supported(p.B, p.H, p.W, p.ws, p.nh, p.dh), OAR_UNSUPPORTED_OP, "RelPosAttention: shape outside the kernel's limits");
    OAR_CHECK(p.qkv && p.rh && p.rw && p.o && ((uintptr_t)p.qkv & 15) == 0 && ((uintptr_t)p.o & 15) == 0 && ((uintptr_t)p.bqkv & 15) == 0, OAR_INTERNAL,
              "RelPosAttention: bad or misaligned arguments");
    const int gh = p.ws ? p.ws : p.H, gw = p.ws ? p.ws : p.W, N = gh * gw, q_tiles = (N + kFlashQueries - 1) / kFlashQueries;
    const int nW = p.ws ? ((p.H + p.ws - 1) / p.ws) * ((p.W + p.ws - 1) / p.ws) : 1;
    const int64_t grid = (int64_t)p.B * nW * p.nh * q_tiles;
    const size_t lds = relpos_attention_lds_bytes(gh, gw);   // (the kernel carves its five arrays in the order of that sum)
    const double tokens = (double)p.B * p.H * p.W, sets = (double)p.B * nW * p.nh, C = (double)p.nh * p.dh;
    ProfScope ps(s, "relpos_attention", 4.0 * (4.0 * tokens * C + sets * q_tiles * 2.0 * N * p.dh), sets * N * (4.0 * N * p.dh + 2.0 * (gh + gw) * p.dh));
    flash_dispatch(p.dh, [&](auto n) {
        auto kern = relpos_attention_kernel<decltype(n)::value>;
        if (lds > 64 * 1024) OAR_MAX_LDS_ONCE(kern, (int)relpos_attention_lds_bytes(kRpMaxGrid, kRpMaxGrid));
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kFlashThreads), lds, s, p, q_tiles);
    });
}

}  // namespace k
}  // namespace oar
