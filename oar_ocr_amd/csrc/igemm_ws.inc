// igemm_ws.inc -- weight-stationary implicit-GEMM kernel; included by igemm_ws_1x1.hip and igemm_ws_gen.hip, which
// instantiate it for IGEMM_WS_IS1X1 = true / false (two translation units: the instantiations compile in parallel).
#include "igemm_dev.h"

namespace oar {
namespace k {

// ------------------------------------------------------------------------------------------ igemm ws (weight-stationary)
// Same math and the same weight fragments as conv_igemm_kernel, different data movement.  Findings it is built on
// (single-shape micro-benchmarks, tools/igemm_bench.py, M=245760 K=N=192):
//  * every wave of conv_igemm_kernel re-fetches the same weight fragments through L1 -- 2/3 of its vector-memory traffic;
//  * a wave that stores its tile and then loads (bias, next pixels) waits for its own stores to be ACKNOWLEDGED
//    (~4-5 us under load), because s_waitcnt vmcnt is in-order: per tile that cost as much as half the K loop;
//  * the SIMD arbiter favours its oldest wave: with a fixed split waves 0-3 of a workgroup finished at 123 us and
//    waves 12-15 at 178 us.
// So: a persistent workgroup (16 waves, one workgroup per CU) keeps its cout tile of W (NT*16 couts x K) and the bias
// resident in LDS in fragment order; its waves pull wave tiles (PF*16 pixels x the cout tile) from an LDS counter;
// every pixel fragment is loaded from memory exactly once per cout tile (HBM/L2 -> VGPR, 3 register stages, loads
// issued from inline asm with hand-counted s_waitcnt because hipcc drains the queue with vmcnt(0) if left to place
// the waits); weight fragments come from LDS (one conflict-free ds_read_b128 per PF*4 MFMAs, 3-slot ring); the
// first two K chunks of the NEXT tile are requested before the stores of the current one, and the accumulators
// start from the bias, so nothing ever waits behind a store.
struct IgemmWsP {
    IgemmP g;
    int ny;             // cout tiles
    int groups;         // teams per XCD; team t handles cout tiles t, t+groups, ...
    long wt_per_xcd;    // wave tiles (PF*16 pixels) per XCD band
    long wt_total;      // ceil(M / (PF*16))
};

template <int NT, int PF, bool IS1X1>
__global__ __launch_bounds__(1024) void conv_igemm_ws_kernel(IgemmWsP q) {
    extern __shared__ float4 ws_lds[];   // [kc][nf][lane] weights | [nf][16] bias | counter
    const IgemmP& p = q.g;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pl_ = lane & 15, g = lane >> 4;
    const int xcd = (int)(blockIdx.x & 7);             // workgroup b runs on XCD b % 8 (only locality depends on it)
    const int j = (int)(blockIdx.x >> 3);              // workgroup index inside the XCD
    const int per_xcd = (int)(gridDim.x >> 3);
    const int team = j % q.groups, member = j / q.groups, team_size = (per_xcd - team + q.groups - 1) / q.groups;
    float* lds_bias = reinterpret_cast<float*>(ws_lds + (long)NT * p.KC * 64);
    unsigned* ws_ctr = reinterpret_cast<unsigned*>(lds_bias + NT * 16);
    // this workgroup's wave tiles inside the XCD band: one contiguous range for 1x1 layers; dealt cyclically for kh x kw
    // layers, so that the tiles in flight on the XCD form one compact run of image rows and the tap re-reads of the rows
    // above / below hit its L2 (see igemm_ws3.hip)
    long wt_begin, wt_count, wt_stride;
    {
        const long x0 = (long)xcd * q.wt_per_xcd, x1 = min(q.wt_total, x0 + q.wt_per_xcd);
        const long n_x = max(0L, x1 - x0), share = (n_x + team_size - 1) / team_size;
        if (IS1X1) {
            wt_stride = 1;
            wt_begin = x0 + (long)member * share;
            wt_count = max(0L, min(share, x1 - wt_begin));
        } else {
            wt_stride = team_size;
            wt_begin = x0 + member;
            wt_count = n_x > member ? (n_x - member + team_size - 1) / team_size : 0;
        }
    }
    constexpr int NL = PF;                 // vector-memory loads per chunk (pixels only)

    auto issue = [](f32x4& dst, const float* src) { asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(src)); };
    struct Stage { f32x4 x[PF]; bool ok[PF]; };
    struct Tile { long m0; long pix_base[PF]; int ih0[PF], iw0[PF]; };
    auto tile_of = [&](long wt, Tile& t) {
        t.m0 = wt * (PF * 16);
#pragma clang loop unroll(full)
        for (int pf = 0; pf < PF; ++pf) {
            long m = min(t.m0 + pf * 16 + pl_, p.M - 1);   // clamped rows compute garbage that is never stored
            if (IS1X1) {
                t.pix_base[pf] = m * (long)p.Cin; t.ih0[pf] = 0; t.iw0[pf] = 0;
            } else {
                long hw = (long)p.Ho * p.Wo;
                long n = m / hw; long r = m - n * hw;
                int oh = (int)(r / p.Wo), ow = (int)(r - (long)oh * p.Wo);
                t.pix_base[pf] = n * (long)p.H * p.W * p.Cin;
                t.ih0[pf] = oh * p.sh - p.pt; t.iw0[pf] = ow * p.sw - p.pl;
            }
        }
    };
    auto x_addr = [&](const Tile& t, int kc, int pf, bool& ok_out) -> const float* {
        const int k = min(kc * 16 + 4 * g, p.K - 4);   // zero-padded K tail of W: re-read a valid quad
        if (IS1X1) { ok_out = true; return p.x + t.pix_base[pf] + k; }
        const int tap = (int)__umulhi((unsigned)k, p.cin_magic), ci = k - tap * p.Cin;   // (Cin >= 4 on these kernels: the magic number exists)
        const int tap_h = igemm_tap_h(p, tap), tap_w = tap - tap_h * p.kw;
        const int ih = t.ih0[pf] + tap_h * p.dh, iw = t.iw0[pf] + tap_w * p.dw;
        ok_out = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
        const int ihc = min(max(ih, 0), p.H - 1), iwc = min(max(iw, 0), p.W - 1);
        return p.x + t.pix_base[pf] + ((long)ihc * p.W + iwc) * p.Cin + ci;
    };
    auto grab = [&]() -> long {
        unsigned u = 0;
        if (lane == 0) u = atomicAdd(ws_ctr, 1u);
        return (long)(unsigned)__builtin_amdgcn_readfirstlane((int)u);
    };

    (void)wave;

    for (int ntile = team; ntile < q.ny; ntile += q.groups) {
        const int nf0 = ntile * NT;
        // ---- (re)fill the LDS weight tile: global fragment order [nf][kc][lane] -> LDS [kc][nf][lane]; bias; counter
        __syncthreads();
        if (threadIdx.x == 0) *ws_ctr = 0;
        if (threadIdx.x < NT * 16) {
            const int c = nf0 * 16 + (int)threadIdx.x;
            const int cc = c < p.gemm_cout ? c : 0;
            lds_bias[threadIdx.x] = p.bias ? p.bias[p.convt ? cc % p.Cout : cc] : 0.f;
        }
        {
            const float4* wsrc = reinterpret_cast<const float4*>(p.w) + (long)nf0 * p.KC * 64;
            const int total = NT * p.KC * 64;
            // batches of 8 independent loads per thread (a load -> ds_write loop pays one L2 round trip per iteration)
            const int stride = (int)blockDim.x;
            int i0 = threadIdx.x;
            for (; i0 + 7 * stride < total; i0 += 8 * stride) {
                float4 v[8];
#pragma clang loop unroll(full)
                for (int u = 0; u < 8; ++u) v[u] = wsrc[i0 + u * stride];
#pragma clang loop unroll(full)
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + u * stride, l = i & 63, f = i >> 6;   // f = nf * KC + kc
                    const int nf = f / p.KC, kc = f - nf * p.KC;
                    ws_lds[(kc * NT + nf) * 64 + l] = v[u];
                }
            }
            for (; i0 < total; i0 += stride) {
                const int l = i0 & 63, f = i0 >> 6;
                const int nf = f / p.KC, kc = f - nf * p.KC;
                ws_lds[(kc * NT + nf) * 64 + l] = wsrc[i0];
            }
        }
        __syncthreads();

        long u = grab();
        if (u >= wt_count) continue;
        Tile cur, nxt;
        tile_of(wt_begin + u * wt_stride, cur);
        Stage s0, s1, s2;   // named (not an array): every access below resolves at compile time, nothing goes to scratch
        auto stage = [&](auto Ic) -> Stage& {
            constexpr int I = decltype(Ic)::value % 3;
            if constexpr (I == 0) return s0; else if constexpr (I == 1) return s1; else return s2;
        };
#pragma clang loop unroll(full)
        for (int pf = 0; pf < PF; ++pf) issue(s0.x[pf], x_addr(cur, 0, pf, s0.ok[pf]));
#pragma clang loop unroll(full)
        for (int pf = 0; pf < PF; ++pf) issue(s1.x[pf], x_addr(cur, 1, pf, s1.ok[pf]));
        // first tile of this wave: land both chunks now (run_tile's chunks 0 and 1 never wait)
#pragma clang loop unroll(full)
        for (int pf = 0; pf < PF; ++pf) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(s0.x[pf])); asm volatile("" : "+v"(s1.x[pf])); }

        const float4* wl = ws_lds + lane;
        // one tile.  Chunk i lives in stage i%3 (chunks 0 and 1 were requested by the previous tile, see the boundary
        // code below); the weight ring restarts every tile.
        auto run_tile = [&]() {
            f32x4 acc[NT][PF];
#pragma clang loop unroll(full)
            for (int nf = 0; nf < NT; ++nf) {
                const float4 bq = *reinterpret_cast<const float4*>(lds_bias + nf * 16 + g * 4);
#pragma clang loop unroll(full)
                for (int pf = 0; pf < PF; ++pf) acc[nf][pf] = (f32x4){bq.x, bq.y, bq.z, bq.w};
            }
            float4 wr[3];
            wr[0] = wl[0];
            wr[1] = NT > 1 ? wl[64] : wl[(long)NT * 64];
            // chunk kc: SI = kc % 3 = its stage.  WAIT = false for chunks 0 and 1, whose pixels were landed before the
            // previous tile's stores were issued (see run_tile's tail): vmcnt cannot be used while stores are in flight
            // behind the loads of interest -- stores may be acknowledged BEFORE older loads return, so an allowance that
            // counts them proves nothing (observed as sparse wrong outputs).  From chunk 2 on the allowance is loads only.
            auto chunk = [&](int kc, auto SIc, auto WAITc) {
                constexpr int SI = decltype(SIc)::value;
                constexpr bool WAIT = decltype(WAITc)::value;
                Stage& cs = stage(std::integral_constant<int, SI>{});
                Stage& ns = stage(std::integral_constant<int, SI + 2>{});
                constexpr int r0 = SI == 0 ? 0 : SI == 1 ? NT % 3 : (2 * NT) % 3;
                if (WAIT) {
#pragma clang loop unroll(full)
                    for (int pf = 0; pf < PF; ++pf) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(cs.x[pf]) : "n"(NL));
                }
                {   // request chunk kc+2 of the stream: this tile's, or the next tile's chunk kc+2-KC
                    const int k2 = kc + 2;
                    const bool in_cur = k2 < p.KC;
                    const int kk = in_cur ? k2 : k2 - p.KC;
#pragma clang loop unroll(full)
                    for (int pf = 0; pf < PF; ++pf) {
                        Tile t;
                        t.m0 = 0;
                        t.pix_base[pf] = in_cur ? cur.pix_base[pf] : nxt.pix_base[pf];
                        t.ih0[pf] = in_cur ? cur.ih0[pf] : nxt.ih0[pf];
                        t.iw0[pf] = in_cur ? cur.iw0[pf] : nxt.iw0[pf];
                        issue(ns.x[pf], x_addr(t, kk, pf, ns.ok[pf]));
                    }
                }
                if (!IS1X1) {
#pragma clang loop unroll(full)
                    for (int pf = 0; pf < PF; ++pf)
#pragma clang loop unroll(full)
                        for (int e = 0; e < 4; ++e) cs.x[pf][e] = cs.ok[pf] ? cs.x[pf][e] : 0.f;
                }
                const int k1 = min(kc + 1, p.KC - 1), k2c = min(kc + 2, p.KC - 1);
#pragma clang loop unroll(full)
                for (int nf = 0; nf < NT; ++nf) {
                    {   // fragment two ahead in the flattened (kc, nf) order goes into the slot freed by the previous one
                        const int dk = (nf + 2) / NT, nf2 = (nf + 2) % NT;   // compile-time after unrolling
                        const int kq = dk == 0 ? kc : dk == 1 ? k1 : k2c;
                        __builtin_amdgcn_sched_barrier(0);   // pinned: left alone the scheduler hoists every ds_read of the trip
                        wr[(r0 + nf + 2) % 3] = wl[((long)kq * NT + nf2) * 64];
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const float4 w = wr[(r0 + nf) % 3];
                    const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma clang loop unroll(full)
                    for (int jj = 0; jj < 4; ++jj)
#pragma clang loop unroll(full)
                        for (int pf = 0; pf < PF; ++pf)
                            acc[nf][pf] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[jj], cs.x[pf][jj], acc[nf][pf], 0, 0, 0);
                }
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            using Wy = std::true_type;
            using Wn = std::false_type;
            chunk(0, I0{}, Wn{});
            chunk(1, I1{}, Wn{});
            int kc = 2;
            for (; kc + 2 < p.KC; kc += 3) { chunk(kc, I2{}, Wy{}); chunk(kc + 1, I0{}, Wy{}); chunk(kc + 2, I1{}, Wy{}); }
            if (kc < p.KC) chunk(kc, I2{}, Wy{});
            if (kc + 1 < p.KC) chunk(kc + 1, I0{}, Wy{});
            // land the two chunks requested for the next tile BEFORE any store is issued (they are 1-2 chunks old)
#pragma clang loop unroll(full)
            for (int pf = 0; pf < PF; ++pf) asm volatile("s_waitcnt vmcnt(0)" : "+v"(s0.x[pf]), "+v"(s1.x[pf]), "+v"(s2.x[pf]));
            if constexpr (PF == 1) {
                if (p.ctc_part) { igemm_ctc_epilogue<NT>(p, acc, cur.m0, pl_, g, nf0, ntile, q.ny); return; }
            }
            igemm_epilogue<NT, PF, true>(p, acc, cur.m0, pl_, g, nf0, false);   // float4 path only (checked by the host)
        };

        for (;;) {
            const long un = grab();
            const bool has_next = un < wt_count;
            tile_of(wt_begin + (has_next ? un : u) * wt_stride, nxt);   // no next tile: the tail requests re-read this one (never consumed)
            run_tile();
            if (!has_next) break;
            // ---- tile boundary: chunk 0 and 1 of the next tile sit (landed) in stages KC%3 and (KC+1)%3; rotate them
            // into stages 0 and 1
            const int rot = p.KC % 3;
            if (rot == 1) { s0 = s1; s1 = s2; }
            else if (rot == 2) { s1 = s0; s0 = s2; }
            cur = nxt; u = un;
        }
        // drain the never-consumed tail requests before their registers are reused
#pragma clang loop unroll(full)
        for (int pf = 0; pf < PF; ++pf) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(s0.x[pf]));
            asm volatile("" : "+v"(s1.x[pf]));
            asm volatile("" : "+v"(s2.x[pf]));
        }
    }
}

template <int NT, int PF, bool IS1X1>
static void launch_igemm_ws(hipStream_t s, const IgemmP& p, int ny, size_t lds) {
    OAR_MAX_LDS_ONCE((conv_igemm_ws_kernel<NT, PF, IS1X1>), 160 * 1024);
    IgemmWsP q;
    q.g = p; q.ny = ny;
    const int waves = 16, per_xcd = 32;
    q.wt_total = (p.M + PF * 16 - 1) / (PF * 16);
    q.wt_per_xcd = (q.wt_total + 7) / 8;
    q.groups = ny < per_xcd ? ny : per_xcd;
    hipLaunchKernelGGL((conv_igemm_ws_kernel<NT, PF, IS1X1>), dim3(per_xcd * 8), dim3(waves * 64), lds, s, q);
}


void IGEMM_WS_ENTRY(hipStream_t s, const IgemmP& p, int ws_nt, int ny, size_t lds) {
    switch (ws_nt) {
        case 8: launch_igemm_ws<8, igemm_ws_pf(8), IGEMM_WS_IS1X1>(s, p, ny, lds); break;
        case 6: launch_igemm_ws<6, igemm_ws_pf(6), IGEMM_WS_IS1X1>(s, p, ny, lds); break;
        case 4: launch_igemm_ws<4, igemm_ws_pf(4), IGEMM_WS_IS1X1>(s, p, ny, lds); break;
        case 3: launch_igemm_ws<3, igemm_ws_pf(3), IGEMM_WS_IS1X1>(s, p, ny, lds); break;
        case 2: launch_igemm_ws<2, igemm_ws_pf(2), IGEMM_WS_IS1X1>(s, p, ny, lds); break;
        default: launch_igemm_ws<1, igemm_ws_pf(1), IGEMM_WS_IS1X1>(s, p, ny, lds); break;
    }
}

}  // namespace k
}  // namespace oar
