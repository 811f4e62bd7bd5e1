// lm_decode_split.hip -- split-key attention of the language-model chain (lm_decode.hip): the same sums as lm_attn_kernel, cut over the keys.
//
//   lm_attn_split   one workgroup per (row, kv head, chunk of <= 8 query heads of the group, span s): keys [s S, min((s + 1) S, p + 1)) of the row's own sequence.
//                   Per 64 keys: all 256 threads stage the K and V rows in LDS (the rows are contiguous in the cache: coalesced 16-byte loads, every load of a
//                   tile issued before the first is stored), lane j of a wave scores key j against the wave's heads (q read from LDS as a broadcast), one butterfly
//                   for the tile's maximum and one for its sum, then the lanes turn to d and add the tile's weighted values.  Wave w owns the heads w HPW .. of the
//                   chunk: its running (maximum, sum) are wave-uniform, its value sums live in lanes d and d + 64.  One partial (m, l, acc[dh]) per head and span.
//   lm_attn_merge   one workgroup per (row, head): partials 0 .. ceil((p + 1) / S) - 1 in span order, rescaled to their common maximum; writes o.
//
// All f32, no float atomics, nothing waits on another workgroup.  A row's output depends on (p, dh, S) and the data: the spans and tiles are cut at multiples of
// S and 64 of the row's own positions, a tile's sums run in key order, and neither the row's slot, the number of rows, the grid (sized from the step's largest
// position: a workgroup whose span starts at or beyond p + 1 returns) nor what the workspace held enters.  Keys at and beyond p + 1 are never loaded.
#include "common.h"
#include "lm_decode.h"

namespace oar {
namespace k {

namespace {

struct LmSplitP {
    const LmStep* st;
    const float* q; int q_ld;
    const float *kc, *vc;
    int H, KVH, dh, maxpos, S, nsmax, gchunks;
    float scale;
    float* ws;
    float* o; int o_ld;
    const int* alive;
};

__device__ __forceinline__ float split_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float split_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <int GT>
__global__ __launch_bounds__(kLmSplitThreads) void lm_attn_split_kernel(LmSplitP p) {
    extern __shared__ float4 lm_split_lds4[];
    if (*p.alive == 0) return;
    constexpr int HPW = (GT + kLmSplitWaves - 1) / kLmSplitWaves;   // heads of the chunk a wave owns
    constexpr int TK = kLmSplitTile;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int span = (int)blockIdx.x, b = (int)blockIdx.y, kvh = (int)blockIdx.z / p.gchunks, g0 = ((int)blockIdx.z - kvh * p.gchunks) * GT;
    const LmRow& R = p.st->rows[b];
    const int n = R.pos + 1, k_lo = span * p.S;
    if (k_lo >= n) return;   // (uniform over the workgroup: before any barrier)
    const int k_hi = k_lo + p.S < n ? k_lo + p.S : n;
    const int dh = p.dh, dh4 = dh >> 2, G = p.H / p.KVH, ldk = lm_split_ldk(dh);
    float* qs = reinterpret_cast<float*>(lm_split_lds4);   // [GT][dh]
    float* ks = qs + GT * dh;                               // [64][ldk]
    float* vs = ks + TK * ldk;                              // [64][dh]
    float* ps = vs + TK * dh;                               // [GT][64]
    for (int i = tid; i < GT * dh4; i += kLmSplitThreads) {
        const int g = i / dh4, c = i - g * dh4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g0 + g < G) v = *reinterpret_cast<const float4*>(p.q + (size_t)b * p.q_ld + (size_t)(kvh * G + g0 + g) * dh + c * 4);
        reinterpret_cast<float4*>(qs)[i] = v;
    }
    const size_t base = ((size_t)R.seq * p.KVH + kvh) * p.maxpos * dh;
    const bool d0 = lane < dh, d1 = lane + 64 < dh;
    float m[HPW], l[HPW], acc[HPW][2];
#pragma unroll
    for (int h = 0; h < HPW; ++h) { m[h] = -INFINITY; l[h] = 0.0f; acc[h][0] = 0.0f; acc[h][1] = 0.0f; }
    for (int t0 = k_lo; t0 < k_hi; t0 += TK) {
        const int nk = k_hi - t0 < TK ? k_hi - t0 : TK, n4 = nk * dh4;
        const float4* kg = reinterpret_cast<const float4*>(p.kc + base + (size_t)t0 * dh);
        const float4* vg = reinterpret_cast<const float4*>(p.vc + base + (size_t)t0 * dh);
        __syncthreads();   // (the previous tile has been read)
        constexpr int U = 4;
        for (int i0 = tid; i0 < n4; i0 += U * kLmSplitThreads) {
            float4 kk[U], vv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * kLmSplitThreads;
                kk[u] = make_float4(0.f, 0.f, 0.f, 0.f); vv[u] = kk[u];
                if (i < n4) { kk[u] = kg[i]; vv[u] = vg[i]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * kLmSplitThreads;
                if (i < n4) {
                    const int row = i / dh4, c = i - row * dh4;
                    *reinterpret_cast<float4*>(ks + row * ldk + c * 4) = kk[u];
                    reinterpret_cast<float4*>(vs)[i] = vv[u];
                }
            }
        }
        __syncthreads();
        float cs[HPW];
#pragma unroll
        for (int h = 0; h < HPW; ++h) {
            const int g = wave * HPW + h;
            cs[h] = 0.0f;
            if (g < GT && g0 + g < G) {   // (uniform over the wave)
                float s = 0.0f;
                if (lane < nk) {
                    const float4* kr = reinterpret_cast<const float4*>(ks + lane * ldk);
                    const float4* qr = reinterpret_cast<const float4*>(qs + g * dh);
                    for (int c = 0; c < dh4; ++c) {
                        const float4 k4 = kr[c], q4 = qr[c];
                        s = fmaf(q4.x, k4.x, s); s = fmaf(q4.y, k4.y, s); s = fmaf(q4.z, k4.z, s); s = fmaf(q4.w, k4.w, s);
                    }
                }
                s = lane < nk ? s * p.scale : -INFINITY;
                const float mn = fmaxf(m[h], split_wave_max(s));
                const float e = expf(s - mn);             // (0 for a lane without a key)
                ps[g * TK + lane] = e;
                const float c = expf(m[h] - mn);          // (m = -inf at the span's first tile: 0)
                l[h] = l[h] * c + split_wave_sum(e);
                m[h] = mn;
                cs[h] = c;
            }
        }
        __syncthreads();   // (a wave reads its own weights only: this orders its LDS writes before its reads)
        float t[HPW][2];
#pragma unroll
        for (int h = 0; h < HPW; ++h) { t[h][0] = 0.0f; t[h][1] = 0.0f; }
        if (wave * HPW < GT && g0 + wave * HPW < G) {
#pragma unroll 4
            for (int j = 0; j < nk; ++j) {
                const float v0 = d0 ? vs[j * dh + lane] : 0.0f, v1 = d1 ? vs[j * dh + lane + 64] : 0.0f;
#pragma unroll
                for (int h = 0; h < HPW; ++h) {
                    const int g = wave * HPW + h;
                    const float pj = (g < GT && g0 + g < G) ? ps[g * TK + j] : 0.0f;   // (uniform over the wave; a head beyond the group has no weights)
                    t[h][0] = fmaf(pj, v0, t[h][0]);
                    t[h][1] = fmaf(pj, v1, t[h][1]);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < HPW; ++h) {
            acc[h][0] = acc[h][0] * cs[h] + t[h][0];
            acc[h][1] = acc[h][1] * cs[h] + t[h][1];
        }
    }
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
        const int g = wave * HPW + h;
        if (g < GT && g0 + g < G) {
            float* w = p.ws + (((size_t)b * p.H + (size_t)(kvh * G + g0 + g)) * p.nsmax + span) * (size_t)(dh + 2);
            if (lane == 0) { w[0] = m[h]; w[1] = l[h]; }
            if (d0) w[2 + lane] = acc[h][0];
            if (d1) w[2 + lane + 64] = acc[h][1];
        }
    }
}

__global__ __launch_bounds__(kLmMergeThreads) void lm_attn_merge_kernel(LmSplitP p) {
    if (*p.alive == 0) return;
    const int d = (int)threadIdx.x, head = (int)blockIdx.x, b = (int)blockIdx.y, dh = p.dh;
    const LmRow& R = p.st->rows[b];
    const int ns = (R.pos + p.S) / p.S;   // ceil((p + 1) / S): the spans lm_attn_split has written for this row
    if (d >= dh) return;
    const float* w = p.ws + ((size_t)b * p.H + head) * p.nsmax * (size_t)(dh + 2);
    float M = w[0];
#pragma unroll 8
    for (int i = 1; i < ns; ++i) M = fmaxf(M, w[(size_t)i * (dh + 2)]);   // (independent loads: several in flight)
    float L = 0.0f, O = 0.0f;
#pragma unroll 8
    for (int i = 0; i < ns; ++i) {
        const float* wi = w + (size_t)i * (dh + 2);
        const float c = expf(wi[0] - M);
        L = L + wi[1] * c;
        O = O + wi[2 + d] * c;
    }
    p.o[(size_t)b * p.o_ld + head * dh + d] = O / L;
}

}  // namespace

void lm_attention_split(hipStream_t s, const LmAttnArgs& g, int nrows, bool prefill, int max_pos_in_step) {
    OAR_CHECK(g.ws && lm_split_keys_supported(g.split_keys) && lm_head_dim_supported(g.dh) && nrows >= 1 && nrows <= kLmRows && max_pos_in_step >= 0 && max_pos_in_step < g.maxpos,
              OAR_INTERNAL, "lm_attention_split: workspace, span, head size, rows or positions outside the kernels' limits");
    const int G = g.H / g.KVH, gt = lm_split_gt(G), Hd = g.H * g.dh, Kd = g.KVH * g.dh;
    LmSplitP p{};
    p.st = g.st; p.q = g.q; p.q_ld = g.q_ld; p.kc = g.kc; p.vc = g.vc; p.H = g.H; p.KVH = g.KVH; p.dh = g.dh; p.maxpos = g.maxpos; p.S = g.split_keys;
    p.nsmax = lm_split_spans(g.maxpos, g.split_keys); p.gchunks = (G + gt - 1) / gt; p.scale = 1.0f / sqrtf((float)g.dh); p.ws = g.ws; p.o = g.o; p.o_ld = g.o_ld; p.alive = g.alive;
    const int spans = lm_split_spans(max_pos_in_step + 1, g.split_keys);
    const double keys = (double)nrows * (max_pos_in_step + 1), part = 4.0 * nrows * g.H * (double)spans * (g.dh + 2);
    const size_t lds = lm_split_lds_bytes(g.dh, gt);
    {
        ProfScope ps(s, prefill ? "lm_prefill_attn_split" : "lm_attn_split", 4.0 * (2.0 * keys * Kd * p.gchunks + nrows * Hd) + part, 4.0 * keys * Hd);
        const dim3 grid((unsigned)spans, (unsigned)nrows, (unsigned)(g.KVH * p.gchunks));
        if (gt == 8) {
            OAR_MAX_LDS_ONCE(lm_attn_split_kernel<8>, 80 * 1024);
            hipLaunchKernelGGL(lm_attn_split_kernel<8>, grid, dim3(kLmSplitThreads), lds, s, p);
        } else if (gt == 4) {
            OAR_MAX_LDS_ONCE(lm_attn_split_kernel<4>, 80 * 1024);
            hipLaunchKernelGGL(lm_attn_split_kernel<4>, grid, dim3(kLmSplitThreads), lds, s, p);
        } else if (gt == 2) {
            OAR_MAX_LDS_ONCE(lm_attn_split_kernel<2>, 80 * 1024);
            hipLaunchKernelGGL(lm_attn_split_kernel<2>, grid, dim3(kLmSplitThreads), lds, s, p);
        } else {
            OAR_MAX_LDS_ONCE(lm_attn_split_kernel<1>, 80 * 1024);
            hipLaunchKernelGGL(lm_attn_split_kernel<1>, grid, dim3(kLmSplitThreads), lds, s, p);
        }
    }
    {
        ProfScope ps(s, prefill ? "lm_prefill_attn_merge" : "lm_attn_merge", part + 4.0 * nrows * Hd, 0);
        hipLaunchKernelGGL(lm_attn_merge_kernel, dim3((unsigned)g.H, (unsigned)nrows), dim3(kLmMergeThreads), 0, s, p);
    }
}

}  // namespace k
}  // namespace oar
