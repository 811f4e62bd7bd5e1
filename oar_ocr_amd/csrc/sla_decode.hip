// sla_decode.hip -- the SLANet structure head (PaddleOCR SLAHead._decode: AttentionGRUCell + GRUCell + the two output
// heads) as ONE launch: every step of the greedy recurrence, all images.  The engine's Loop rewrite (engine_loops.cc, match_sla_loop) emits it.
//
// One workgroup of 1024 threads (16 waves, one CU) per image; images are independent, so there is no communication
// between workgroups and nothing ever waits on global memory.  The workgroup walks all M steps; the phases of a step are
// separated by __syncthreads:
//   1  h4   = [W_h2h ; W_hh] h + [b_h2h ; b_hh]                 4H rows x H     (hp | hr hz hc: everything that reads only h)
//   2  e[j] = sum_k tanh(proj[j][k] + hp[k]) * w_score[k]       HW rows x H     the largest phase: HW * H tanh
//   3  alpha = softmax(e)                                       block max, exp, block sum
//   4  ctx  = alpha^T fea                                       wave w: rows w, w + 16, ...; lanes: columns; 16 partials summed in wave order
//   5  xg   = W_ih[:, :C] ctx + W_ih[:, C + pre] + b_ih         3H rows x C     the one-hot product is a gather of one column
//   6  r, z, c, h = (h - c) z + c                               H threads
//   7  s1 | l1 = [W_s1 ; W_l1] h + b                            2H rows x H
//   8  logits = W_s2 s1 + b, loc = sigmoid(W_l2 l1 + b)         V + L rows x H  written to the scan outputs [M][B][.]
//   9  pre  = argmax(logits), the lowest index among equal values
// Matrix-vector products: a group of G lanes (a power of two <= 64, the row length in float4s rounded up) owns an output
// row, reads it with 16-byte loads against the vector in LDS and reduces across the group with shuffles.  The weights are
// repacked on the host with their rows padded to a multiple of four floats (zeros), the LDS vectors are padded with zeros
// likewise, so every weight load is an aligned float4.  proj and fea are activations: 16-byte loads when their row length
// and base address allow, scalar loads otherwise.
// State in LDS (floats): h Hp | h4 4H | e / alpha HW | ctx Cp | xg 3H | s1 l1 2 Hp | logits V | ctx partials 16 C: 63.5 KB at the largest
// supported shape (H = C = 512, V = HW = 1024), 23 KB for the SLANet_plus head.  Weights and proj (2.4 MB per step for that head)
// stream from L2 every step.  f32 throughout; products are fused (fmaf) only inside the dot products, the gate arithmetic keeps
// the reference's operation order.
#include "common.h"
#include "kernels.h"

namespace oar {
namespace k {

namespace {

constexpr int kSlaThreads = 1024, kSlaWaves = kSlaThreads / 64;

__device__ __forceinline__ float group_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + expf(-v)); }

// out(r, W[r] . x) for r < rows; W [rows][4 * K4] row-major in global memory, x [4 * K4] in LDS, both 16-byte aligned.
// Every thread runs the same number of iterations: the shuffles always see whole waves.
template <typename F>
__device__ __forceinline__ void gemv_rows(const float* __restrict__ W, int K4, const float* x, int rows, int G, F&& out) {
    const int tid = (int)threadIdx.x, g = tid / G, l = tid & (G - 1), ng = kSlaThreads / G;
    const float4* xv = reinterpret_cast<const float4*>(x);
    for (int r0 = 0; r0 < rows; r0 += ng) {
        const int r = r0 + g;
        float acc = 0.0f;
        if (r < rows) {
            const float4* wr = reinterpret_cast<const float4*>(W + (size_t)r * (size_t)K4 * 4);
            for (int q = l; q < K4; q += G) {
                const float4 w = wr[q], v = xv[q];
                acc = fmaf(w.x, v.x, acc); acc = fmaf(w.y, v.y, acc); acc = fmaf(w.z, v.z, acc); acc = fmaf(w.w, v.w, acc);
            }
        }
        acc = group_sum(acc, G);
        if (r < rows && l == 0) out(r, acc);
    }
}

__device__ __forceinline__ int group_for(int n) {   // lanes per row: the smallest power of two >= n, at most a wave
    int g = 1;
    while (g < n && g < 64) g <<= 1;
    return g;
}

__global__ __launch_bounds__(kSlaThreads) void sla_decode_kernel(SlaDecodeP p, int vec_proj) {
    extern __shared__ float4 sla_lds4[];
    __shared__ float red_a[kSlaWaves], red_b[kSlaWaves], red_v[kSlaWaves];
    __shared__ int red_i[kSlaWaves];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int B = p.B, HW = p.HW, C = p.C, H = p.H, V = p.V, L = p.L;
    const int Hp = (H + 3) & ~3, Cp = (C + 3) & ~3, H3 = 3 * H;
    auto pad4 = [](int n) { return (n + 3) & ~3; };
    float* h = reinterpret_cast<float*>(sla_lds4);            // [Hp]
    float* h4 = h + Hp;                                        // [4H]: hp | hr | hz | hc
    float* e = h4 + pad4(4 * H);                               // [HW]: scores, then alpha
    float* ctx = e + pad4(HW);                                 // [Cp]
    float* xg = ctx + Cp;                                      // [3H]
    float* sl1 = xg + pad4(H3);                                // [2 Hp]: s1 | l1
    float* lg = sl1 + 2 * Hp;                                  // [V]
    float* part = lg + pad4(V);                                // [16][C]
    const int b = (int)blockIdx.x;
    const float* fea = p.fea + (size_t)b * HW * C;
    const float* proj = p.proj + (size_t)b * HW * H;

    for (int i = tid; i < Hp; i += kSlaThreads) h[i] = i < H ? p.h0[(size_t)b * H + i] : 0.0f;
    for (int i = tid; i < Cp; i += kSlaThreads) ctx[i] = 0.0f;
    for (int i = tid; i < 2 * Hp; i += kSlaThreads) sl1[i] = 0.0f;
    int pre = (int)p.pre0[b];
    __syncthreads();

    const int g_h = group_for(Hp / 4), g_c = group_for(Cp / 4);
    for (int step = 0; step < p.M; ++step) {
        // 1: everything that reads only h
        gemv_rows(p.w_h4, Hp / 4, h, 4 * H, g_h, [&](int r, float v) { h4[r] = v + p.b_h4[r]; });
        __syncthreads();
        // 2: attention scores
        if (vec_proj) {
            const int K4 = H / 4, G = g_h, g = tid / G, l = tid & (G - 1), ng = kSlaThreads / G;
            const float4* hpv = reinterpret_cast<const float4*>(h4);
            const float4* wsv = reinterpret_cast<const float4*>(p.w_score);
            for (int j0 = 0; j0 < HW; j0 += ng) {
                const int j = j0 + g;
                float acc = 0.0f;
                if (j < HW) {
                    const float4* pr = reinterpret_cast<const float4*>(proj + (size_t)j * H);
                    for (int q = l; q < K4; q += G) {
                        const float4 a = pr[q], hv = hpv[q], w = wsv[q];
                        acc = fmaf(tanhf(a.x + hv.x), w.x, acc); acc = fmaf(tanhf(a.y + hv.y), w.y, acc);
                        acc = fmaf(tanhf(a.z + hv.z), w.z, acc); acc = fmaf(tanhf(a.w + hv.w), w.w, acc);
                    }
                }
                acc = group_sum(acc, G);
                if (j < HW && l == 0) e[j] = acc;
            }
        } else {
            const int G = group_for(H), g = tid / G, l = tid & (G - 1), ng = kSlaThreads / G;
            for (int j0 = 0; j0 < HW; j0 += ng) {
                const int j = j0 + g;
                float acc = 0.0f;
                if (j < HW)
                    for (int q = l; q < H; q += G) acc = fmaf(tanhf(proj[(size_t)j * H + q] + h4[q]), p.w_score[q], acc);
                acc = group_sum(acc, G);
                if (j < HW && l == 0) e[j] = acc;
            }
        }
        __syncthreads();
        // 3: softmax over the HW positions (HW <= 1024: one per thread)
        {
            const float v = tid < HW ? e[tid] : -INFINITY;
            float m = v;
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            if (lane == 0) red_a[wave] = m;
            __syncthreads();
            m = red_a[0];
            for (int w = 1; w < kSlaWaves; ++w) m = fmaxf(m, red_a[w]);
            const float ex = tid < HW ? expf(v - m) : 0.0f;
            float s = ex;
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) red_b[wave] = s;
            __syncthreads();
            s = red_b[0];
            for (int w = 1; w < kSlaWaves; ++w) s += red_b[w];
            if (tid < HW) e[tid] = ex / s;
        }
        __syncthreads();
        // 4: context vector
        {
            float acc[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = 0.0f;
            for (int j = wave; j < HW; j += kSlaWaves) {
                const float a = e[j];
                const float* fr = fea + (size_t)j * C;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int c = lane + 64 * q;
                    if (c < C) acc[q] = fmaf(a, fr[c], acc[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = lane + 64 * q;
                if (c < C) part[wave * C + c] = acc[q];
            }
            __syncthreads();
            if (tid < C) {
                float s = part[tid];
                for (int w = 1; w < kSlaWaves; ++w) s += part[w * C + tid];
                ctx[tid] = s;
            }
        }
        __syncthreads();
        // 5: input half of the GRU gates; the previous token selects one column of W_ih
        {
            const bool tok = pre >= 0 && pre < V;
            const float* col = p.w_ihv + (size_t)(tok ? pre : 0) * H3;
            gemv_rows(p.w_ihc, Cp / 4, ctx, H3, g_c, [&](int r, float v) { xg[r] = (v + (tok ? col[r] : 0.0f)) + p.b_ih[r]; });
        }
        __syncthreads();
        // 6: the GRU cell
        if (tid < H) {
            const float r = sigmoid_f(xg[tid] + h4[H + tid]), z = sigmoid_f(xg[H + tid] + h4[2 * H + tid]);
            const float c = tanhf(xg[2 * H + tid] + r * h4[3 * H + tid]);
            h[tid] = (h[tid] - c) * z + c;
        }
        __syncthreads();
        // 7: first layer of both heads
        gemv_rows(p.w_sl1, Hp / 4, h, 2 * H, g_h, [&](int r, float v) { sl1[r < H ? r : Hp + (r - H)] = v + p.b_sl1[r]; });
        __syncthreads();
        // 8: second layers, written to the scan outputs
        {
            float* lo = p.logits + ((size_t)step * B + b) * V;
            float* bo = p.loc + ((size_t)step * B + b) * L;
            gemv_rows(p.w_s2, Hp / 4, sl1, V, g_h, [&](int r, float v) { const float y = v + p.b_s2[r]; lg[r] = y; lo[r] = y; });
            gemv_rows(p.w_l2, Hp / 4, sl1 + Hp, L, g_h, [&](int r, float v) { bo[r] = sigmoid_f(v + p.b_l2[r]); });
        }
        __syncthreads();
        // 9: greedy token, the lowest index among equal logits (V <= 1024: one per thread)
        {
            float v = tid < V ? lg[tid] : -INFINITY;
            int ix = tid < V ? tid : 0x7fffffff;
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(v, o, 64);
                const int oi = __shfl_xor(ix, o, 64);
                if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
            }
            if (lane == 0) { red_v[wave] = v; red_i[wave] = ix; }
            __syncthreads();
            v = red_v[0]; ix = red_i[0];
            for (int w = 1; w < kSlaWaves; ++w) {
                const float ov = red_v[w];
                const int oi = red_i[w];
                if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
            }
            pre = ix;
        }
        // (red_v / red_i are next written after the barriers of the following step: no barrier needed here)
    }
    for (int i = tid; i < H; i += kSlaThreads) p.h_out[(size_t)b * H + i] = h[i];
    if (tid == 0) p.pre_out[b] = (float)pre;
}

}  // namespace

bool sla_decode_supported(int HW, int C, int H, int V, int L, int M) {
    return H >= 1 && H <= kSlaMaxH && C >= 1 && C <= kSlaMaxC && V >= 1 && V <= kSlaMaxV && HW >= 1 && HW <= kSlaMaxHW && L >= 1 && L <= kSlaMaxL && M >= 1 && M <= kSlaMaxM;
}

size_t sla_decode_lds_bytes(int HW, int C, int H, int V) {
    auto pad4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    const size_t Hp = pad4((size_t)H), Cp = pad4((size_t)C);
    return 4 * (Hp + pad4(4 * (size_t)H) + pad4((size_t)HW) + Cp + pad4(3 * (size_t)H) + 2 * Hp + pad4((size_t)V) + pad4((size_t)kSlaWaves * C));
}

void sla_decode(hipStream_t s, const SlaDecodeP& p) {
    OAR_CHECK(sla_decode_supported(p.HW, p.C, p.H, p.V, p.L, p.M), OAR_UNSUPPORTED_OP, "SLADecode: shape outside the kernel's limits");
    if (p.B <= 0) return;
    const size_t lds = sla_decode_lds_bytes(p.HW, p.C, p.H, p.V);
    OAR_CHECK(lds <= 64 * 1024, OAR_INTERNAL, "SLADecode: LDS plan exceeds 64 KB");
    const int vec_proj = (p.H % 4 == 0) && (reinterpret_cast<uintptr_t>(p.proj) & 15) == 0;
    // per step and image: the products of phases 1, 2, 4, 5, 7, 8 (2 flops each) and the bytes they stream
    const double macs = 4.0 * p.H * p.H + (double)p.HW * p.H + (double)p.HW * p.C + 3.0 * p.H * p.C + 2.0 * p.H * p.H + ((double)p.V + p.L) * p.H;
    const double bytes = 4.0 * (macs + 3.0 * p.H + p.V + p.L);
    ProfScope ps(s, "sla_decode", bytes * p.M * p.B, 2.0 * macs * p.M * p.B);
    hipLaunchKernelGGL(sla_decode_kernel, dim3((unsigned)p.B), dim3(kSlaThreads), lds, s, p, vec_proj);
}

}  // namespace k
}  // namespace oar
