// add_layernorm.hip -- residual add + LayerNorm over the last axis as ONE launch:  s = a + b,  y = LN(s) * gamma + beta, s stored only when
// a later reader wants it.  a, y and s are [rows][C]; row r of b is b[(r % b_rows) * C ...] with b_rows | rows, so a same-shape operand (b_rows = rows), a
// [1, T, C] positional table (b_rows = T) and a [C] vector (b_rows = 1) are the same kernel.
//
// The arithmetic and the order of every sum are those of k::layernorm (kernels.hip) applied to the f32 sum, and the build has -ffp-contract=off
// -fno-fast-math: a launch is bit-identical to k::binary (Add) followed by k::layernorm, which is what the tests hold it to.
//   4 | C <= 1024 and every pointer 16-byte aligned: half a wave per row, the row in registers as float4s (layernorm_v4_kernel's form): each operand read
//     once, 16-byte accesses, two rows per wave in flight, eight rows per workgroup.
//   anything else: one wave per row, 4-byte accesses, the operands re-read through the cache (layernorm_kernel's form).
// A pure bandwidth kernel with no reuse between workgroups: no XCD remap.
#include "common.h"
#include "kernels.h"

namespace oar {
namespace k {

namespace {

__device__ __forceinline__ float aln_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per row
template <bool WS>
__global__ __launch_bounds__(256) void add_layernorm_kernel(const float* a, const float* b, long b_rows, const float* g, const float* be, float* sum, float* y, long rows, int C, float eps) {
    long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* ar = a + row * C;
    const float* br = b + (row % b_rows) * C;
    float s = 0.f;
    for (int i = lane; i < C; i += 64) {
        const float x = ar[i] + br[i];
        if (WS) sum[row * C + i] = x;
        s += x;
    }
    float mean = aln_wave_sum(s) / (float)C;
    float v = 0.f;
    for (int i = lane; i < C; i += 64) { float d = (ar[i] + br[i]) - mean; v += d * d; }
    float var = aln_wave_sum(v) / (float)C;
    float inv = 1.0f / sqrtf(var + eps);
    for (int i = lane; i < C; i += 64) {
        float t = ((ar[i] + br[i]) - mean) * inv;
        if (g) t *= g[i];
        if (be) t += be[i];
        y[row * C + i] = t;
    }
}

// half a wave per row, the summed row in registers
template <int NV, bool WS>
__global__ __launch_bounds__(256) void add_layernorm_v4_kernel(const float4* __restrict__ a, const float4* __restrict__ b, long b_rows, const float4* __restrict__ g, const float4* __restrict__ be,
                                                               float4* __restrict__ sum, float4* __restrict__ y, long rows, int C4, float invC, float eps) {
    const long row = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (row >= rows) return;
    const int l = threadIdx.x & 31;
    const float4* ar = a + row * C4;
    const float4* br = b + (row % b_rows) * C4;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = l + 32 * i;
        if (j < C4) {
            const float4 p = ar[j], q = br[j];
            v[i] = make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w);
            if (WS) sum[row * C4 + j] = v[i];
        } else {
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 32);
    const float mean = s * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (l + 32 * i < C4) {
            const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
            q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 32);
    const float inv = 1.0f / sqrtf(q * invC + eps);
    float4* yr = y + row * C4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = l + 32 * i;
        if (j >= C4) continue;
        float4 t = make_float4((v[i].x - mean) * inv, (v[i].y - mean) * inv, (v[i].z - mean) * inv, (v[i].w - mean) * inv);
        if (g) { const float4 gg = g[j]; t.x *= gg.x; t.y *= gg.y; t.z *= gg.z; t.w *= gg.w; }
        if (be) { const float4 bb = be[j]; t.x += bb.x; t.y += bb.y; t.z += bb.z; t.w += bb.w; }
        yr[j] = t;
    }
}

template <int NV>
void launch_v4(hipStream_t s, dim3 grid, const float* a, const float* b, long b_rows, const float* gamma, const float* beta, float* sum_out, float* y, long rows, int C4, float invC, float eps) {
    auto A = reinterpret_cast<const float4*>(a); auto B = reinterpret_cast<const float4*>(b); auto G = reinterpret_cast<const float4*>(gamma);
    auto E = reinterpret_cast<const float4*>(beta); auto S = reinterpret_cast<float4*>(sum_out); auto Y = reinterpret_cast<float4*>(y);
    if (sum_out) hipLaunchKernelGGL((add_layernorm_v4_kernel<NV, true>), grid, dim3(256), 0, s, A, B, b_rows, G, E, S, Y, rows, C4, invC, eps);
    else hipLaunchKernelGGL((add_layernorm_v4_kernel<NV, false>), grid, dim3(256), 0, s, A, B, b_rows, G, E, S, Y, rows, C4, invC, eps);
}

}  // namespace

void add_layernorm(hipStream_t s, const float* a, const float* b, int64_t b_rows, const float* gamma, const float* beta, float* sum_out, float* y, int64_t rows, int C, float eps) {
    if (rows == 0) return;
    const double small = 4.0 * C * ((b_rows == rows ? 0.0 : (double)b_rows) + (gamma ? 1.0 : 0.0) + (beta ? 1.0 : 0.0));
    ProfScope ps(s, "add_layernorm", 4.0 * (double)rows * C * (2 + (b_rows == rows ? 1 : 0) + (sum_out ? 1 : 0)) + small, 9.0 * (double)rows * C);
    static const bool v4 = [] { const char* e = getenv("OAR_LN_V4"); return !e || atoi(e) != 0; }();   // (k::layernorm's switch: the two routes take the same form)
    const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(sum_out) | reinterpret_cast<uintptr_t>(y) |
                           reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta)) & 15) == 0;
    if (v4 && (C & 3) == 0 && C <= 1024 && aligned) {
        const int C4 = C / 4, nv = (C4 + 31) / 32;
        const dim3 grid((unsigned)((rows + 7) / 8));
        const float invC = 1.0f / (float)C;
        if (nv <= 1) launch_v4<1>(s, grid, a, b, (long)b_rows, gamma, beta, sum_out, y, (long)rows, C4, invC, eps);
        else if (nv <= 2) launch_v4<2>(s, grid, a, b, (long)b_rows, gamma, beta, sum_out, y, (long)rows, C4, invC, eps);
        else if (nv <= 3) launch_v4<3>(s, grid, a, b, (long)b_rows, gamma, beta, sum_out, y, (long)rows, C4, invC, eps);
        else if (nv <= 4) launch_v4<4>(s, grid, a, b, (long)b_rows, gamma, beta, sum_out, y, (long)rows, C4, invC, eps);
        else launch_v4<8>(s, grid, a, b, (long)b_rows, gamma, beta, sum_out, y, (long)rows, C4, invC, eps);
        return;
    }
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (sum_out) hipLaunchKernelGGL(add_layernorm_kernel<true>, grid, dim3(256), 0, s, a, b, (long)b_rows, gamma, beta, sum_out, y, (long)rows, C, eps);
    else hipLaunchKernelGGL(add_layernorm_kernel<false>, grid, dim3(256), 0, s, a, b, (long)b_rows, gamma, beta, sum_out, y, (long)rows, C, eps);
}

}  // namespace k
}  // namespace oar
