// qvis_misc.hip -- the steps of the Qwen2-VL / Qwen2.5-VL vision towers that the SigLIP chain never needed: RMSNorm over rows, the MLP's
// activation (plain, or act(gate) * up over a stacked gate / up result), and a row gather for the merge-unit permutation into window order and back.
// Bandwidth kernels: float4 accesses, no LDS, no atomics; every index is guarded by the row and column counts the launcher was given.
#include "common.h"
#include "kernels_dev.h"
#include "qvis.h"

namespace oar {
namespace k {

namespace {

constexpr int kQvisThreads = 256, kQvisWave = 64;

// one wave per row: pass 1 sums the squares (a lane's float4s in turn, then a butterfly over the wave: the same order whatever the grid), pass 2 rereads
// the row -- from the cache, it was read a moment ago -- and scales it
__global__ __launch_bounds__(kQvisThreads) void qvis_rmsnorm_kernel(const float* x, const float* __restrict__ g, float* y, long rows, int D4, float inv_d, float eps) {
    const long row = (long)blockIdx.x * (kQvisThreads / kQvisWave) + (threadIdx.x / kQvisWave);
    if (row >= rows) return;   // (wave-uniform: the butterfly below runs in whole waves)
    const int lane = (int)(threadIdx.x % kQvisWave);
    const float4* xr = reinterpret_cast<const float4*>(x) + (size_t)row * D4;
    float acc = 0.0f;
    for (int i = lane; i < D4; i += kQvisWave) {
        const float4 v = xr[i];
        acc += v.x * v.x;
        acc += v.y * v.y;
        acc += v.z * v.z;
        acc += v.w * v.w;
    }
    for (int off = kQvisWave / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, kQvisWave);
    const float r = 1.0f / sqrtf(acc * inv_d + eps);
    const float4* gr = reinterpret_cast<const float4*>(g);
    float4* yr = reinterpret_cast<float4*>(y) + (size_t)row * D4;
    for (int i = lane; i < D4; i += kQvisWave) {
        const float4 v = xr[i], w = gr[i];
        float4 o;
        o.x = v.x * r * w.x; o.y = v.y * r * w.y; o.z = v.z * r * w.z; o.w = v.w * r * w.w;
        yr[i] = o;
    }
}

template <int ACT>
__device__ __forceinline__ float qvis_act1(float v) {
    if (ACT == QVIS_QUICK_GELU) return v * (1.0f / (1.0f + expf(-1.702f * v)));
    if (ACT == QVIS_SILU) return v * (1.0f / (1.0f + expf(-v)));
    return 0.5f * v * (1.0f + erf_rational(v * 0.70710678118654752440f));   // (apply_act's ACT_GELU_ERF, the implicit-GEMM epilogue's form)
}

// one thread per float4 of the output; in_ld4 is F / 4 (plain) or 2 F / 4 (gated), the up half F4 float4s behind the gate half
template <int ACT, bool GATED>
__global__ __launch_bounds__(kQvisThreads) void qvis_act_kernel(const float* in, float* out, long total, int F4) {
    const long idx = (long)blockIdx.x * kQvisThreads + threadIdx.x;
    if (idx >= total) return;
    const long row = idx / F4;
    const int f = (int)(idx - row * F4);
    const float4* ir = reinterpret_cast<const float4*>(in) + (size_t)row * (GATED ? 2 * F4 : F4);
    const float4 a = ir[f];
    float4 o;
    o.x = qvis_act1<ACT>(a.x); o.y = qvis_act1<ACT>(a.y); o.z = qvis_act1<ACT>(a.z); o.w = qvis_act1<ACT>(a.w);
    if (GATED) {
        const float4 u = ir[F4 + f];
        o.x *= u.x; o.y *= u.y; o.z *= u.z; o.w *= u.w;
    }
    reinterpret_cast<float4*>(out)[idx] = o;
}

__global__ __launch_bounds__(kQvisThreads) void qvis_row_gather_kernel(const float* __restrict__ in, const int* __restrict__ idx, float* __restrict__ out, long total, int R4, long n_in_rows) {
    const long i = (long)blockIdx.x * kQvisThreads + threadIdx.x;
    if (i >= total) return;
    const long row = i / R4;
    const int f = (int)(i - row * R4);
    const long src = idx[row];
    if (src < 0 || src >= n_in_rows) return;
    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(in)[(size_t)src * R4 + f];
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

unsigned blocks_for(int64_t total, int per_block, const char* what) {
    const int64_t n = (total + per_block - 1) / per_block;
    OAR_CHECK(n >= 1 && n < ((int64_t)1 << 31), OAR_INTERNAL, std::string(what) + ": too many elements for one launch");
    return (unsigned)n;
}

template <int ACT>
void launch_act(hipStream_t s, const float* in, float* out, int64_t total, int F4, bool gated, unsigned blocks) {
    if (gated) hipLaunchKernelGGL((qvis_act_kernel<ACT, true>), dim3(blocks), dim3(kQvisThreads), 0, s, in, out, (long)total, F4);
    else hipLaunchKernelGGL((qvis_act_kernel<ACT, false>), dim3(blocks), dim3(kQvisThreads), 0, s, in, out, (long)total, F4);
}

}  // namespace

void qvis_rmsnorm(hipStream_t s, const float* x, const float* g, float* y, int64_t rows, int D, float eps, const char* prof_class) {
    OAR_CHECK(x && g && y && rows >= 1 && D >= 4 && D % 4 == 0 && aligned16(x, g, y), OAR_INTERNAL, "qvis_rmsnorm: bad arguments");
    const unsigned blocks = blocks_for(rows, kQvisThreads / kQvisWave, "qvis_rmsnorm");
    ProfScope ps(s, prof_class ? prof_class : "qvis_rmsnorm", 8.0 * (double)rows * D + 4.0 * D, 4.0 * (double)rows * D);
    hipLaunchKernelGGL(qvis_rmsnorm_kernel, dim3(blocks), dim3(kQvisThreads), 0, s, x, g, y, (long)rows, D / 4, 1.0f / (float)D, eps);
}

void qvis_act(hipStream_t s, const float* in, float* out, int64_t rows, int F, int act, int gated, const char* prof_class) {
    OAR_CHECK(in && out && rows >= 1 && F >= 4 && F % 4 == 0 && aligned16(in, out) && qvis_act_known(act), OAR_INTERNAL, "qvis_act: bad arguments");
    const int64_t total = rows * (F / 4);
    const unsigned blocks = blocks_for(total, kQvisThreads, "qvis_act");
    ProfScope ps(s, prof_class ? prof_class : "qvis_act", 4.0 * (double)rows * F * (gated ? 3.0 : 2.0), (double)rows * F * 8.0);
    if (act == QVIS_QUICK_GELU) launch_act<QVIS_QUICK_GELU>(s, in, out, total, F / 4, gated != 0, blocks);
    else if (act == QVIS_SILU) launch_act<QVIS_SILU>(s, in, out, total, F / 4, gated != 0, blocks);
    else launch_act<QVIS_GELU_ERF>(s, in, out, total, F / 4, gated != 0, blocks);
}

void qvis_row_gather(hipStream_t s, const float* in, const int32_t* idx, float* out, int64_t n_rows, int64_t n_in_rows, int row_floats, const char* prof_class) {
    OAR_CHECK(in && idx && out && n_rows >= 1 && n_in_rows >= 1 && row_floats >= 4 && row_floats % 4 == 0 && aligned16(in, out), OAR_INTERNAL, "qvis_row_gather: bad arguments");
    const int64_t total = n_rows * (row_floats / 4);
    const unsigned blocks = blocks_for(total, kQvisThreads, "qvis_row_gather");
    ProfScope ps(s, prof_class ? prof_class : "qvis_row_gather", 8.0 * (double)n_rows * row_floats + 4.0 * n_rows, 0.0);
    hipLaunchKernelGGL(qvis_row_gather_kernel, dim3(blocks), dim3(kQvisThreads), 0, s, in, idx, out, (long)total, row_floats / 4, (long)n_in_rows);
}

}  // namespace k
}  // namespace oar
