// vis_misc.hip -- the small steps around the vision encoder's Linears and attention: the position table resampled to every image's grid, and the
// 2 x 2 (m x m) gather in front of the projector.  One thread per float4 of an output row; the images of a call are found by a scan over at most 16 starts.
#include "common.h"
#include "kernels.h"

namespace oar {
namespace k {

namespace {

__device__ __forceinline__ int vis_image_of(const VisGrids& g, int row) {
    int i = 0;
    while (i + 1 < g.n && row >= g.start[i + 1]) ++i;
    return i;
}

__device__ __forceinline__ void vis_axis(int o, int out, int G, int& i0, int& i1, float& w0, float& w1) {
    float c = ((float)o + 0.5f) * (float)G / (float)out - 0.5f;
    c = fminf(fmaxf(c, 0.0f), (float)(G - 1));
    i0 = (int)floorf(c);
    i1 = min(i0 + 1, G - 1);
    w1 = c - (float)i0;
    w0 = 1.0f - w1;
}

__global__ __launch_bounds__(256) void vis_pos_embed_kernel(const float* __restrict__ table, float* __restrict__ out, VisGrids g, int G, int D4, int total) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= total) return;
    const int row = idx / D4, f = idx - row * D4;
    const int im = vis_image_of(g, row), local = row - g.start[im], w = g.w[im];
    const int oy = local / w, ox = local - oy * w;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    vis_axis(oy, g.h[im], G, y0, y1, wy0, wy1);
    vis_axis(ox, w, G, x0, x1, wx0, wx1);
    const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
    const float4* t = reinterpret_cast<const float4*>(table);
    const float4 a = t[(size_t)(y0 * G + x0) * D4 + f], b = t[(size_t)(y0 * G + x1) * D4 + f], c = t[(size_t)(y1 * G + x0) * D4 + f], d = t[(size_t)(y1 * G + x1) * D4 + f];
    float4 r;
    r.x = a.x * w00 + b.x * w01 + c.x * w10 + d.x * w11;
    r.y = a.y * w00 + b.y * w01 + c.y * w10 + d.y * w11;
    r.z = a.z * w00 + b.z * w01 + c.z * w10 + d.z * w11;
    r.w = a.w * w00 + b.w * w01 + c.w * w10 + d.w * w11;
    reinterpret_cast<float4*>(out)[(size_t)row * D4 + f] = r;
}

// one thread per float4 of the INPUT: row (image, y, x) goes to output row start / m^2 + (y / m) (w / m) + x / m, at column ((y % m) m + x % m) D
__global__ __launch_bounds__(256) void vis_merge_gather_kernel(const float* __restrict__ x, float* __restrict__ out, VisGrids g, int m, int D4, int total) {
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= total) return;
    const int row = idx / D4, f = idx - row * D4;
    const int im = vis_image_of(g, row), local = row - g.start[im], w = g.w[im];
    const int y = local / w, xx = local - y * w;
    const int orow = g.start[im] / (m * m) + (y / m) * (w / m) + xx / m, slot = (y % m) * m + xx % m;
    reinterpret_cast<float4*>(out)[((size_t)orow * (m * m) + slot) * D4 + f] = reinterpret_cast<const float4*>(x)[(size_t)row * D4 + f];
}

void check_grids(const VisGrids& g, int D, const char* what) {
    OAR_CHECK(g.n >= 1 && g.n <= kVisMaxImages && D > 0 && D % 4 == 0 && g.start[0] == 0, OAR_INTERNAL, std::string(what) + ": bad image table");
    for (int i = 0; i < g.n; ++i)
        OAR_CHECK(g.h[i] >= 1 && g.w[i] >= 1 && g.start[i + 1] - g.start[i] == g.h[i] * g.w[i], OAR_INTERNAL, std::string(what) + ": bad image table");
    OAR_CHECK((int64_t)g.start[g.n] * (D / 4) < ((int64_t)1 << 31), OAR_INTERNAL, std::string(what) + ": too many elements");
}

}  // namespace

void vis_pos_embed(hipStream_t s, const float* table, float* out, const VisGrids& g, int G, int D) {
    check_grids(g, D, "vis_pos_embed");
    OAR_CHECK(table && out && G >= 1, OAR_INTERNAL, "vis_pos_embed: bad arguments");
    const int total = g.start[g.n] * (D / 4);
    ProfScope ps(s, "vis_embed", 4.0 * ((double)G * G * D + (double)total * 4), 7.0 * total * 4);
    hipLaunchKernelGGL(vis_pos_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, table, out, g, G, D / 4, total);
}

void vis_merge_gather(hipStream_t s, const float* x, float* out, const VisGrids& g, int m, int D) {
    check_grids(g, D, "vis_merge_gather");
    OAR_CHECK(x && out && m >= 1, OAR_INTERNAL, "vis_merge_gather: bad arguments");
    for (int i = 0; i < g.n; ++i) OAR_CHECK(g.h[i] % m == 0 && g.w[i] % m == 0, OAR_INTERNAL, "vis_merge_gather: a grid is no multiple of the merge size");
    const int total = g.start[g.n] * (D / 4);
    ProfScope ps(s, "vis_project", 32.0 * total, 0.0);
    hipLaunchKernelGGL(vis_merge_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, out, g, m, D / 4, total);
}

}  // namespace k
}  // namespace oar
