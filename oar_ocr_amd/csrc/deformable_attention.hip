// deformable_attention.hip -- multi-scale deformable attention (the cross-attention of an RT-DETR decoder layer) as ONE launch.  The engine's rewrite pass 3c
// (engine_rewrite.cc) emits it for the exported spelling  Split the value per level -> Transpose + Reshape to [N nh, c, h, w] -> GridSample with the grid 2 loc - 1 ->
// Concat -> Mul by the softmax weights -> ReduceSum  (DESIGN 4.34).  The value projection already writes [N, Lv, nh, c] with the c channels of a (location,
// head) contiguous, so a tap is read straight from there: neither the per-level copies, nor the channels-last conversions, nor the [N nh, c, Q, L P] sample
// tensor exist.
//
// Work split: one lane owns four consecutive output channels of one (n, q): c / 4 lanes per head, nh c / 4 lanes per query.  At RT-DETR's nh c = 256 a wave is
// exactly one query and its 1 KB output row one coalesced store; the c / 4 lanes of a head read one contiguous 4 c-byte run per corner (128 B at c = 32).
// Locations and weights of a head are the same for its lanes: those loads are broadcasts out of one cache line.  A lane loops over the L P samples in
// ascending (level, point) order and adds  weight * (t00 (wy0 wx0) + t01 (wy0 wx1) + t10 (wy1 wx0) + t11 (wy1 wx1)),  the op-by-op route's expression, with
// the pixel position ((g + 1) size - 1) / 2 of g = 2 loc - 1 formed as that route forms it.  The softmax over a head's L P logits is computed by every
// lane of the head itself, in three passes over the (cached) logits -- maximum, sum of expf, and expf / sum per sample -- so no weight array is held in
// registers (a run-time-indexed array would live in scratch) and no lane exchanges anything.  No atomics, no dependence on scheduling: two runs are bit-identical.
// f32 VALU throughout; no LDS, no scratch.
#include "common.h"
#include "kernels.h"
#include "kernels_dev.h"

namespace oar {
namespace k {

namespace {

__global__ __launch_bounds__(kDefThreads) void deformable_attention_kernel(DeformAttnP p, unsigned total) {
    const unsigned t = blockIdx.x * (unsigned)kDefThreads + threadIdx.x;
    if (t >= total) return;
    const int lanes_h = p.c >> 2, lanes_q = p.nh * lanes_h;
    const int nq = (int)(t / (unsigned)lanes_q), r = (int)(t - (unsigned)nq * (unsigned)lanes_q), head = r / lanes_h, c4 = r - head * lanes_h;
    const int n = nq / p.Q, LP = p.L * p.P;
    const size_t hq = (size_t)nq * p.nh + head;                       // (n, q, head)
    const float* wr = p.w + hq * LP;
    const float2* lr = reinterpret_cast<const float2*>(p.loc) + hq * LP;
    float m = 0.0f, sum = 1.0f;
    if (p.softmax) {
        m = wr[0];
        for (int i = 1; i < LP; ++i) m = fmaxf(m, wr[i]);
        sum = 0.0f;
        for (int i = 0; i < LP; ++i) sum += expf(wr[i] - m);
    }
    const size_t ld = (size_t)p.nh * p.c;                             // floats between two locations of the value
    const float* vb = p.value + (size_t)n * p.Lv * ld + (size_t)head * p.c + (size_t)c4 * 4;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int l = 0; l < p.L; ++l) {
        // (selected, not indexed: a run-time index into the by-value argument would put the three arrays into scratch)
        const int W = l == 0 ? p.wd[0] : l == 1 ? p.wd[1] : l == 2 ? p.wd[2] : p.wd[3], H = l == 0 ? p.h[0] : l == 1 ? p.h[1] : l == 2 ? p.h[2] : p.h[3];
        const int st = l == 0 ? p.start[0] : l == 1 ? p.start[1] : l == 2 ? p.start[2] : p.start[3];
        const float Wf = (float)W, Hf = (float)H;
        const float* vl = vb + (size_t)st * ld;
        for (int pt = 0; pt < p.P; ++pt) {
            const int i = l * p.P + pt;
            const float2 xy = lr[i];
            const float wv = wr[i];
            const float gx = xy.x * 2.0f - 1.0f, gy = xy.y * 2.0f - 1.0f;                     // the graph's grid
            const float fx = ((gx + 1.0f) * Wf - 1.0f) * 0.5f, fy = ((gy + 1.0f) * Hf - 1.0f) * 0.5f;
            const float x0f = floorf(fx), y0f = floorf(fy), x1f = x0f + 1.0f, y1f = y0f + 1.0f;
            const float wx1 = fx - x0f, wy1 = fy - y0f, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
            // in float, before any conversion: a NaN or an infinity fails every comparison's conjunction and is never turned into an integer
            const bool bx0 = x0f >= 0.0f && x0f < Wf, bx1 = x1f >= 0.0f && x1f < Wf, by0 = y0f >= 0.0f && y0f < Hf, by1 = y1f >= 0.0f && y1f < Hf;
            const int x0 = bx0 ? (int)x0f : 0, x1 = bx1 ? (int)x1f : 0, y0 = by0 ? (int)y0f : 0, y1 = by1 ? (int)y1f : 0;
            float4 t00 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), t01 = t00, t10 = t00, t11 = t00;
            if (by0 && bx0) t00 = *reinterpret_cast<const float4*>(vl + (size_t)(y0 * W + x0) * ld);
            if (by0 && bx1) t01 = *reinterpret_cast<const float4*>(vl + (size_t)(y0 * W + x1) * ld);
            if (by1 && bx0) t10 = *reinterpret_cast<const float4*>(vl + (size_t)(y1 * W + x0) * ld);
            if (by1 && bx1) t11 = *reinterpret_cast<const float4*>(vl + (size_t)(y1 * W + x1) * ld);
            const float a = p.softmax ? expf(wv - m) / sum : wv;
            const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
            acc.x += (t00.x * w00 + t01.x * w01 + t10.x * w10 + t11.x * w11) * a;
            acc.y += (t00.y * w00 + t01.y * w01 + t10.y * w10 + t11.y * w11) * a;
            acc.z += (t00.z * w00 + t01.z * w01 + t10.z * w10 + t11.z * w11) * a;
            acc.w += (t00.w * w00 + t01.w * w01 + t10.w * w10 + t11.w * w11) * a;
        }
    }
    *reinterpret_cast<float4*>(p.y + (size_t)t * 4) = acc;            // lane t owns floats [4 t, 4 t + 4) of y [N Q][nh c]
}

}  // namespace

bool deformable_attention_supported(int64_t N, int64_t Q, int64_t nh, int64_t c, int64_t L, int64_t P, int64_t Lv) {
    if (N < 1 || Q < 1 || nh < 1 || c < 4 || (c & 3) || c > kDefMaxC || L < 1 || L > kDefMaxLevels || P < 1 || L * P > kDefMaxSamples || Lv < 1) return false;
    const int64_t lim = (int64_t)1 << 31;
    if (nh >= lim / c || N >= lim || Q >= lim || Lv >= lim) return false;
    return N * Lv < lim && N * Q < lim / (nh * c / 4);               // tokens of the value; threads
}

void deformable_attention(hipStream_t s, const DeformAttnP& p) {
    OAR_CHECK(deformable_attention_supported(p.N, p.Q, p.nh, p.c, p.L, p.P, p.Lv), OAR_UNSUPPORTED_OP, "DeformableAttention: shape outside the kernel's limits");
    int64_t rows = 0;
    for (int l = 0; l < p.L; ++l) {
        OAR_CHECK(p.h[l] >= 1 && p.wd[l] >= 1 && p.start[l] == rows, OAR_INTERNAL, "DeformableAttention: the levels do not tile the value");
        rows += (int64_t)p.h[l] * p.wd[l];
    }
    OAR_CHECK(rows == p.Lv, OAR_INTERNAL, "DeformableAttention: the levels do not sum to the value's length");
    OAR_CHECK(p.value && p.loc && p.w && p.y && ((uintptr_t)p.value & 15) == 0 && ((uintptr_t)p.y & 15) == 0 && ((uintptr_t)p.loc & 7) == 0, OAR_INTERNAL,
              "DeformableAttention: bad or misaligned arguments");
    const unsigned total = (unsigned)((int64_t)p.N * p.Q * p.nh * (p.c / 4));
    const double samples = (double)p.N * p.Q * p.nh * p.L * p.P;
    // bytes: four corners of c floats per sample (what the taps need when nothing is cached), a location pair and a weight per sample, the output row
    ProfScope ps(s, "deformable_attention", 4.0 * (samples * (4.0 * p.c + 3.0) + (double)p.N * p.Q * p.nh * p.c), samples * (9.0 * p.c + 24.0));
    hipLaunchKernelGGL(deformable_attention_kernel, dim3((total + kDefThreads - 1) / kDefThreads), dim3(kDefThreads), 0, s, p, total);
}

}  // namespace k
}  // namespace oar
