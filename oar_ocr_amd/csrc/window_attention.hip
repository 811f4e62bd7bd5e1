// window_attention.hip -- the attention of one Swin block (UniMERNet's encoder; plain, padded, shifted and masked windows) as ONE launch.  The engine's rewrite pass 3b
// (engine_rewrite.cc) emits it for the spelling  window partition -> q / k / v Linear -> per-window multi-head attention with an additive relative-position bias ->
// projection -> window reverse:  a Linear is per token, so the three projections read the tokens in image order and this kernel gathers a window's rows by
// address -- neither partition copy, nor the reverse copy, nor any permuted copy of q, k, v or the output exists.
//
// One workgroup of 256 threads (4 waves) per (window, head).  It stages the head's K and V rows of the window in LDS (K rows padded to an odd stride: lane j
// reads key j, so an even stride would put the 64 lanes on few banks), then every wave takes query rows i = wave, wave + 4, ...: lane j (+ 64, + 128, + 192)
// forms q_i . k_j with fmaf over d, applies the scale where the graph had it (Div or Mul) and adds bias[head][i][j]; max, expf, sum and divide over the wave;
// the probabilities go through LDS, and the weighted value sum runs over 64 / dhp lane groups (dhp: head_dim rounded up to a power of two) that take every
// (64 / dhp)-th key in ascending order and are combined by a fixed shuffle tree: run-to-run identical.  f32 VALU throughout; a (window, head) is a few hundred
// kFLOP, and what the op-by-op route costs is launches and bytes, not matrix throughput.
// LDS (dynamic): N (dh | 1) + N dh + 4 * 64 + 4 N floats, N = ws^2: 71,680 bytes at the largest shapes (N = 256, dh = 32; N = 128, dh = 64 needs 70,144),
// opted in above 64 KB.  No scratch.
// Padded and shifted windows are address arithmetic as well: window_token_row (kernels.h) maps a window's local token through the roll to its
// row in image order, or to "padding".  A padding token is staged as a key whose K / V rows are the k / v Linears' biases (the graph pads in front of the
// Linears) and takes part in the soft-max; as a query it is skipped, inside the uniform trip count.  The per-window mask is read from global memory like the
// bias and added behind it.  All of this is run-time fields of the one kernel: it costs 4 VGPRs (60 against 56), and a second kernel would double the code.
#include "common.h"
#include "kernels.h"
#include "kernels_dev.h"

namespace oar {
namespace k {

namespace {

__global__ __launch_bounds__(kWinThreads) void window_attention_kernel(WindowAttnP p) {
    extern __shared__ float4 wa_lds4[];
    const int ws = p.ws, N = ws * ws, dh = p.dh, ks = dh | 1;
    float* Ks = reinterpret_cast<float*>(wa_lds4);   // [N][ks]
    float* Vs = Ks + N * ks;                         // [N][dh]
    float* qs = Vs + N * dh;                         // [waves][kWinMaxDh]
    float* ps = qs + kWinWaves * kWinMaxDh;            // [waves][N]
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, head = (int)blockIdx.y, win = (int)blockIdx.x;
    const int wb = p.Wp / ws;
    const int b = win / p.nW, wi = win - b * p.nW, wy = wi / wb, wx = wi - wy * wb;
    const size_t img0 = (size_t)b * p.H * p.W;       // the image's token (0, 0)
    auto row = [&](int n) { return window_token_row(wy, wx, n, ws, p.H, p.W, p.Hp, p.Wp, p.shift); };   // within the image; -1: padding
    const int col0 = head * dh;
    if (p.Hp == p.H && p.Wp == p.W) {                // no padding: every token is real, and the loads of the loop's iterations stay independent of any branch
        for (int e = tid; e < N * dh; e += kWinThreads) {
            const int j = e / dh, d = e - j * dh;
            const size_t g = img0 + row(j);
            Ks[j * ks + d] = p.k[g * p.ldk + col0 + d];
            Vs[j * dh + d] = p.v[g * p.ldv + col0 + d];
        }
    } else {
        for (int e = tid; e < N * dh; e += kWinThreads) {
            const int j = e / dh, d = e - j * dh, g = row(j);
            float kv, vv;
            if (g >= 0) {
                kv = p.k[(img0 + g) * p.ldk + col0 + d];
                vv = p.v[(img0 + g) * p.ldv + col0 + d];
            } else {                                 // a padding token went through the Linears as zeros: its key and value are their biases
                kv = p.kbias ? p.kbias[col0 + d] : 0.0f;
                vv = p.vbias ? p.vbias[col0 + d] : 0.0f;
            }
            Ks[j * ks + d] = kv;
            Vs[j * dh + d] = vv;
        }
    }
    int dhp = 1;
    while (dhp < dh) dhp <<= 1;
    const int G = 64 / dhp, grp = lane / dhp, dl = lane & (dhp - 1);
    const float* bias = p.bias + (size_t)head * N * N;
    const float* mask = p.mask ? p.mask + (size_t)wi * N * N : nullptr;
    const float* qr = qs + wave * kWinMaxDh;
    float* pr = ps + wave * N;
    for (int i0 = 0; i0 < N; i0 += kWinWaves) {       // (uniform trip count: the barriers are reached by every wave)
        const int i = i0 + wave;
        const int gi = i < N ? row(i) : -1;
        const bool on = gi >= 0;                     // (a padding query is skipped: nothing is written for it)
        __syncthreads();                             // K / V are staged; the previous row's q and probabilities have been read
        if (on && lane < dh) qs[wave * kWinMaxDh + lane] = p.q[(img0 + gi) * p.ldq + col0 + lane];
        __syncthreads();
        float sc[kWinMaxN / 64];
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < kWinMaxN / 64; ++t) {
            const int j = lane + 64 * t;
            float a = -INFINITY;
            if (on && j < N) {
                const float* kr = Ks + j * ks;
                const float bv = bias[(size_t)i * N + j];                       // (both loads are issued in front of the dot product, which hides them)
                const float mv = mask ? mask[(size_t)i * N + j] : 0.0f;
                a = 0.0f;
                for (int d = 0; d < dh; ++d) a = fmaf(qr[d], kr[d], a);
                a = p.scale_div ? a / p.scale : a * p.scale;
                a = a + bv;
                if (mask) a = a + mv;
            }
            sc[t] = a;
            m = fmaxf(m, a);
        }
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < kWinMaxN / 64; ++t) {
            const int j = lane + 64 * t;
            float e = 0.0f;
            if (on && j < N) e = expf(sc[t] - m);
            sc[t] = e;
            s += e;
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
#pragma unroll
        for (int t = 0; t < kWinMaxN / 64; ++t) {
            const int j = lane + 64 * t;
            if (on && j < N) pr[j] = sc[t] / s;
        }
        __syncthreads();
        float a = 0.0f;
        if (on && dl < dh)
            for (int j = grp; j < N; j += G) a = fmaf(pr[j], Vs[j * dh + dl], a);
        for (int o = 32; o >= dhp; o >>= 1) a += __shfl_xor(a, o, 64);
        if (on && lane < dh) p.o[(img0 + gi) * p.ldo + col0 + lane] = a;   // (lane < dh <= dhp: group 0, dl == lane)
    }
}

}  // namespace

bool window_attention_supported(int ws, int heads, int head_dim) {
    if (ws < 1 || ws > 16 || heads < 1 || heads > 65535 || head_dim < 1 || head_dim > kWinMaxDh) return false;
    return ws * ws <= kWinMaxN && ws * ws * head_dim <= kWinMaxNd;
}

void window_attention(hipStream_t s, const WindowAttnP& p) {
    OAR_CHECK(window_attention_supported(p.ws, p.nh, p.dh) && p.B >= 1 && p.H >= 1 && p.W >= 1 && p.Hp >= p.H && p.Wp >= p.W && p.Hp % p.ws == 0 && p.Wp % p.ws == 0 &&
                  p.Hp - p.H < p.ws && p.Wp - p.W < p.ws && p.shift >= 0 && p.shift < std::min(p.Hp, p.Wp) && (int64_t)p.nW == (int64_t)(p.Hp / p.ws) * (p.Wp / p.ws),
              OAR_UNSUPPORTED_OP, "WindowAttention: shape outside the kernel's limits");
    const int N = p.ws * p.ws, C = p.nh * p.dh;
    OAR_CHECK(p.ldq >= C && p.ldk >= C && p.ldv >= C && p.ldo >= C && p.q && p.k && p.v && p.bias && p.o, OAR_INTERNAL, "WindowAttention: bad arguments");
    OAR_CHECK((int64_t)p.B * p.H * p.W <= 0x7fffffff && (int64_t)p.Hp * p.Wp <= 0x7fffffff, OAR_UNSUPPORTED_OP, "WindowAttention: too many tokens");
    const int64_t windows = (int64_t)p.B * p.nW;
    OAR_CHECK(windows <= 0x7fffffff, OAR_UNSUPPORTED_OP, "WindowAttention: too many windows");
    const size_t lds = window_attention_lds_bytes(N, p.dh);   // (the kernel carves its four arrays in the order of that sum)
    if (lds > 64 * 1024) OAR_MAX_LDS_ONCE(window_attention_kernel, 72 * 1024);
    const double tokens = (double)p.B * p.H * p.W;   // real tokens: a padding token costs neither a query nor a row of q, k, v or o
    ProfScope ps(s, "window_attention", 4.0 * (4.0 * tokens * C + (double)windows * p.nh * N * N * (p.mask ? 2 : 1)), 4.0 * tokens * N * C);
    hipLaunchKernelGGL(window_attention_kernel, dim3((unsigned)windows, (unsigned)p.nh), dim3(kWinThreads), lds, s, p);
}

}  // namespace k
}  // namespace oar
