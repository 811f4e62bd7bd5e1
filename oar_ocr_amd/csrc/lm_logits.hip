// lm_logits.hip -- repetition penalty and no-repeat-ngram in front of the language model's greedy choice, on the device so that every step of a call
// can still be enqueued up front.  Two kernels join a step of the chain (lm_decode.hip) when a processor is on:
//   lm_head_step   the lm-head (the body of lm_rows_dev.h, unchanged arithmetic) that writes a row's logits also to the step buffer [16][pad4(V)] at the row's slot;
//                  the caller's logits, when asked for, are written as before: they stay the raw logits
//   lm_select      one workgroup per head row: appends the token fed back by the step before to the sequence's history and presence bitmap, marks the banned
//                  continuations in an LDS bitmap, streams the row once (penalty on seen ids, -inf on banned ones) and leaves ONE (value, lowest index) candidate,
//                  which the unchanged lm_combine takes as a one-partial array: tokens, eos, alive and the next input row stay lm_combine's
// Only the workgroup of a sequence's row touches that sequence's history in a launch; integer LDS atomics mark the bans; no float atomics: two runs give the same
// bytes.  x / r is the correctly rounded division (hipcc's default; this file is built without any fast-division flag).
#include "lm_logits.h"
#include "lm_rows_dev.h"

namespace oar {
namespace k {

namespace {

template <int NB, typename WT>
__global__ __launch_bounds__(kLmThreads) void lm_head_step_kernel(LmRowsP p) { lm_rows_body<NB, LM_HEAD_STEP, WT>(p); }

__global__ __launch_bounds__(kLmSelectThreads) void lm_select_kernel(LmSelectP p) {
    extern __shared__ uint32_t ban_s[];   // [words] when ngram > 1
    __shared__ float red_v[kLmSelectWaves];
    __shared__ int red_i[kLmSelectWaves];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, b = (int)blockIdx.x;
    const int slot = p.st->head[b];
    const LmRow& R = p.st->rows[slot];
    const int seq = R.seq, gen = R.gen, V = p.V;
    // lm_combine's guards (uniform over the workgroup; only lm_combine, a launch of its own, writes them): it takes no candidate of such a row
    if (p.state && (p.state->alive == 0 || p.state->done[seq] != 0)) return;
    int32_t* h = p.hist + (size_t)seq * p.cap;
    uint32_t* sw = p.seen + (size_t)seq * p.words;
    int H = p.hlen[seq] + gen;   // ids this row sees: the prompt part and one id per earlier step
    if (H > p.cap) H = p.cap;    // (the host sizes cap to the prompt part + max_new)
    // (a) the token the step before fed back: every thread knows it, thread 0 stores it; nobody reads h[H - 1] or its seen bit from memory in this launch
    const bool app = gen > 0 && H > 0;
    int last = -1, lw = -1;
    uint32_t lb = 0;
    if (app) {
        int t = p.tokens[(size_t)seq * p.max_new + gen - 1];
        if (p.forced) {
            const int f = p.forced[(size_t)seq * p.max_new + gen - 1];
            if (f >= 0 && f < V) t = f;
        }
        last = t;
        if (t >= 0 && t < V) { lw = t >> 5; lb = 1u << (t & 31); }
        if (tid == 0) {
            h[H - 1] = t;
            if (lw >= 0) sw[lw] = sw[lw] | lb;
        }
    }
    auto at = [&](int i) { return (app && i == H - 1) ? last : h[i]; };
    // (b) bans: every i whose n - 1 ids equal the last n - 1 bans the id behind them
    const int n = p.ngram;
    const bool bans = n > 1 && H >= n;
    if (bans) {
        for (int w = tid; w < p.words; w += kLmSelectThreads) ban_s[w] = 0u;
        __syncthreads();
        const int m = n - 1;
        for (int i = tid; i <= H - n; i += kLmSelectThreads) {
            bool eq = true;
            for (int j = 0; j < m && eq; ++j) eq = at(i + j) == at(H - m + j);
            if (eq) {
                const int t = at(i + m);
                if (t >= 0 && t < V) atomicOr(&ban_s[t >> 5], 1u << (t & 31));
            }
        }
        __syncthreads();
    }
    // (c) one pass over the row, 16 bytes a thread: four logits share one nibble of a seen word and of a ban word
    const float* x = p.logits + (size_t)slot * p.ld;
    const float r = p.penalty;
    const bool pen = r != 1.0f;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    auto take = [&](float v, int idx, bool seen, bool banned) {
        if (seen) v = v < 0.0f ? v * r : v / r;
        if (banned) v = -INFINITY;
        if (better(v, idx, bv, bi)) { bv = v; bi = idx; }
    };
    const int nq = V >> 2;
    constexpr int U = kLmSelectUnroll;   // quads of a thread whose loads are in flight together: one workgroup has to pull the whole row
    for (int q0 = tid; q0 < nq; q0 += U * kLmSelectThreads) {
        float4 v[U];
        uint32_t sv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * kLmSelectThreads;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            sv[u] = 0u;
            if (q < nq) {
                v[u] = reinterpret_cast<const float4*>(x)[q];
                if (pen) sv[u] = sw[q >> 3];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * kLmSelectThreads;
            if (q < nq) {
                const int w = q >> 3, sh = (q & 7) * 4;
                uint32_t s = sv[u], bn = 0u;
                if (pen && w == lw) s |= lb;
                s = (s >> sh) & 15u;
                if (bans) bn = (ban_s[w] >> sh) & 15u;
                take(v[u].x, 4 * q, s & 1u, bn & 1u);
                take(v[u].y, 4 * q + 1, s & 2u, bn & 2u);
                take(v[u].z, 4 * q + 2, s & 4u, bn & 4u);
                take(v[u].w, 4 * q + 3, s & 8u, bn & 8u);
            }
        }
    }
    for (int i = (nq << 2) + tid; i < V; i += kLmSelectThreads) {   // the last V % 4 logits
        const int w = i >> 5;
        const uint32_t bit = 1u << (i & 31);
        uint32_t s = 0u;
        if (pen) { s = sw[w]; if (w == lw) s |= lb; }
        take(x[i], i, (s & bit) != 0u, bans && (ban_s[w] & bit) != 0u);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kLmSelectWaves; ++w)
            if (better(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
        // (d) the row's one candidate; an index that never won (every logit NaN) becomes token 0 in lm_combine
        reinterpret_cast<float2*>(p.part)[b] = make_float2(bv, __int_as_float(bi));
        if (p.tok_out) p.tok_out[b] = (bi < 0 || bi >= V) ? 0 : bi;
    }
}

template <typename WT, int NB>
void launch_head_step_nb(hipStream_t s, const LmRowsP& p, int wgs, size_t lds) {
    OAR_MAX_LDS_ONCE((lm_head_step_kernel<NB, WT>), 64 * 1024);
    hipLaunchKernelGGL((lm_head_step_kernel<NB, WT>), dim3((unsigned)wgs), dim3(kLmThreads), lds, s, p);
}

template <typename WT>
void launch_head_step(hipStream_t s, LmRowsP p, int B, bool prefill) {
    p.Kp = lm_pad4(p.K);
    p.groups = lm_groups_for(p.N);
    const int wgs = lm_wgs_for(p.N);
    p.nwg = wgs;
    const size_t lds = lm_rows_lds_bytes(B, p.K);
    const double wbytes = sizeof(WT) * (double)p.N * p.Kp;
    ProfScope ps(s, prefill ? "lm_prefill_head" : "lm_head", wbytes + 4.0 * B * ((double)p.K + 2.0 * p.N), 2.0 * (double)p.N * p.K * B);
    switch (lm_nb(B)) {
        case 1: launch_head_step_nb<WT, 1>(s, p, wgs, lds); break;
        case 2: launch_head_step_nb<WT, 2>(s, p, wgs, lds); break;
        case 4: launch_head_step_nb<WT, 4>(s, p, wgs, lds); break;
        case 8: launch_head_step_nb<WT, 8>(s, p, wgs, lds); break;
        default: launch_head_step_nb<WT, 16>(s, p, wgs, lds); break;
    }
}

}  // namespace

void lm_head_step(hipStream_t s, const LmDecodeP& p, const LmStep* st, int nhead, bool prefill) {
    LmRowsP r{};
    r.st = st; r.alive = &p.state->alive; r.xin = p.arena; r.xin_ld = p.D; r.xin_arena = 1; r.K = p.D; r.N = p.V; r.W = p.w_lm; r.rms_g = p.lnf; r.eps = p.eps;
    r.logits = p.logits; r.max_new = p.max_new; r.part = reinterpret_cast<float2*>(p.part);
    r.y = p.step_logits; r.y_ld = lm_select_ld(p.V);
    if (p.bf16) launch_head_step<uint16_t>(s, r, nhead, prefill);
    else launch_head_step<float>(s, r, nhead, prefill);
}

void lm_select(hipStream_t s, const LmSelectP& p, int nhead, bool prefill) {
    OAR_CHECK(nhead >= 1 && nhead <= kLmRows && p.V >= 1 && (p.ngram <= 1 || p.V <= kLmSelectMaxVocab) && p.ld >= p.V && (p.ld & 3) == 0 && p.words == lm_select_words(p.V), OAR_INTERNAL,
              "lm_select: rows, vocabulary or row stride outside the kernel's limits");
    const size_t lds = lm_select_lds_bytes(p.V, p.ngram);
    OAR_MAX_LDS_ONCE(lm_select_kernel, 64 * 1024);
    ProfScope ps(s, prefill ? "lm_prefill_select" : "lm_select", nhead * (4.0 * p.V + (p.penalty != 1.0f ? 4.0 * p.words : 0.0) + 4.0 * p.cap), 0);
    hipLaunchKernelGGL(lm_select_kernel, dim3((unsigned)nhead), dim3(kLmSelectThreads), lds, s, p);
}

}  // namespace k
}  // namespace oar
