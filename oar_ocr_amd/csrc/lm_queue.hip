// lm_queue.hip -- the turnover of a cache slot between two sequences of a queued generation (lm_queue.h).  The chain (lm_decode.hip) indexes tokens,
// forced tokens, logits, `done` and the decode row by R.seq, which is the slot here; between the old sequence's last step and the new one's first row, in stream
// order, one launch per scheduling point
//   copies the slot's token row to the retired sequence's output row (eos from the tokens the chain wrote up to max_new) and its logits rows likewise (zero rows
//   behind those the chain wrote), zeroes the slot's token and logits rows, clears done[slot] and copies the admitted sequence's forced tokens into the slot's row.
// grid (workgroups per entry, entries): workgroup x of an entry takes the 16-byte groups x, x + gridDim.x, ... of the logits; workgroup 0 also the token rows.
// Every element is read, written and zeroed by one thread: no atomics, no LDS, no order between workgroups.  Rows are moved 16 bytes at a time when a row's
// length is a multiple of 4 elements (the buffers' bases are 256-byte aligned), element by element otherwise.
#include "common.h"
#include "lm_queue.h"

namespace oar {
namespace k {

namespace {

__global__ __launch_bounds__(kLmQueueThreads) void lm_queue_turnover_kernel(LmQueueTurnP p) {
    const LmQueueTurn T = p.turn[blockIdx.y];
    const int tid = (int)threadIdx.x, MN = p.max_new;
    if (blockIdx.x == 0) {
        int32_t* st = p.slot_tokens + (size_t)T.slot * MN;
        int32_t* ot = T.out_seq >= 0 ? p.out_tokens + (size_t)T.out_seq * MN : nullptr;
        int32_t* sf = p.slot_forced && T.in_seq >= 0 ? p.slot_forced + (size_t)T.slot * MN : nullptr;
        const int32_t* af = sf ? p.all_forced + (size_t)T.in_seq * MN : nullptr;
        if ((MN & 3) == 0) {
            for (int q = tid; q < (MN >> 2); q += kLmQueueThreads) {
                if (ot) {
                    int4 v = reinterpret_cast<const int4*>(st)[q];
                    const int g = q << 2;
                    if (g + 0 >= T.produced) v.x = p.eos;
                    if (g + 1 >= T.produced) v.y = p.eos;
                    if (g + 2 >= T.produced) v.z = p.eos;
                    if (g + 3 >= T.produced) v.w = p.eos;
                    reinterpret_cast<int4*>(ot)[q] = v;
                }
                reinterpret_cast<int4*>(st)[q] = make_int4(0, 0, 0, 0);
                if (sf) reinterpret_cast<int4*>(sf)[q] = reinterpret_cast<const int4*>(af)[q];
            }
        } else {
            for (int g = tid; g < MN; g += kLmQueueThreads) {
                if (ot) ot[g] = g < T.produced ? st[g] : p.eos;
                st[g] = 0;
                if (sf) sf[g] = af[g];
            }
        }
        if (tid == 0) p.state->done[T.slot] = 0;
    }
    if (!p.slot_logits || T.out_seq < 0) return;   // (a slot that held no sequence has zero rows)
    const size_t n = (size_t)MN * p.V, live = (size_t)T.produced * p.V;   // elements of a sequence's logits; those the chain wrote
    float* sl = p.slot_logits + (size_t)T.slot * n;
    float* ol = p.out_logits + (size_t)T.out_seq * n;
    const size_t stride = (size_t)gridDim.x * kLmQueueThreads, i0 = (size_t)blockIdx.x * kLmQueueThreads + tid;
    if ((n & 3) == 0) {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (size_t q = i0; q < (n >> 2); q += stride) {
            const size_t e = q << 2;
            float4 v = zero;
            if (e < live) {
                v = reinterpret_cast<const float4*>(sl)[q];
                if (e + 1 >= live) v.y = 0.f;
                if (e + 2 >= live) v.z = 0.f;
                if (e + 3 >= live) v.w = 0.f;
            }
            reinterpret_cast<float4*>(ol)[q] = v;
            reinterpret_cast<float4*>(sl)[q] = zero;
        }
    } else {
        for (size_t e = i0; e < n; e += stride) {
            ol[e] = e < live ? sl[e] : 0.f;
            sl[e] = 0.f;
        }
    }
}

}  // namespace

void lm_queue_turnover(hipStream_t s, const LmQueueTurnP& p) {
    OAR_CHECK(p.n_turn >= 1 && p.n_turn <= kLmRows && p.turn && p.slot_tokens && p.out_tokens && p.state && p.max_new >= 1 && (!p.slot_logits || p.out_logits) &&
                  (!p.slot_forced || p.all_forced),
              OAR_INTERNAL, "lm_queue_turnover: entries outside 1..16 or a missing buffer");
    const int nb = lm_queue_turnover_blocks(p.max_new, p.V, p.slot_logits != nullptr);
    ProfScope ps(s, "lm_queue_turnover", (double)p.n_turn * (4.0 * 4 * p.max_new + (p.slot_logits ? 3.0 * 4 * p.max_new * p.V : 0.0)), 0);
    hipLaunchKernelGGL(lm_queue_turnover_kernel, dim3((unsigned)nb, (unsigned)p.n_turn), dim3(kLmQueueThreads), 0, s, p);
}

}  // namespace k
}  // namespace oar
