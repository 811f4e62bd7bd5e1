// lm_logits.h -- repetition penalty and no-repeat-ngram in front of the greedy choice (lm_logits.hip): sizes, the kernel's arguments and the launchers.
// Plain C++ (no HIP header): the host, the checks that need no device and the host-only resource test compile it.
//
// Per sequence the device keeps hist[cap] (the caller's prompt ids, then every token fed back), seen[ceil(V / 32)] (bit t: id t is in hist) and the prompt part's
// length hlen; a step that gives token `gen` of a sequence sees H = hlen + gen ids.  lm_select_kernel, one workgroup per head row between the lm-head and
// lm_combine: (a) appends the token the step before fed back (tokens[gen - 1], or its forced token), (b) marks the continuations of every earlier occurrence of the
// last n - 1 ids in an LDS bitmap, (c) streams the row's V logits of the step buffer once with the seen words beside them -- x < 0 ? x r : x / r for a seen id,
// -inf for a banned one -- and reduces to (value, lowest index), (d) writes that one candidate where lm_combine reads a one-partial array.
#pragma once
#include <cstddef>
#include <cstdint>

#include "lm_decode.h"

namespace oar {
namespace k {

constexpr int kLmSelectThreads = 1024;            // one workgroup pulls a whole row of logits: as many waves as a workgroup holds
constexpr int kLmSelectUnroll = 4;                // quads (16 bytes) of a thread in flight together
constexpr int kLmSelectWaves = kLmSelectThreads / 64;
constexpr int kLmSelectMaxVocab = 1 << 19;        // the ban bitmap of a row lives in LDS: 64 KiB at this vocabulary
constexpr int kLmHistoryMax = 65536;              // ids of a sequence's history that the caller may give

inline int lm_select_words(int V) { return (V + 31) >> 5; }
inline int lm_select_ld(int V) { return lm_pad4(V); }                                       // floats of one row of the step logits buffer (rows start 16-byte aligned)
inline size_t lm_select_lds_bytes(int V, int ngram) { return ngram > 1 ? (size_t)lm_select_words(V) * 4 : 0; }   // dynamic LDS: the ban bitmap
inline size_t lm_select_static_lds_bytes() { return (size_t)kLmSelectWaves * 8; }
inline int lm_launches_per_step_select(int L, bool split) { return (split ? 6 : 5) * L + 3; }

struct LmSelectP {
    const LmStep* st;
    const LmState* state;        // null: no alive / done guard (the direct entry)
    const float* logits; int ld; // the step buffer: row `slot` of the step at logits + slot * ld
    int V, words;
    int32_t* hist; int cap;      // [16][cap]
    const int32_t* hlen;         // [16]: ids of the prompt part
    uint32_t* seen;              // [16][words]
    const int32_t* tokens; const int32_t* forced; int max_new;   // the call's token table and forced tokens ([sequences][max_new]; forced may be null)
    float penalty; int ngram;
    void* part;                  // float2 [16]: head row b's candidate
    int32_t* tok_out;            // null, or [16]: the token lm_combine would take from the candidate
};

// the lm-head of a step with processors: lm_head's launch, the row's logits also to step_logits[slot]
void lm_head_step(ihipStream_t* s, const LmDecodeP& p, const LmStep* st, int nhead, bool prefill);
void lm_select(ihipStream_t* s, const LmSelectP& p, int nhead, bool prefill);

}  // namespace k
}  // namespace oar
