// lm_queue.h -- queued generation on the language-model chain: any number of sequences share the model's <= 16 cache slots, and a slot whose
// sequence has ended is handed to the next waiting one.  The scheduler (lm_queue.cc) is host code that builds one LmStep per step; the chain (lm_decode.hip) runs
// it unchanged with R.seq = the slot; lm_queue_turnover (lm_queue.hip) moves a slot's token / logits rows to the retired sequence's output rows and prepares the
// slot for the admitted one.  Plain C++ (no HIP header): the host-only test compiles the scheduler with a driver of its own.
//
// Seeing `done`: behind every kLmQueueStride-th step the host enqueues a copy of LmState into a pinned ring and records an event; before it builds step i it waits
// only for the newest copy taken at a step <= i - kLmQueueLookahead, so the device keeps a lookahead of queued steps.  A `done` flag counts only when that copy
// was taken at or behind the step in front of which the slot's present sequence was admitted (the turnover in front of that step cleared the flag).
// The guarantee: a sequence gets at most kLmQueueLookahead + kLmQueueStride decode rows after the step that produced its eos (exactly: at most
// kLmQueueLookahead + kLmQueueStride - 2).  Every pinned ring (LmState copies, LmQueueStage tables, GEMM-phase tables) has kLmQueueRing entries, entry i mod
// kLmQueueRing for step i: the wait in front of step i proves every copy enqueued up to step i - kLmQueueRing finished.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lm_decode.h"
#include "lm_prefill.h"

struct ihipStream_t;

namespace oar {
namespace k {

#ifndef OAR_LM_QUEUE_STRIDE      // (a build option for the measurement of DESIGN 4.44: build.py's OAR_LM_QUEUE_LAG)
#define OAR_LM_QUEUE_STRIDE 1
#define OAR_LM_QUEUE_LOOKAHEAD 2
#endif
constexpr int kLmQueueStride = OAR_LM_QUEUE_STRIDE, kLmQueueLookahead = OAR_LM_QUEUE_LOOKAHEAD;   // the measurement: DESIGN 4.44
static_assert(kLmQueueStride >= 1 && kLmQueueLookahead >= 1, "the host looks at a copy at least one step behind the enqueue");
constexpr int kLmQueueRing = kLmQueueLookahead + kLmQueueStride;
constexpr int kLmQueueMaxSeq = 65535;
constexpr int kLmQueueThreads = 256;          // turnover kernel
constexpr int kLmQueueVecPerThread = 8;       // 16-byte accesses a thread of the turnover kernel is sized for
constexpr int kLmQueueMaxBlocks = 2048;       // workgroups per turnover entry at the most

// copy c is taken behind step (c + 1) kLmQueueStride - 1; the newest copy the host may wait for before it builds step i (-1: none yet)
inline int64_t lm_queue_copy_step(int64_t c) { return (c + 1) * kLmQueueStride - 1; }
inline int64_t lm_queue_copy_for(int64_t i) { return i < kLmQueueLookahead ? -1 : (i - kLmQueueLookahead + 1) / kLmQueueStride - 1; }

// One waiting sequence: prompt length, the arena row of its first prompt position, the rotary position of its first generated token, its position ids
// ([3][len], or null: 0 .. len - 1 on all axes).
struct LmQueueSeq { int32_t len, xrow0, next_pos; const int32_t* pid; };
// One turnover: the slot's rows go to sequence out_seq (-1: the slot was free), which got `produced` decode rows' tokens; sequence in_seq (-1: none) moves in.
struct LmQueueTurn { int32_t slot, out_seq, produced, in_seq; };
// What one scheduling point uploads: the step and the turnovers in front of it (one pinned ring entry, one device copy).
struct LmQueueStage { LmStep step; LmQueueTurn turn[kLmRows]; };
struct LmQueueAdmit { int32_t slot, seq; };
struct LmQueueStats { int64_t steps, rows, dead_rows, admissions, gemm_phases, max_dead_rows, min_slot_admissions, min_slot_turnovers; };

class LmQueue {
public:
    LmQueue(const LmQueueSeq* seqs, int n_seq, int slots, int max_new, bool gemm, int xdec0);
    int64_t step() const { return step_; }   // index of the step the next scheduling point builds
    // The scheduling point in front of step step(): retires, admits, builds the step.  done: the LmState::done of the newest copy the host has seen (null: none),
    // taken behind step done_step.  st.turn[0 .. n_turn) are the turnovers, gemm: the admitted sequences whose positions 0 .. len - 2 take the GEMM phase (in
    // slot order).  False: no step is left (st.turn may still hold the last retirements).
    bool next(const int32_t* done, int64_t done_step, LmQueueStage& st, int& n_turn, int& max_pos, std::vector<LmQueueAdmit>& gemm);
    const std::vector<int32_t>& produced() const { return produced_; }   // per sequence: tokens the chain wrote before it retired
    int64_t rows() const { return rows_; }
    int64_t admissions() const { return admissions_; }
    int64_t min_slot_admissions() const;   // the fewest sequences one slot held
    int64_t min_slot_turnovers() const;    // the fewest turnover entries one slot got (a slot that held one sequence got two: in and out)
private:
    enum : int { FREE = 0, PREFILL = 1, DECODE = 2 };
    struct Slot { int state; int32_t seq, pp, gen; int64_t admit_step, admissions, turnovers; };
    std::vector<LmQueueSeq> seqs_;
    std::vector<int32_t> produced_;
    Slot slot_[kLmRows];
    int slots_, max_new_, xdec0_, next_seq_ = 0;
    bool gemm_;
    int64_t step_ = 0, rows_ = 0, admissions_ = 0;
};

// The packed GEMM phase of one scheduling point's admissions: the rows (positions 0 .. len - 2 of every admitted sequence, seq = its slot), cut into chunks of
// chunk_rows, and every chunk's attention tiles.  rows / tiles are filled from their start; false when they would not fit rows_cap / tiles_cap.
struct LmQueuePhase { std::vector<int> chunk; std::vector<size_t> tile0; size_t n_rows = 0, n_tiles = 0; };
bool lm_queue_pack(const LmQueueSeq* seqs, const LmQueueAdmit* adm, int n_adm, int chunk_rows, int heads, LmPfRow* rows, size_t rows_cap, LmPfTile* tiles, size_t tiles_cap,
                   LmQueuePhase& ph);
// Bounds of one phase's tables for these prompt lengths: at most `slots` sequences are admitted at one point.
void lm_queue_phase_caps(const int32_t* lengths, int n_seq, int slots, int chunk_rows, int heads, size_t* rows_cap, size_t* tiles_cap);

// lm_queue.hip
struct LmQueueTurnP {
    const LmQueueTurn* turn; int n_turn;
    int32_t* slot_tokens; int32_t* out_tokens;        // [slots][max_new], [n_seq][max_new]
    int32_t* slot_forced; const int32_t* all_forced;  // the same shapes, or null
    float* slot_logits; float* out_logits;            // [.][max_new][V], or null
    LmState* state;
    int max_new, V, eos;
};
// workgroups per entry: one without logits, else one per kLmQueueThreads x kLmQueueVecPerThread 16-byte groups of a sequence's max_new x V floats
inline int lm_queue_turnover_blocks(int max_new, int V, bool logits) {
    if (!logits) return 1;
    const size_t vec = ((size_t)max_new * (size_t)V + 3) / 4, per = (size_t)kLmQueueThreads * kLmQueueVecPerThread;
    const size_t b = (vec + per - 1) / per;
    return (int)(b < 1 ? 1 : b > (size_t)kLmQueueMaxBlocks ? (size_t)kLmQueueMaxBlocks : b);
}
void lm_queue_turnover(ihipStream_t* s, const LmQueueTurnP& p);

}  // namespace k
}  // namespace oar
