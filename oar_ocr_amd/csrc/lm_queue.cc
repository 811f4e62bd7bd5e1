// lm_queue.cc -- the scheduler of queued generation (lm_queue.h).  Host code without a HIP call: the host-only test links it with a simulated device.
#include "lm_queue.h"

#include <algorithm>
#include <functional>

namespace oar {
namespace k {

LmQueue::LmQueue(const LmQueueSeq* seqs, int n_seq, int slots, int max_new, bool gemm, int xdec0)
    : seqs_(seqs, seqs + n_seq), produced_((size_t)n_seq, 0), slots_(slots), max_new_(max_new), xdec0_(xdec0), gemm_(gemm) {
    for (Slot& s : slot_) s = Slot{FREE, -1, 0, 0, 0, 0, 0};
}

int64_t LmQueue::min_slot_admissions() const {
    int64_t m = slot_[0].admissions;
    for (int s = 1; s < slots_; ++s) m = std::min(m, slot_[s].admissions);
    return m;
}

int64_t LmQueue::min_slot_turnovers() const {
    int64_t m = slot_[0].turnovers;
    for (int s = 1; s < slots_; ++s) m = std::min(m, slot_[s].turnovers);
    return m;
}

bool LmQueue::next(const int32_t* done, int64_t done_step, LmQueueStage& st, int& n_turn, int& max_pos, std::vector<LmQueueAdmit>& gemm) {
    st = LmQueueStage{};
    n_turn = 0; max_pos = 0;
    gemm.clear();
    int turn_of[kLmRows];
    // retirement: max_new tokens written (the host knows without looking), or a `done` flag that belongs to the slot's present sequence
    for (int s = 0; s < slots_; ++s) {
        Slot& S = slot_[s];
        turn_of[s] = -1;
        if (S.state != DECODE) continue;
        if (S.gen >= max_new_ || (done && done_step >= S.admit_step && done[s])) {
            produced_[(size_t)S.seq] = S.gen;
            turn_of[s] = n_turn;
            st.turn[n_turn++] = LmQueueTurn{s, S.seq, S.gen, -1};
            S.state = FREE;
            ++S.turnovers;
        }
    }
    // admission: request order into free slots in slot order
    for (int s = 0; s < slots_ && next_seq_ < (int)seqs_.size(); ++s) {
        Slot& S = slot_[s];
        if (S.state != FREE) continue;
        const int seq = next_seq_++;
        if (turn_of[s] < 0) { turn_of[s] = n_turn; st.turn[n_turn++] = LmQueueTurn{s, -1, 0, -1}; ++S.turnovers; }
        st.turn[turn_of[s]].in_seq = seq;
        const int T = seqs_[(size_t)seq].len;
        const bool phase = gemm_ && T > 1;   // positions 0 .. T - 2 go through the GEMM phase, the last joins the step
        S.state = PREFILL; S.seq = seq; S.pp = phase ? T - 1 : 0; S.gen = 0; S.admit_step = step_;
        ++S.admissions; ++admissions_;
        if (phase) gemm.push_back(LmQueueAdmit{s, seq});
    }
    // the step: one decode row per decoding slot, then prompt rows of the prefilling slots in (slot, position) order
    LmStep& cur = st.step;
    for (int s = 0; s < slots_; ++s) {
        Slot& S = slot_[s];
        if (S.state != DECODE) continue;
        const LmQueueSeq& Q = seqs_[(size_t)S.seq];
        LmRow& R = cur.rows[cur.nrows];
        R.seq = s; R.pos = Q.len + S.gen - 1; R.xrow = xdec0_ + s; R.gen = S.gen; R.pad = 0;
        R.rp[0] = R.rp[1] = R.rp[2] = Q.next_pos + S.gen - 1;
        cur.head[cur.nhead++] = cur.nrows++;
        max_pos = std::max(max_pos, (int)R.pos);
        ++S.gen;
    }
    for (int s = 0; s < slots_ && cur.nrows < kLmRows; ++s) {
        Slot& S = slot_[s];
        if (S.state != PREFILL) continue;
        const LmQueueSeq& Q = seqs_[(size_t)S.seq];
        while (S.pp < Q.len && cur.nrows < kLmRows) {
            const int t = S.pp++;
            LmRow& R = cur.rows[cur.nrows];
            R.seq = s; R.pos = t; R.xrow = Q.xrow0 + t; R.gen = t == Q.len - 1 ? 0 : -1; R.pad = 0;
            for (int a = 0; a < 3; ++a) R.rp[a] = Q.pid ? Q.pid[(size_t)a * Q.len + t] : t;
            if (R.gen >= 0) { cur.head[cur.nhead++] = cur.nrows; S.state = DECODE; S.gen = 1; }
            ++cur.nrows;
            max_pos = std::max(max_pos, t);
        }
    }
    if (cur.nrows == 0) return false;   // the queue is empty and every slot has retired
    rows_ += cur.nrows;
    ++step_;
    return true;
}

bool lm_queue_pack(const LmQueueSeq* seqs, const LmQueueAdmit* adm, int n_adm, int chunk_rows, int heads, LmPfRow* rows, size_t rows_cap, LmPfTile* tiles, size_t tiles_cap,
                   LmQueuePhase& ph) {
    ph = LmQueuePhase{};
    std::vector<int32_t> lengths((size_t)n_adm);
    size_t n = 0;
    for (int i = 0; i < n_adm; ++i) {
        const LmQueueSeq& Q = seqs[adm[i].seq];
        lengths[(size_t)i] = Q.len;
        if (n + (size_t)(Q.len - 1) > rows_cap) return false;
        for (int t = 0; t < Q.len - 1; ++t) {
            LmPfRow& R = rows[n++];
            R = LmPfRow{adm[i].slot, t, {t, t, t}, Q.xrow0 + t, {0, 0}};
            if (Q.pid)
                for (int a = 0; a < 3; ++a) R.rp[a] = Q.pid[(size_t)a * Q.len + t];
        }
    }
    ph.n_rows = n;
    std::vector<LmPfSpan> spans;
    std::vector<int> first;
    lm_pf_chunks(lengths.data(), n_adm, chunk_rows, spans, first, ph.chunk);
    for (LmPfSpan& sp : spans) sp.seq = adm[sp.seq].slot;   // (lm_pf_chunks numbers the sequences of its list)
    std::vector<LmPfTile> t;
    for (size_t ci = 0; ci < ph.chunk.size(); ++ci) {
        ph.tile0.push_back(t.size());
        lm_pf_tiles(spans.data() + first[ci], first[ci + 1] - first[ci], heads, t);
    }
    ph.tile0.push_back(t.size());
    if (t.size() > tiles_cap) return false;
    std::copy(t.begin(), t.end(), tiles);
    ph.n_tiles = t.size();
    return true;
}

void lm_queue_phase_caps(const int32_t* lengths, int n_seq, int slots, int chunk_rows, int heads, size_t* rows_cap, size_t* tiles_cap) {
    std::vector<int32_t> top(lengths, lengths + n_seq);
    const size_t n = std::min<size_t>((size_t)slots, top.size());
    std::partial_sort(top.begin(), top.begin() + (std::ptrdiff_t)n, top.end(), std::greater<int32_t>());
    size_t rows = 0;
    for (size_t i = 0; i < n; ++i) rows += (size_t)(top[i] - 1);
    // a run of len query rows meets at most len / 64 + 2 tiles a head; a phase has at most slots + chunks runs
    const size_t runs = n + rows / (size_t)chunk_rows + 1;
    *rows_cap = rows;
    *tiles_cap = (size_t)heads * (rows / kLmPfQueries + 2 * runs);
}

}  // namespace k
}  // namespace oar
