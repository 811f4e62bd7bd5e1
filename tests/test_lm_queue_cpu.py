"""The scheduler of queued generation (csrc/lm_queue.h, lm_queue.cc) without a GPU: the scheduler is compiled with a driver written here that plays the
device (the `done` flags, the lagged copies, the slots' occupants), queues with given end steps are simulated in both prefill modes and the schedule's invariants
asserted; the same driver runs once more as a stand-alone program under AddressSanitizer and UBSan; the argument checks that need no device, and the exports."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oar_ocr_amd import api, vl
from oar_ocr_amd.synth import lm_queue_cases as Q

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "oar_ocr_amd" / "csrc"
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# The driver: the host loop of oar_lm_generate_queue with the device replaced by arrays.  Input (a file): n_seq slots max_new gemm chunk_rows heads, the prompt
# lengths, and per sequence the token index at which it emits eos (-1: never).  Output: one JSON object with the figures and every violated invariant.
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "lm_queue.h"
using namespace oar::k;
static std::vector<std::string> bad;
static void check(bool ok, const std::string& what, long long a = 0, long long b = 0) { if (!ok && bad.size() < 20) bad.push_back(what + " " + std::to_string(a) + " " + std::to_string(b)); }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n_seq, slots, max_new, gemm, chunk_rows, heads;
    if (std::fscanf(f, "%d %d %d %d %d %d", &n_seq, &slots, &max_new, &gemm, &chunk_rows, &heads) != 6) return 2;
    std::vector<int32_t> len((size_t)n_seq), end((size_t)n_seq);
    for (int& v : len) if (std::fscanf(f, "%d", &v) != 1) return 2;
    for (int& v : end) if (std::fscanf(f, "%d", &v) != 1) return 2;
    std::fclose(f);
    std::vector<LmQueueSeq> seqs((size_t)n_seq);
    int total = 0;
    for (int q = 0; q < n_seq; ++q) { seqs[(size_t)q] = LmQueueSeq{len[(size_t)q], total, len[(size_t)q], nullptr}; total += len[(size_t)q]; }
    size_t rows_cap = 0, tiles_cap = 0;
    lm_queue_phase_caps(len.data(), n_seq, slots, chunk_rows, heads, &rows_cap, &tiles_cap);
    std::vector<LmPfRow> pf_rows(rows_cap + 1);
    std::vector<LmPfTile> pf_tiles(tiles_cap + 1);
    // the device
    int32_t dev_done[kLmRows] = {};
    int dev_occ[kLmRows];
    for (int& v : dev_occ) v = -1;
    struct Copy { int32_t done[kLmRows]; long long index; };
    std::vector<Copy> pin_state((size_t)kLmQueueRing, Copy{{}, -1});
    std::vector<long long> stage_step((size_t)kLmQueueRing, -1), phase_step((size_t)kLmQueueRing, -1);
    std::vector<LmQueueStage> pin_stage((size_t)kLmQueueRing);
    // per sequence
    std::vector<int> next_pos((size_t)n_seq, 0), tokens((size_t)n_seq, 0), dead((size_t)n_seq, 0), retired((size_t)n_seq, 0), admitted((size_t)n_seq, 0);
    std::vector<long long> last_decode((size_t)n_seq, -1);
    LmQueue S(seqs.data(), n_seq, slots, max_new, gemm != 0, total);
    std::vector<LmQueueAdmit> admits;
    LmQueuePhase ph;
    Copy seen_state{{}, -1};
    long long seen = -1, phases = 0, phase_chunks = 0, turnovers = 0, max_rows = 0, next_admit = 0;
    const long long limit = 4LL * ((long long)total + (long long)n_seq * (max_new + kLmQueueRing)) + 64;   // the call ends
    for (;;) {
        const long long i = S.step();
        if (i > limit) { check(false, "the call does not end"); break; }
        const size_t e = (size_t)(i % kLmQueueRing);
        const long long cpy = lm_queue_copy_for(i);
        if (cpy > seen) {
            check(pin_state[(size_t)(cpy % kLmQueueRing)].index == cpy, "a state copy was overwritten before it was read", cpy, pin_state[(size_t)(cpy % kLmQueueRing)].index);
            check(lm_queue_copy_step(cpy) < i && lm_queue_copy_step(cpy) <= i - kLmQueueLookahead, "a copy from too late a step", cpy, i);
            seen_state = pin_state[(size_t)(cpy % kLmQueueRing)];
            seen = cpy;
        }
        const long long proven = seen >= 0 ? lm_queue_copy_step(seen) : -1;   // every copy enqueued up to this step has finished
        check(stage_step[e] <= proven, "a stage entry rewritten before its event", stage_step[e], proven);
        int n_turn = 0, max_pos = 0;
        const bool more = S.next(seen >= 0 ? seen_state.done : nullptr, proven, pin_stage[e], n_turn, max_pos, admits);
        if (!more && n_turn == 0) break;
        stage_step[e] = i;
        const LmQueueStage& st = pin_stage[e];
        check(n_turn >= 0 && n_turn <= slots, "turnover count", n_turn);
        bool turned[kLmRows] = {};
        for (int t = 0; t < n_turn; ++t) {
            const LmQueueTurn& T = st.turn[t];
            check(T.slot >= 0 && T.slot < slots && !turned[T.slot], "turnover slot", T.slot);
            if (T.slot < 0 || T.slot >= slots) continue;
            turned[T.slot] = true;
            check(dev_occ[T.slot] == T.out_seq, "a turnover retires another sequence than the slot holds", dev_occ[T.slot], T.out_seq);
            if (T.out_seq >= 0) {
                check(T.produced == tokens[(size_t)T.out_seq] && T.produced >= 1 && T.produced <= max_new, "produced", T.produced, tokens[(size_t)T.out_seq]);
                check(!retired[(size_t)T.out_seq], "retired twice", T.out_seq);
                check(T.produced == max_new || (end[(size_t)T.out_seq] >= 0 && end[(size_t)T.out_seq] < T.produced), "retired before its end", T.out_seq);
                retired[(size_t)T.out_seq] = 1;
            }
            if (T.in_seq >= 0) {
                check(T.in_seq == next_admit, "admission out of request order", T.in_seq, next_admit);
                ++next_admit;
                check(T.in_seq < n_seq && !admitted[(size_t)T.in_seq], "admitted twice", T.in_seq);
                admitted[(size_t)T.in_seq] = 1;
            }
            dev_occ[T.slot] = T.in_seq;
            dev_done[T.slot] = 0;
            ++turnovers;
        }
        if (!more) break;
        if (!admits.empty()) {
            check(gemm != 0, "a GEMM phase in rows mode");
            check(phase_step[e] <= proven, "a phase entry rewritten before its event", phase_step[e], proven);
            phase_step[e] = i;
            const bool fit = lm_queue_pack(seqs.data(), admits.data(), (int)admits.size(), chunk_rows, heads, pf_rows.data(), rows_cap, pf_tiles.data(), tiles_cap, ph);
            check(fit, "a phase outgrew its tables", (long long)rows_cap, (long long)tiles_cap);
            if (fit) {
                size_t sum = 0;
                for (int c : ph.chunk) { sum += (size_t)c; check(c >= 1 && c <= chunk_rows, "chunk size", c); }
                check(sum == ph.n_rows && ph.tile0.size() == ph.chunk.size() + 1 && ph.tile0.back() == ph.n_tiles, "phase tables");
                for (size_t r = 0; r < ph.n_rows; ++r) {
                    const LmPfRow& R = pf_rows[r];
                    const int q = R.seq >= 0 && R.seq < slots ? dev_occ[R.seq] : -1;
                    check(q >= 0, "a phase row of an empty slot", R.seq);
                    if (q < 0) continue;
                    check(R.pos == next_pos[(size_t)q] && R.pos < len[(size_t)q] - 1 && R.xrow == seqs[(size_t)q].xrow0 + R.pos, "a phase row out of order", q, R.pos);
                    ++next_pos[(size_t)q];
                }
                for (size_t t = 0; t < ph.n_tiles; ++t) check(pf_tiles[t].seq >= 0 && pf_tiles[t].seq < slots && pf_tiles[t].head >= 0 && pf_tiles[t].head < heads, "tile");
                phase_chunks += (long long)ph.chunk.size();
            }
            ++phases;
        }
        const LmStep& step = st.step;
        check(step.nrows >= 1 && step.nrows <= kLmRows && step.nhead >= 0 && step.nhead <= step.nrows, "rows of a step", step.nrows, step.nhead);
        max_rows = step.nrows > max_rows ? step.nrows : max_rows;
        int heads_seen = 0, mp = 0;
        for (int r = 0; r < step.nrows && r < kLmRows; ++r) {
            const LmRow& R = step.rows[r];
            const int q = R.seq >= 0 && R.seq < slots ? dev_occ[R.seq] : -1;
            check(q >= 0, "a row of an empty slot", R.seq, i);
            if (q < 0) continue;
            mp = R.pos > mp ? R.pos : mp;
            check(!retired[(size_t)q], "a row of a retired sequence", q, i);
            check(R.pos == next_pos[(size_t)q], "a row out of order", q, R.pos);
            ++next_pos[(size_t)q];
            if (R.pos < len[(size_t)q] - 1) { check(R.gen == -1 && R.xrow == seqs[(size_t)q].xrow0 + R.pos, "a prompt row", q, R.pos); continue; }
            check(R.gen == tokens[(size_t)q] && R.gen == R.pos - (len[(size_t)q] - 1) && R.gen < max_new, "token index", q, R.gen);
            check(R.gen == 0 ? R.xrow == seqs[(size_t)q].xrow0 + R.pos : R.xrow == total + R.seq, "arena row", q, R.xrow);
            check(R.rp[0] == R.pos, "rotary position", q, R.rp[0]);
            bool listed = false;
            for (int h = 0; h < step.nhead; ++h) listed = listed || step.head[h] == r;
            check(listed, "a token row missing from head[]", q, r);
            ++heads_seen;
            if (R.gen > 0) check(last_decode[(size_t)q] == i - 1, "decode rows not in consecutive steps", q, i);
            last_decode[(size_t)q] = i;
            if (end[(size_t)q] >= 0 && R.gen > end[(size_t)q]) ++dead[(size_t)q];
            if (end[(size_t)q] == R.gen) dev_done[R.seq] = 1;
            ++tokens[(size_t)q];
        }
        check(heads_seen == step.nhead && mp == max_pos, "head count or max_pos", heads_seen, step.nhead);
        if ((i + 1) % kLmQueueStride == 0) {
            const long long c = (i + 1) / kLmQueueStride - 1;
            Copy& dst = pin_state[(size_t)(c % kLmQueueRing)];
            for (int s = 0; s < kLmRows; ++s) dst.done[s] = dev_done[s];
            dst.index = c;
        }
    }
    long long rows = 0, dead_rows = 0, max_dead = 0;
    for (int q = 0; q < n_seq; ++q) {
        check(retired[(size_t)q] && admitted[(size_t)q], "a sequence never retired", q);
        check(next_pos[(size_t)q] == len[(size_t)q] - 1 + tokens[(size_t)q], "rows of a sequence", q);
        check(S.produced()[(size_t)q] == tokens[(size_t)q], "produced()", q);
        const int want = end[(size_t)q] >= 0 && end[(size_t)q] < max_new ? end[(size_t)q] + 1 : max_new;
        check(tokens[(size_t)q] >= want && tokens[(size_t)q] - want == dead[(size_t)q], "tokens of a sequence", q, tokens[(size_t)q]);
        check(dead[(size_t)q] <= kLmQueueLookahead + kLmQueueStride, "dead rows above the bound", q, dead[(size_t)q]);
        rows += next_pos[(size_t)q]; dead_rows += dead[(size_t)q]; max_dead = dead[(size_t)q] > max_dead ? dead[(size_t)q] : max_dead;
    }
    for (int s = 0; s < slots; ++s) check(dev_occ[s] == -1, "a slot still held at the end", s);
    const long long step_rows = S.rows();
    check(gemm ? step_rows <= rows : step_rows == rows, "rows()", step_rows, rows);
    std::printf("{\"steps\": %lld, \"rows\": %lld, \"step_rows\": %lld, \"dead_rows\": %lld, \"max_dead\": %lld, \"admissions\": %lld, \"phases\": %lld, \"phase_chunks\": %lld, "
                "\"turnovers\": %lld, \"max_rows\": %lld, \"min_slot_admissions\": %lld, \"min_slot_turnovers\": %lld, \"bad\": [", (long long)S.step(), rows, step_rows, dead_rows, max_dead, (long long)S.admissions(), phases,
                phase_chunks, turnovers, max_rows, (long long)S.min_slot_admissions(), (long long)S.min_slot_turnovers());
    for (size_t b = 0; b < bad.size(); ++b) std::printf("%s\"%s\"", b ? ", " : "", bad[b].c_str());
    std::printf("]}\n");
    return bad.empty() ? 0 : 1;
}
"""


def _queues():
    """name -> (slots, max_new, lengths, ends): ends[i] is the token index at which sequence i emits eos, -1 never."""
    rng = np.random.default_rng(44)
    w = {}
    w["one"] = (16, 12, [5], [-1])
    w["one_slot_one_seq_eos_first"] = (1, 12, [1], [0])
    w["17_on_16"] = (16, 12, list(rng.integers(1, 40, 17)), list(rng.integers(-1, 12, 17)))
    w["200_on_16"] = (16, 12, list(rng.integers(1, 40, 200)), list(rng.integers(-1, 14, 200)))
    w["200_on_3"] = (3, 9, list(rng.integers(1, 20, 200)), list(rng.integers(-1, 9, 200)))
    w["40_on_1"] = (1, 12, list(rng.integers(1, 40, 40)), list(rng.integers(-1, 12, 40)))
    w["prompts_of_1"] = (16, 12, [1] * 50, list(rng.integers(-1, 12, 50)))
    w["max_new_1"] = (16, 1, list(rng.integers(1, 40, 40)), list(rng.integers(-1, 1, 40)))
    w["max_new_1_on_3"] = (3, 1, [1] * 10, [-1] * 10)
    w["no_eos"] = (16, 12, list(rng.integers(1, 40, 20)), [-1] * 20)
    w["all_eos_at_once"] = (16, 12, [3] * 40, [0] * 40)
    w["long_prompts"] = (16, 6, list(rng.integers(100, 300, 24)), list(rng.integers(-1, 6, 24)))
    ref = Q.workload()
    w["workload_16"] = (16, Q.MAX_NEW, list(Q.LENGTHS), [int(c) - 1 if c < Q.MAX_NEW else -1 for c in ref["counts"]])
    w["workload_4"] = (4,) + w["workload_16"][1:]
    return w


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("lm_queue")
    (d / "driver.cc").write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([CXX, "-std=c++17", "-O1", f"-I{CSRC}", str(d / "driver.cc"), str(CSRC / "lm_queue.cc"), "-o", str(exe)], check=True, capture_output=True, timeout=600)
    return d, exe


def _run(exe, d, name, slots, max_new, lengths, ends, gemm, chunk_rows=2048, heads=4):
    spec = d / f"{name}_{gemm}_{chunk_rows}.txt"
    spec.write_text(f"{len(lengths)} {slots} {max_new} {gemm} {chunk_rows} {heads}\n" + " ".join(str(int(v)) for v in lengths) + "\n" + " ".join(str(int(v)) for v in ends) + "\n")
    r = subprocess.run([str(exe), str(spec)], capture_output=True, text=True, timeout=120)
    assert r.returncode in (0, 1) and r.stdout, (name, r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout)


def _groups_steps(lengths, ends, max_new, gemm):
    """Steps of the groups-of-16 schedule that stops at eos, without its lag: per group the prefill steps and the decode steps up to its longest sequence's end."""
    total = 0
    for i in range(0, len(lengths), 16):
        ln, en = lengths[i:i + 16], ends[i:i + 16]
        prefill = 1 if gemm else -(-sum(int(v) for v in ln) // 16)
        total += prefill + max((int(e) + 1 if 0 <= e < max_new else max_new) for e in en) - 1
    return total


@pytest.mark.parametrize("gemm", [0, 1], ids=["rows", "gemm"])
def test_simulated_queues_keep_the_schedules_invariants(driver, gemm):
    d, exe = driver
    c = Q.queue_constants()
    assert c["ring"] >= c["lookahead"] + c["stride"] and c["stride"] >= 1 and c["lookahead"] >= 1
    for name, (slots, max_new, lengths, ends) in _queues().items():
        for chunk in (2048, 64):
            g = _run(exe, d, name, slots, max_new, lengths, ends, gemm, chunk)
            groups = _groups_steps(lengths, ends, max_new, gemm)
            print(f"{name} {'gemm' if gemm else 'rows'} chunk {chunk}: {len(lengths)} sequences on {slots} slots: {g['steps']} steps ({groups} in groups of 16), {g['rows']} rows, "
                  f"{g['dead_rows']} dead (most {g['max_dead']}), {g['phases']} phases of {g['phase_chunks']} chunks, {g['turnovers']} turnovers")
            assert g["bad"] == [], (name, g["bad"])
            assert g["admissions"] == len(lengths) and g["max_rows"] <= 16 and g["max_dead"] <= c["lookahead"] + c["stride"]
            if all(e < 0 for e in ends):
                assert g["dead_rows"] == 0
            if gemm:
                assert g["step_rows"] == g["rows"] - sum(int(t) - 1 for t in lengths)
                # everything admitted at one point shares a phase: the first fill of the slots is one phase, not one per sequence
                assert g["phases"] <= g["admissions"] - min(slots, len(lengths)) + 1 or all(t == 1 for t in lengths)
                assert (g["phases"] == 0) == all(t == 1 for t in lengths)
            else:
                assert g["phases"] == 0 and g["step_rows"] == g["rows"]
    # the workload of the GPU test: what it asserts about the slots' use holds in the simulation (every slot holds two sequences or more, the rows prefill on 16 slots
    # aside, where the last slot starts at step 14 and the queue is empty before it retires)
    for name in ("workload_16", "workload_4"):
        slots, max_new, lengths, ends = _queues()[name]
        g = _run(exe, d, name, slots, max_new, lengths, ends, gemm)
        assert g["min_slot_turnovers"] >= 2 and g["min_slot_admissions"] >= (1 if (slots == 16 and not gemm) else 2), g


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, driver):
    """The same driver and scheduler as a stand-alone program with -fsanitize=address,undefined, on the two largest queues in both modes."""
    d, _ = driver
    exe = tmp_path / "driver_san"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(d / "driver.cc"), str(CSRC / "lm_queue.cc"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    qs = _queues()
    for name in ("200_on_16", "200_on_3", "long_prompts", "max_new_1"):
        for gemm in (0, 1):
            slots, max_new, lengths, ends = qs[name]
            g = _run(exe, tmp_path, name, slots, max_new, lengths, ends, gemm, 64)
            assert g["bad"] == [], (name, g["bad"])


def _request(n_seq, lengths, max_new, keep):
    ids = [np.zeros(max(int(t), 1), np.int32) for t in lengths]
    ptrs = (C.c_void_p * max(len(ids), 1))(*[a.ctypes.data for a in ids])
    ln = np.asarray(lengths, np.int32)
    tokens, counts = np.zeros((max(len(ids), 1), max(max_new, 1)), np.int32), np.zeros(max(len(ids), 1), np.int32)
    keep += [ids, ptrs, ln, tokens, counts]
    req = vl.LmRequest()
    req.n_seq = n_seq
    req.lengths = ln.ctypes.data_as(C.POINTER(C.c_int32))
    req.input_ids = C.cast(ptrs, C.POINTER(C.c_void_p))
    req.max_new_tokens = max_new
    req.eos_token_id = -1
    req.tokens, req.counts = tokens.ctypes.data, counts.ctypes.data
    return req


def _cfg(**kw):
    ref_case = Q.R.CASES["A"]
    d = dict(hidden_size=ref_case.D, num_hidden_layers=ref_case.L, num_attention_heads=ref_case.heads, num_key_value_heads=ref_case.kv_heads, head_dim=ref_case.head_dim,
             intermediate_size=ref_case.F, vocab_size=ref_case.vocab, mrope_section=list(ref_case.mrope_section), max_positions=64, max_sequences=16)
    d.update(kw)
    return vl.CausalLMConfig(**d).to_c()


def test_argument_checks_need_no_device():
    L = vl._lib()
    keep = []
    cfg = _cfg()
    ok = _request(20, [3] * 20, 8, keep)
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(ok), 0) == api.OAR_OK
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(ok), 16) == api.OAR_OK and L.oar_lm_queue_check(C.byref(cfg), C.byref(ok), 1) == api.OAR_OK
    assert L.oar_lm_queue_check(C.byref(cfg), None, 0) == api.OAR_INVALID_INPUT and L.oar_lm_queue_check(None, C.byref(ok), 0) == api.OAR_INVALID_INPUT
    assert L.oar_lm_generate_queue(None, C.byref(ok), 0) == api.OAR_INVALID_INPUT
    assert L.oar_lm_queue_stats(None, None, 0) == api.OAR_INVALID_INPUT
    for slots in (-1, 17, 1 << 20):
        assert L.oar_lm_queue_check(C.byref(cfg), C.byref(ok), slots) == api.OAR_INVALID_INPUT, slots
    small = _cfg(max_sequences=4)
    assert L.oar_lm_queue_check(C.byref(small), C.byref(ok), 4) == api.OAR_OK and L.oar_lm_queue_check(C.byref(small), C.byref(ok), 5) == api.OAR_INVALID_INPUT
    for n in (0, -1, 65536):
        bad = _request(20, [3] * 20, 8, keep)
        bad.n_seq = n
        assert L.oar_lm_queue_check(C.byref(cfg), C.byref(bad), 0) == api.OAR_INVALID_INPUT, n
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(_request(3, [3, 57, 3], 8, keep)), 0) == api.OAR_INVALID_INPUT       # 57 + 8 > 64 positions
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(_request(3, [3, 56, 3], 8, keep)), 0) == api.OAR_OK
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(_request(3, [3, 0, 3], 8, keep)), 0) == api.OAR_INVALID_INPUT
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(_request(3, [3, 3, 3], 0, keep)), 0) == api.OAR_INVALID_INPUT
    many = _request(65535, [1] * 65535, 2, keep)
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(many), 0) == api.OAR_OK
    nul = _request(3, [3, 3, 3], 8, keep)
    nul.tokens = None
    assert L.oar_lm_queue_check(C.byref(cfg), C.byref(nul), 0) == api.OAR_INVALID_INPUT


def test_the_new_entries_are_exported():
    L = vl._lib()
    for name in ("oar_lm_generate_queue", "oar_lm_queue_check", "oar_lm_queue_stats"):
        assert getattr(L, name) is not None
    header = (ROOT / "include" / "oar_mi355x.h").read_text()
    for name in ("oar_lm_generate_queue(", "oar_lm_queue_check(", "oar_lm_queue_stats("):
        assert name in header
    assert vl.QUEUE_STATS[:5] == ("steps", "rows", "dead_rows", "admissions", "gemm_phases")
