"""qvis_misc.hip compiled for gfx950: exactly the instantiations of its three kernel templates, each without scratch, spills or LDS and at an
occupancy of at least 4 waves per SIMD (bandwidth kernels); every new export is declared in the public header; and the host routines that need no device
(qvis_plan.h: the argument checks, the window plan, the rotary tables) run clean as a stand-alone program under the address and undefined-behaviour sanitizers."""
import re
import shutil
import subprocess
from pathlib import Path

from oar_ocr_amd import api, build

ROOT = Path(__file__).resolve().parent.parent
CXX = shutil.which("g++") or shutil.which("c++") or build.HIPCC
PATTERNS = (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
            ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))
NEW_EXPORTS = ("oar_qvis_create", "oar_qvis_destroy", "oar_qvis_encode", "oar_qvis_cost", "oar_qvis_check", "oar_qvis_window_plan", "oar_k_qvis_rmsnorm", "oar_k_qvis_act",
               "oar_k_qvis_row_gather")


def test_qvis_misc_kernel_resources():
    assert "qvis_misc.hip" in build.SOURCES
    src = build.CSRC / "qvis_misc.hip"
    r = subprocess.run([build.HIPCC] + build.FLAGS + ["-c", str(src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in PATTERNS:
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    templates = {"qvis_rmsnorm_kernel": 1, "qvis_act_kernel": 6, "qvis_row_gather_kernel": 1}      # the activation: 3 forms x (plain, gated)
    assert sorted(re.findall(r"__global__[^\n]*void (\w+)\(", src.read_text())) == sorted(templates)
    for t, n in templates.items():
        assert sum(t in k for k in kernels) == n, (t, sorted(kernels))
    assert len(kernels) == sum(templates.values()), sorted(kernels)
    for k, v in kernels.items():
        print(f"{k}: {v['vgprs']} VGPRs, {v.get('agprs', 0)} AGPRs, occupancy {v['occupancy']} waves / SIMD")
        assert v["spill"] == 0 and v.get("sgpr_spill", 0) == 0 and v["scratch"] == 0 and v["lds"] == 0, (k, v)
        assert v["occupancy"] >= 4, (k, v)


def test_the_new_exports_are_declared_and_built():
    header = (ROOT / "include" / "oar_mi355x.h").read_text()
    L = api.lib()
    for sym in NEW_EXPORTS:
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in api.EXPORTS and hasattr(L, sym), sym
    launchers = (build.CSRC / "qvis.h").read_text()
    assert all(f"void {n}(" in launchers for n in ("qvis_rmsnorm", "qvis_act", "qvis_row_gather"))
    assert "qvis_" not in (build.CSRC / "kernels.h").read_text()            # the launchers stay out of the header every translation unit sees


DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "qvis_plan.h"
using namespace oar::qvis;
static int fails = 0;
static void check(bool ok, const char* what) { if (!ok) { std::printf("FAILED %s\n", what); ++fails; } }
static bool head_ok(int64_t heads, int64_t dh) { return heads >= 1 && dh >= 8 && dh <= 80 && dh % 8 == 0; }
int main() {
    const int32_t full[2] = {1, 5};
    oar_qvis_cfg c{};
    c.kind = OAR_QVIS_QWEN2_5; c.embed = 160; c.layers = 3; c.heads = 2; c.intermediate = 200; c.patch = 2; c.temporal_patch = 2; c.channels = 3; c.merge = 2;
    c.out_hidden = 48; c.act = OAR_QVIS_SILU; c.window_size = 16; c.n_fullatt = 1; c.fullatt_block_indexes = full; c.rope_theta = 10000.0f; c.max_tokens = 468; c.max_images = 3;
    check(check_cfg(c, head_ok).ok(), "a good configuration");
    { oar_qvis_cfg d = c; d.n_fullatt = 2; check(check_cfg(d, head_ok).code == OAR_INVALID_INPUT, "a full-attention index of 5 with 3 layers"); }
    { oar_qvis_cfg d = c; d.window_size = 18; check(check_cfg(d, head_ok).code == OAR_INVALID_INPUT, "window_size 18"); }
    { oar_qvis_cfg d = c; d.heads = 1; check(check_cfg(d, head_ok).code == OAR_UNSUPPORTED_OP, "head size 160"); }
    { oar_qvis_cfg d = c; d.act = 9; check(check_cfg(d, head_ok).code == OAR_UNSUPPORTED_OP, "act 9"); }
    { oar_qvis_cfg d = c; d.embed = 0; check(check_cfg(d, head_ok).code == OAR_INVALID_INPUT, "embed 0"); }
    const int32_t grids[6] = {14, 14, 16, 16, 4, 4};
    int64_t total = 0;
    check(check_grids(2, 3, 468, 3, grids, &total).ok() && total == 468, "the grids of case W5");
    check(check_grids(2, 3, 467, 3, grids, &total).code == OAR_INVALID_INPUT, "one patch above max_tokens");
    check(check_grids(2, 2, 468, 3, grids, &total).code == OAR_INVALID_INPUT, "three images with max_images 2");
    check(check_grids(4, 3, 468, 3, grids, &total).code == OAR_INVALID_INPUT, "14 is no multiple of merge 4");
    check(check_grids(2, 3, 468, 0, grids, &total).code == OAR_INVALID_INPUT, "no image");
    Plan p;
    check(window_plan(2, 2, 16, 3, grids, &p).ok(), "the plan of case W5");
    const int want[9] = {64, 48, 48, 36, 64, 64, 64, 64, 16};
    check(p.seg_len.size() == 9 && p.window_index.size() == 117 && p.reverse_index.size() == 117, "sizes of the plan");
    for (size_t i = 0; i < p.seg_len.size() && i < 9; ++i) check(p.seg_len[i] == want[i], "a window segment of case W5");
    for (size_t s = 0; s < p.window_index.size(); ++s) check(p.reverse_index[(size_t)p.window_index[s]] == (int32_t)s, "reverse_index inverts window_index");
    check(window_plan(2, 14, 100, 3, grids, &p).code == OAR_INVALID_INPUT, "window_size 100 at patch 14");
    check(window_plan(2, 2, 16, 0, nullptr, &p).ok() && p.window_index.empty() && p.seg_len.empty(), "no image: an empty plan");
    const int32_t odd[2] = {3, 4};
    check(window_plan(2, 2, 16, 1, odd, &p).code == OAR_INVALID_INPUT, "a grid that is no multiple of merge");
    const int32_t wide[4] = {2, 32768, 32768, 2};                          // long thin grids: one unit row / column, 16384 units each
    check(window_plan(2, 14, 112, 2, wide, &p).ok() && p.window_index.size() == 32768 && p.seg_len.size() == 8192, "long thin grids");
    check(window_plan(2, 2, 16, 3, grids, &p).ok(), "the plan again");
    for (int dh : {8, 40, 80}) {
        std::vector<float> cs, sn, cw, sw;
        const std::vector<float> inv = inv_freq_of(dh, 10000.0f);
        rotary_tables(3, grids, 2, dh, inv, nullptr, &cs, &sn);
        rotary_tables(3, grids, 2, dh, inv, p.window_index.data(), &cw, &sw);
        check(cs.size() == (size_t)468 * (dh / 2) && cw.size() == cs.size() && sn.size() == cs.size() && sw.size() == cs.size(), "table sizes");
        const size_t h2 = (size_t)dh / 2;
        bool same = true;
        for (size_t slot = 0; slot < 117 && same; ++slot)
            for (size_t i = 0; i < 4 * h2; ++i) same = same && cw[slot * 4 * h2 + i] == cs[(size_t)p.window_index[slot] * 4 * h2 + i] && sw[slot * 4 * h2 + i] == sn[(size_t)p.window_index[slot] * 4 * h2 + i];
        check(same, "the window-ordered tables are the caller-ordered ones permuted unit by unit");
        check(cs[0] == 1.0f && sn[0] == 0.0f, "position 0");
    }
    std::printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
"""


def test_the_host_routines_run_clean_under_the_sanitizers(tmp_path):
    (tmp_path / "driver.cc").write_text(DRIVER)
    exe = tmp_path / "driver_san"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{build.CSRC}", str(tmp_path / "driver.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("0 failures") and not out.stderr, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
