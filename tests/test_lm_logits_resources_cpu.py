"""Register / LDS guards of lm_logits.hip (hipcc cross-compiles without a GPU): the lm-head that also fills the step buffer and lm_select_kernel use
no scratch, spill nothing and leave room for at least two waves per SIMD; the head variant costs what lm_decode.hip's lm_head_kernel costs; lm_decode.hip, whose
rows body now lives in lm_rows_dev.h, still compiles to exactly the kernels tests/test_lm_resources_cpu.py counts; and the exported symbols, the header and the
regenerated sys crate agree on the three new entries."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from oar_ocr_amd import api, build

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "oar_ocr_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
NEW_ENTRIES = ("oar_lm_generate_ex", "oar_lm_logits_check", "oar_k_lm_select")

needs_hipcc = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")

_RES = {}


def _resources(src):
    if src in _RES:
        return _RES[src]
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        "--cuda-device-only", "-c", str(CSRC / src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("sgprs", r"TotalSGPRs: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    _RES[src] = out
    return out


@needs_hipcc
def test_lm_logits_kernels():
    res = {k: v for k, v in _resources("lm_logits.hip").items() if "_kernel" in k}
    heads = {k: v for k, v in res.items() if "lm_head_step_kernel" in k}
    select = [v for k, v in res.items() if "lm_select_kernel" in k]
    assert len(heads) == 10 and len(select) == 1 and len(res) == 11, sorted(res)     # 1 / 2 / 4 / 8 / 16 rows x {f32, bf16} weights
    for name, r in sorted(res.items()):
        print(name[-40:], "SGPRs", r["sgprs"], "VGPRs", r["vgprs"], "waves/SIMD", r["occupancy"], "static LDS", r["lds"])
        assert r["spill"] == 0 and r["scratch"] == 0 and r["occupancy"] >= 2, (name, r)
    assert select[0].get("sgpr_spill", 0) == 0, select[0]      # (the 8- and 16-row lm-heads park scalars in vector lanes, as lm_decode.hip's do: held to their twins below)
    # the select kernel's LDS: the reduction's few words statically, the ban bitmap dynamically (64 KiB at the largest vocabulary it takes: two workgroups a CU)
    prog = ('#include <cstdio>\n#include "lm_logits.h"\nint main() { using namespace oar::k; std::printf("%zu %zu %zu %zu %d %d %d\\n", lm_select_static_lds_bytes(), '
            'lm_select_lds_bytes(kLmSelectMaxVocab, 2), lm_select_lds_bytes(103424, 3), lm_select_lds_bytes(103424, 1), lm_select_words(10007), lm_select_ld(10007), '
            'lm_launches_per_step_select(18, false)); return 0; }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "lds.cc").write_text(prog)
        cxx = shutil.which("g++") or shutil.which("c++") or HIPCC
        subprocess.run([cxx, "-std=c++17", f"-I{CSRC}", str(Path(d) / "lds.cc"), "-o", str(Path(d) / "lds")], check=True, capture_output=True, timeout=300)
        static, big, paddle, off, words, ld, launches = [int(v) for v in subprocess.run([str(Path(d) / "lds")], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert select[0]["lds"] <= static and big == 64 * 1024 and paddle == 3232 * 4 and off == 0 and 2 * (big + static) <= LDS_PER_CU
    assert words == 313 and ld == 10008 and launches == 5 * 18 + 3      # V = 10007: a tail word of 23 bits, rows padded to 16 bytes


@needs_hipcc
def test_the_head_variant_costs_what_the_lm_head_costs_and_lm_decode_keeps_its_kernels():
    dec = _resources("lm_decode.hip")
    kinds = {"lm_rows_kernel": 10, "lm_qkv_rows_kernel": 10, "lm_gate_rows_kernel": 10, "lm_head_kernel": 10, "lm_attn_kernel": 4, "lm_combine_kernel": 1, "lm_embed_kernel": 1}
    for kind, count in kinds.items():
        assert len([k for k in dec if kind in k]) == count, (kind, sorted(dec))
    assert sum(kinds.values()) == len([k for k in dec if "_kernel" in k])
    assert not any("select" in k or "head_step" in k for k in dec)
    log = _resources("lm_logits.hip")
    for name, r in log.items():
        m = re.search(r"lm_head_step_kernelILi(\d+)E(\w)EE", name)
        if not m:
            continue
        twin = [v for k, v in dec.items() if re.search(rf"lm_head_kernelILi{m.group(1)}E{m.group(2)}EE", k)]
        assert len(twin) == 1
        # one more store per lane: the registers may differ by a few, the occupancy class and the LDS may not, and no more scalars are parked in vector lanes
        assert r["occupancy"] == twin[0]["occupancy"] and r["lds"] == twin[0]["lds"] and abs(r["vgprs"] - twin[0]["vgprs"]) <= 8, (name, r, twin[0])
        assert r.get("sgpr_spill", 0) <= twin[0].get("sgpr_spill", 0) + 8, (name, r, twin[0])


def test_no_fast_division_flag_reaches_the_build():
    assert "lm_logits.hip" in build.SOURCES
    assert "-fno-fast-math" in build.FLAGS and not any("fast-div" in f or "correctly-rounded" in f or f == "-ffast-math" for f in build.FLAGS)


def test_exports_header_and_sys_crate_agree_on_the_new_entries():
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import gen_rust_sys
    finally:
        sys.path.pop(0)
    h = gen_rust_sys.parse_header()
    funcs = {name: params for name, _, params in h["funcs"]}
    assert [len(funcs[n]) for n in NEW_ENTRIES] == [3, 3, 10]
    fields = dict(h["structs"])["oar_lm_logits_cfg"]
    assert [f for f, _, _ in fields] == ["repetition_penalty", "no_repeat_ngram_size", "history_lengths", "history_ids"]
    from oar_ocr_amd import vl
    assert [f[0] for f in vl.LmLogitsCfg._fields_] == [f for f, _, _ in fields]
    import ctypes as C
    assert C.sizeof(vl.LmLogitsCfg) == 24
    crate = (ROOT / "rust" / "oar-mi355x-sys" / "src" / "lib.rs").read_text()
    assert crate == gen_rust_sys.generate(h)
    for n in NEW_ENTRIES:
        assert f"pub fn {n}(" in crate and n in api.EXPORTS
    assert "pub struct oar_lm_logits_cfg" in crate and "pub history_ids: *const *const i32," in crate
    L = api.lib()
    for n in NEW_ENTRIES:
        assert getattr(L, n) is not None
