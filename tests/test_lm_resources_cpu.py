"""Register / LDS guards of lm_decode.hip (hipcc cross-compiles without a GPU): no kernel of the file touches scratch or spills, and the LDS a launch asks for
lets two workgroups share a CU (160 KiB), so one's staging overlaps the other's streaming."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "oar_ocr_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024


def _resources(src):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        "--cuda-device-only", "-c", str(CSRC / src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_lm_kernels_use_no_scratch_and_fit_two_workgroups_per_cu(tmp_path):
    res = _resources("lm_decode.hip")
    kinds = {"lm_rows_kernel": 10, "lm_qkv_rows_kernel": 10, "lm_gate_rows_kernel": 10, "lm_head_kernel": 10, "lm_attn_kernel": 4, "lm_combine_kernel": 1, "lm_embed_kernel": 1}
    for kind, count in kinds.items():      # rows kernels: 1 / 2 / 4 / 8 / 16 rows x {f32, bf16} weights; attention: 1 / 2 / 4 / 8 query heads per workgroup
        ks = {k: v for k, v in res.items() if kind in k}
        assert len(ks) == count, (kind, sorted(ks))
        for name, r in ks.items():
            assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
            print(kind, name[-24:], "VGPRs", r["vgprs"], "waves/SIMD", r["occupancy"], "static LDS", r["lds"])
    assert sum(kinds.values()) == len([k for k in res if "_kernel" in k])
    # two waves per SIMD: two 256-thread workgroups of a rows kernel per CU, one 512-thread workgroup of the attention kernel
    for name, r in res.items():
        assert r["occupancy"] >= 2, (name, r)
    # the LDS the host asks for, from the host-compiled header
    prog = tmp_path / "lds.cc"
    prog.write_text('#include <cstdio>\n#include "lm_decode.h"\nint main() { using namespace oar::k; std::printf("%zu %zu %zu %zu %zu\\n", lm_rows_lds_bytes(16, 1024), '
                    'lm_rows_lds_bytes(16, 3072), lm_rows_lds_bytes(3, 40), lm_rows_static_lds_bytes(), lm_attn_lds_bytes()); return 0; }\n')
    cxx = shutil.which("g++") or shutil.which("c++") or HIPCC
    exe = tmp_path / "lds"
    subprocess.run([cxx, "-std=c++17", f"-I{CSRC}", str(prog), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    d1024, d3072, small, static, attn = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert d1024 == d3072 == 16 * 1024 * 4 and small == 4 * 40 * 4          # one 1024-column chunk of 16 rows at the most; 3 rows take the 4-row instantiation
    rows_static = max(r["lds"] for k, r in res.items() if "rows_kernel" in k or "lm_head_kernel" in k)
    attn_static = max(r["lds"] for k, r in res.items() if "lm_attn_kernel" in k)
    assert rows_static <= static and attn_static <= attn, (rows_static, static, attn_static, attn)
    assert 2 * (d1024 + static) <= LDS_PER_CU and 2 * attn <= LDS_PER_CU
