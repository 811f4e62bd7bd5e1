"""Register / LDS guards of lm_decode_split.hip (hipcc cross-compiles without a GPU): no kernel touches scratch or spills, each leaves room for at least
two waves per SIMD, the LDS is what csrc/lm_decode.h computes (all dynamic) and lets two workgroups share a CU's 160 KiB.  And lm_decode.hip, whose host half now
chooses between the two attentions, still compiles to exactly the kernels tests/test_lm_resources_cpu.py counts."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from oar_ocr_amd.synth import lm_split_cases as S

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "oar_ocr_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024

pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")


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
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def test_lm_split_kernels():
    """lm_attn_split_kernel<1 | 2 | 4 | 8> and lm_attn_merge_kernel: no static LDS, the dynamic LDS of lm_split_lds_bytes, two 256-thread workgroups per CU at the least"""
    res = {k: v for k, v in _resources("lm_decode_split.hip").items() if "_kernel" in k}
    split = {int(re.search(r"lm_attn_split_kernelILi(\d)EE", k).group(1)): v for k, v in res.items() if "lm_attn_split_kernel" in k}
    merge = [v for k, v in res.items() if "lm_attn_merge_kernel" in k]
    assert sorted(split) == [1, 2, 4, 8] and len(merge) == 1 and len(res) == 5, sorted(res)
    lds = S.split_arithmetic()["lds"]
    for gt, r in sorted(split.items()):
        print(f"lm_attn_split_kernel<{gt}>: {r['vgprs']} VGPRs, {r.get('agprs', 0)} AGPRs, {r['occupancy']} waves / SIMD, dynamic LDS {lds[(8, gt)]} .. {lds[(128, gt)]} B")
        assert r["spill"] == 0 and r.get("sgpr_spill", 0) == 0 and r["scratch"] == 0, (gt, r)
        assert r["lds"] == 0 and r["occupancy"] >= 2, (gt, r)
        assert all(2 * lds[(dh, gt)] <= LDS_PER_CU for dh in range(8, 129, 4))
    r = merge[0]
    print(f"lm_attn_merge_kernel: {r['vgprs']} VGPRs, {r['occupancy']} waves / SIMD, LDS {r['lds']} B")
    assert r["spill"] == 0 and r.get("sgpr_spill", 0) == 0 and r["scratch"] == 0 and r["lds"] == 0 and r["occupancy"] >= 2, r
    assert lds[(128, 8)] == 72704


def test_lm_decode_keeps_its_kernels():
    res = _resources("lm_decode.hip")
    kinds = {"lm_rows_kernel": 10, "lm_qkv_rows_kernel": 10, "lm_gate_rows_kernel": 10, "lm_head_kernel": 10, "lm_attn_kernel": 4, "lm_combine_kernel": 1, "lm_embed_kernel": 1}
    for kind, count in kinds.items():
        assert len([k for k in res if kind in k]) == count, (kind, sorted(res))
    assert sum(kinds.values()) == len([k for k in res if "_kernel" in k])
    assert not any("split" in k or "merge" in k for k in res)
