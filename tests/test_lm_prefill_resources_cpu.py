"""Register / LDS guards of lm_prefill_gemm.hip and lm_prefill_attn.hip (hipcc cross-compiles without a GPU): no kernel touches scratch or spills, each
leaves room for at least two waves per SIMD, the LDS is what csrc/lm_prefill.h computes and lets two workgroups share a CU's 160 KiB.  And the kernels that share
flash_f32_dev.h with the new attention kernel compile to the registers DESIGN 4.41 records."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from oar_ocr_amd.synth import lm_prefill_cases as P

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


def _clean(name, r):
    assert r["spill"] == 0 and r.get("sgpr_spill", 0) == 0 and r["scratch"] == 0, (name, r)


def test_lm_gemm_kernels():
    """four epilogues x {f32, bf16} weights; all LDS static: what lm_gemm_lds_bytes says"""
    res = _resources("lm_prefill_gemm.hip")
    assert len(res) == 8 and all("lm_gemm_kernel" in k for k in res), sorted(res)
    lds = P.prefill_arithmetic((2,))["gemm_lds"]
    for name, r in res.items():
        mode, wt = re.search(r"lm_gemm_kernelILi(\d)E([tf])E", name).groups()
        print(f"lm_gemm_kernel<{mode}, {'bf16' if wt == 't' else 'f32'}>: {r['vgprs']} VGPRs, {r.get('agprs', 0)} AGPRs, {r['occupancy']} waves / SIMD, {r['lds']} B LDS")
        _clean(name, r)
        assert r["occupancy"] >= 2 and r["lds"] == lds and 2 * lds <= LDS_PER_CU, (name, r, lds)


def test_lm_prefill_attn_kernels():
    """DH16 = 1 .. 8: no static LDS (all dynamic, lm_pf_attn_lds_bytes), two 256-thread workgroups per CU by registers and by LDS at every head size"""
    res = _resources("lm_prefill_attn.hip")
    assert sorted(int(re.search(r"lm_prefill_attn_kernelILi(\d)EE", k).group(1)) for k in res) == [1, 2, 3, 4, 5, 6, 7, 8], sorted(res)
    lds = P.prefill_arithmetic((2,))["attn_lds"]
    for name, r in sorted(res.items()):
        dh16 = int(re.search(r"lm_prefill_attn_kernelILi(\d)EE", name).group(1))
        print(f"lm_prefill_attn_kernel<{dh16}>: {r['vgprs']} VGPRs, {r.get('agprs', 0)} AGPRs, {r['occupancy']} waves / SIMD, dynamic LDS {lds[16 * dh16]} B")
        _clean(name, r)
        assert r["lds"] == 0 and r["occupancy"] >= 2 and r["vgprs"] + r.get("agprs", 0) <= 256, (name, r)
        assert 2 * lds[16 * dh16] <= LDS_PER_CU
    assert lds[128] == 67584


def test_the_older_flash_kernels_keep_their_registers():
    """flash_f32_dev.h is shared: mha_attention_kernel<1..4> 52 / 69 / 90 / 106 VGPRs, relpos_attention_kernel<1..4> 59 / 77 / 102 / 119, vis_attention_kernel<1..5>
    72 + 8 / 108 + 8 / 144 + 12 / 183 + 16 / 228 + 20 VGPRs + AGPRs, none with scratch"""
    want = {"mha_attention.hip": ("mha_attention_kernel", {1: (52, None), 2: (69, None), 3: (90, None), 4: (106, None)}),
            "relpos_attention.hip": ("relpos_attention_kernel", {1: (59, None), 2: (77, None), 3: (102, None), 4: (119, None)}),
            "vis_attention.hip": ("vis_attention_kernel", {1: (72, 8), 2: (108, 8), 3: (144, 12), 4: (183, 16), 5: (228, 20)})}
    for src, (kernel, table) in want.items():
        res = {k: v for k, v in _resources(src).items() if kernel in k}
        got = {}
        for name, r in res.items():
            _clean(name, r)
            got[int(re.search(kernel + r"ILi(\d)E", name).group(1))] = (r["vgprs"], r.get("agprs", 0))
        print(src, got)
        assert set(got) == set(table), (src, got)
        for dh16, (v, a) in table.items():
            assert got[dh16][0] == v and (a is None or got[dh16][1] == a), (src, dh16, got[dh16], (v, a))
