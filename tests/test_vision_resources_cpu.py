"""vis_attention.hip and vis_misc.hip compiled for gfx950: every vis_* kernel without scratch, spills or static LDS.  vis_attention.hip: one kernel template, the five instantiations its dispatch names, no scratch, no spills, no static
LDS; the dynamic LDS from the host-compiled k::vis_attention_lds_bytes lets at least two workgroups share a CU's 160 KB at every DH16, and the VGPR count
leaves room for two workgroups' waves on a SIMD (512 registers, one wave per SIMD and workgroup).  VGPRs and occupancy are printed."""
import re
import subprocess

from oar_ocr_amd import build

PATTERNS = (("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
            ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"))


def _resources(src):
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
    return kernels


def test_vis_attention_kernel_resources(tmp_path):
    src = build.CSRC / "vis_attention.hip"
    assert "vis_attention.hip" in build.SOURCES
    kernels = _resources(src)
    named = sorted(int(n) for n in re.findall(r"vis_attention_kernel<(\d), k\w+>", src.read_text()))
    assert named == [1, 2, 3, 4, 5]                                            # what the dispatch names ...
    assert len(kernels) == 5 and all("vis_attention_kernel" in k for k in kernels), sorted(kernels)   # ... is what exists
    got = {}
    for k, v in kernels.items():
        dh16, ld = (int(x) for x in re.search(r"vis_attention_kernelILi(\d)ELi(\d+)EE", k).groups())
        got[dh16] = ld
        print(f"vis_attention_kernel<{dh16}, {ld}>: {v['vgprs']} VGPRs, {v.get('agprs', 0)} AGPRs, occupancy {v['occupancy']} waves / SIMD")
        assert v["spill"] == 0 and v.get("sgpr_spill", 0) == 0 and v["scratch"] == 0 and v["lds"] == 0, (k, v)
        assert v["occupancy"] >= 2 and v["vgprs"] + v.get("agprs", 0) <= 256, (k, v)
    assert got == {1: 68, 2: 68, 3: 68, 4: 68, 5: 84}
    prog = tmp_path / "vis_lds.cpp"
    prog.write_text('#include <cstdio>\n#include "kernels.h"\nint main() { using namespace oar::k; '
                    'for (int dh = 8; dh <= 80; dh += 8) std::printf("%zu ", vis_attention_lds_bytes(dh)); '
                    'const int32_t lens[3] = {4, 60, 140}; std::printf("%lld %d %d\\n", (long long)vis_attention_tile_count(lens, 3, 2), kVisLd5, '
                    '(int)(vis_attention_supported(2, 72) && !vis_attention_supported(2, 12) && !vis_attention_supported(2, 88) && !vis_attention_supported(0, 8))); return 0; }\n')
    exe = tmp_path / "vis_lds"
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O0", "-I", str(build.CSRC), "-I", str(build.CSRC.parent.parent / "include"), str(prog), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    words = out.stdout.split()
    assert words[:8] == ["34816"] * 8 and words[8:10] == ["43008"] * 2 and words[10:] == ["10", "84", "1"], out.stdout   # 2 heads (1 + 1 + 3 tiles)
    assert all(2 * int(b) <= 160 * 1024 for b in words[:10])
    assert 84 % 4 == 0 and (84 // 4) % 2 == 1 and 84 >= 80 + 4                # the "+4" of the shared layout: an odd number of 16-byte slots per row


def test_vis_misc_kernel_resources():
    """vis_pos_embed_kernel and vis_merge_gather_kernel index their by-value image table with a run-time index: that must stay in scalar registers, not become scratch"""
    assert "vis_misc.hip" in build.SOURCES
    kernels = _resources(build.CSRC / "vis_misc.hip")
    assert len(kernels) == 2 and any("vis_pos_embed_kernel" in k for k in kernels) and any("vis_merge_gather_kernel" in k for k in kernels), sorted(kernels)
    for k, v in kernels.items():
        print(f"{k}: {v['vgprs']} VGPRs, {v.get('agprs', 0)} AGPRs, occupancy {v['occupancy']} waves / SIMD")
        assert v["spill"] == 0 and v.get("sgpr_spill", 0) == 0 and v["scratch"] == 0 and v["lds"] == 0, (k, v)
