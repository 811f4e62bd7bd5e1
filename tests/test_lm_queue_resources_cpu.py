"""Register guards of lm_queue.hip (hipcc cross-compiles without a GPU): the one kernel of the file touches neither scratch nor LDS, spills nothing and
reaches the occupancy DESIGN 4.44 states (8 waves per SIMD: a copy kernel hides its latency with waves in flight); and the grid the host asks for follows
entries x 16-byte groups."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from oar_ocr_amd.synth import lm_queue_cases as Q

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "oar_ocr_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
OCCUPANCY = 8

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


def test_lm_queue_turnover_kernel():
    res = {k: v for k, v in _resources("lm_queue.hip").items() if "_kernel" in k}
    assert len(res) == 1 and "lm_queue_turnover_kernel" in next(iter(res)), sorted(res)
    r = next(iter(res.values()))
    print(f"lm_queue_turnover_kernel: {r['vgprs']} VGPRs, {r.get('agprs', 0)} AGPRs, {r['occupancy']} waves / SIMD, LDS {r['lds']} B")
    assert r["spill"] == 0 and r.get("sgpr_spill", 0) == 0 and r["scratch"] == 0 and r["lds"] == 0, r
    assert r["occupancy"] == OCCUPANCY, r


def test_the_turnover_grid_is_sized_by_the_rows_it_moves():
    """The header's lm_queue_turnover_blocks, compiled for the host: one workgroup per entry without logits; with them one per 256 x 8 16-byte groups of a sequence's
    max_new x V floats -- 64 x 103424 floats are 1654784 groups, 808 workgroups -- and at most max_blocks."""
    c = Q.queue_constants()
    assert (c["threads"], c["vec_per_thread"], c["max_blocks"]) == (256, 8, 2048)
    assert c["blocks"] == [1, 1, 1, 808, 2048]
    src = (CSRC / "lm_queue.hip").read_text()
    assert "atomic" not in src.split("namespace oar")[1] and "__shared__" not in src
