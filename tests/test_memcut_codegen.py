"""Codegen guard (CPU; needs hipcc) for the memtable switch's kernels
(lsbm_amd/csrc/memcut_kernels.hip): none of them spills, none uses more LDS
than its stated figure, and none needs more registers than the occupancy it is
meant to run at.  The three heights kernels are arithmetic on a lane's own 64
draws, and the slots and commit kernels a few dependent loads per lane (a
binary search in the records' running sums) that only other waves can hide:
all five are held to full occupancy, 8 waves per SIMD, 512 registers a lane /
8 = 64 VGPRs.  The walk is one workgroup in all, whose first wave walks out of
LDS while the others only move chunks: one wave per SIMD, so no occupancy
depends on its registers (16 chunk loads a lane are in flight at once, which
is where they go); it is held to 128, the figure for four waves per SIMD, so
that growth does not go unnoticed; the one-lane form of the walk
(mc_walk_lane_kernel, the measured fallback) is the same workgroup and is held
to the same figures.  LDS: the
runs kernel keeps 256 runs of 16 bytes (4,096), the emit kernel those and 256
lane starts of 16 bytes (8,192); 8 workgroups of the largest are 64 KiB of the
CU's 160, so LDS never limits them.  The walk's single workgroup stages 4,096
slot words (32,768 bytes) and two rows of 4,096 heights (8,192), with two
words of its own: 40,976 bytes, held to 40,992.  Reads only the register,
scratch and LDS figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> (LDS bytes a workgroup may use, VGPR cap, workgroups that share a CU)
KERNELS = {"mc_heights_runs_kernel": (4096, 64, 8), "mc_heights_link_kernel": (0, 64, 8),
           "mc_heights_emit_kernel": (8192, 64, 8), "mc_slots_kernel": (0, 64, 8), "mc_walk_kernel": (40992, 128, 1),
           "mc_walk_lane_kernel": (40992, 128, 1),
           "mc_commit_kernel": (0, 64, 8)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_memcut_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "memcut_kernels.hip")
    s_file = tmp_path / "memcut_kernels.s"
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-w", "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-o", str(s_file), src],
                   check=True, timeout=900)
    scratch, vgprs, lds, name = {}, {}, {}, None
    for line in s_file.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        for table, pattern in ((scratch, r"^; ScratchSize: (\d+)"), (vgprs, r"^; NumVgprs: (\d+)"),
                               (lds, r"^; LDSByteSize: (\d+)")):
            m = re.match(pattern, line)
            if m and name:
                table[name] = int(m.group(1))
    assert len([s for s in scratch if "mc_" in s]) == len(KERNELS)  # every kernel of the file is listed above
    for k, (lds_bytes, vgpr_cap, per_cu) in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert per_cu * max(lds_bytes, 1) <= 160 * 1024
        assert vgprs[syms[0]] <= vgpr_cap, (k, vgprs[syms[0]])
