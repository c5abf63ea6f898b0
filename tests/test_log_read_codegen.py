"""Codegen guard (CPU; needs hipcc) for the batched log::Reader's kernels
(lsbm_amd/csrc/log_read_kernels.hip): none of them spills, none uses more LDS
than its stated figure, and none needs more registers than the occupancy it is
meant to run at.  The walk, check, cut, classify, state, scratch, count, slot
and fragment kernels and the scans are chains of a few dependent loads per lane
(a header's bytes, a binary search in the running counts, a neighbour slot's
state) that only other waves can hide, so they are held to full occupancy: 8
waves per SIMD, 512 registers a lane / 8 = 64 VGPRs.  The mover carries a
fragment's description and the 16 bytes it assembles; its dependent chain is
one binary search and then independent 16-byte chunks, and six waves per SIMD
hide that: 512 / 6 = 85, rounded down to the allocation granule of 8: 80 VGPRs,
the write movers' derivation.  The walk stages one 32 KiB block and 16 bytes
of address phase in LDS; it is held to 40,960 bytes, so that four workgroups
fit a CU's 160 KiB.  The scans use 32 bytes of wave totals.  Reads only the
register, scratch and LDS figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WALK_LDS = 40960
# kernel -> (LDS bytes a workgroup may use, VGPR cap)
KERNELS = {"lr_walk_kernelILb0": (WALK_LDS, 64), "lr_walk_kernelILb1": (WALK_LDS, 64), "lr_walk_scan_kernel": (32, 64),
           "lr_walk_publish_kernel": (0, 64), "lr_plan_check_kernel": (0, 64), "lr_plan_cut_kernel": (0, 64),
           "lr_plan_classify_kernel": (32, 64), "lr_plan_scan_a_kernel": (32, 64), "lr_plan_state_kernel": (32, 64),
           "lr_plan_scratch_kernel": (0, 64), "lr_plan_count_kernel": (32, 64), "lr_plan_scan_b_kernel": (32, 64),
           "lr_emit_check_kernel": (0, 64), "lr_emit_slots_kernel": (32, 64), "lr_emit_frags_kernel": (0, 64),
           "lr_emit_move_kernel": (0, 80)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_log_read_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "log_read_kernels.hip")
    s_file = tmp_path / "log_read_kernels.s"
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
    assert len([s for s in scratch if "lr_" in s]) == len(KERNELS)  # every kernel of the file is listed above
    for k, (lds_bytes, vgpr_cap) in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert 4 * max(lds_bytes, 1) <= 160 * 1024
        assert vgprs[syms[0]] <= vgpr_cap, (k, vgprs[syms[0]])
