"""Codegen guard (CPU; needs hipcc) for the table packer's kernels
(lsbm_amd/csrc/table_pack_kernels.hip): none of them spills, and none needs
more registers than the occupancy it is meant to run at.

The plan, scan and count kernels use 32 bytes of LDS a workgroup (one scan row
of 4 waves), the mover none, so the CU's 160 KiB of LDS admit any occupancy and
the registers alone decide it.  The scan kernels are one short pass each and
are held to full occupancy: 8 waves per SIMD, which 512 registers a lane divided
by 8 waves caps at 64 VGPRs.  The mover holds the 2 chunks a lane has in flight
(2 x 2 aligned 16-byte source words = 16 registers) beside its piece's
description and the addresses; it is held to 5 waves per SIMD = 20 waves a CU,
each with 4 KiB of loads in flight (80 KiB a CU, above the 72 KiB at which a
gather is measured to run at the memory's rate): 512 / 5 = 102, which the
allocation granule of 8 registers makes 96 VGPRs.  (With 4 chunks in flight it
needed 131 registers, 3 waves per SIMD, and measured 0.8 of this rate.)  Reads
only the register and scratch figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> the VGPRs its occupancy admits
KERNELS = {"pack_plan_tile_kernel": 64, "pack_scan_tiles_kernel": 64, "pack_plan_apply_kernel": 64,
           "pack_count_kernel": 64, "pack_move_kernel": 96}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_table_pack_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "table_pack_kernels.hip")
    s_file = tmp_path / "table_pack_kernels.s"
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-w", "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-o", str(s_file), src],
                   check=True, timeout=900)
    scratch, vgprs, name = {}, {}, None
    for line in s_file.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        m = re.match(r"^; ScratchSize: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.match(r"^; NumVgprs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
    for k, cap in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert vgprs[syms[0]] <= cap, (k, vgprs[syms[0]])
