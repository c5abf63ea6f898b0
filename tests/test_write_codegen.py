"""Codegen guard (CPU; needs hipcc) for the batched DB::Write's kernels
(lsbm_amd/csrc/write_kernels.hip): none of them spills, none uses more LDS than
its stated figure, and none needs more registers than the occupancy it is
meant to run at.  The check, sizes, links, plan and verify kernels are a few
dependent loads per lane (offsets, then a binary search in the running sums)
that only other waves can hide, so they are held to full occupancy: 8 waves
per SIMD, 512 registers a lane / 8 = 64 VGPRs.  The group chain and the frame plan run one wave
in all and are held to the same 64.  The two movers carry an op's or a record's
whole description and the 16 bytes they assemble; their dependent chain is two
binary searches and then independent 16-byte chunks, and six waves per SIMD
hide that: 512 / 6 = 85, rounded down to the allocation granule of 8: 80 VGPRs.
The largest LDS user is the frame plan, 1,024 lengths of 8 bytes = 8,192
bytes for its single workgroup; the group chain stages 1,024 links of 4 bytes;
the scans use 32 bytes of wave totals (the sync scan 16).  LDS never limits:
8 workgroups of the largest figure are 64 KiB of the CU's 160.  Reads only the
register, scratch and LDS figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> (LDS bytes a workgroup may use, VGPR cap)
KERNELS = {"wr_size_tile_kernel": (32, 64), "wr_scan_tiles_kernel": (32, 64), "wr_size_apply_kernel": (32, 64),
           "wr_batch_sum_kernel": (0, 64), "wr_next_sync_kernel": (16, 64), "wr_group_links_kernel": (0, 64),
           "wr_group_chain_kernel": (4096, 64), "wr_group_emit_kernel": (0, 64), "wr_build_check_kernel": (0, 64),
           "wr_build_plan_kernel": (0, 64), "wr_build_move_kernel": (0, 80), "wr_frame_check_kernel": (0, 64),
           "wr_frame_plan_kernel": (8192, 64), "wr_frame_verify_kernel": (0, 64), "wr_frame_move_kernel": (0, 80)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_write_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "write_kernels.hip")
    s_file = tmp_path / "write_kernels.s"
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
    assert len([s for s in scratch if "wr_" in s]) == len(KERNELS)  # every kernel of the file is listed above
    for k, (lds_bytes, vgpr_cap) in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert 8 * max(lds_bytes, 1) <= 160 * 1024
        assert vgprs[syms[0]] <= vgpr_cap, (k, vgprs[syms[0]])
