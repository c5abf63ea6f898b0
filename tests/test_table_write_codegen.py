"""Codegen guard (CPU; needs hipcc) for the batched table finish's kernels
(lsbm_amd/csrc/table_write_kernels.hip): none of them spills, none uses more
LDS than its stated figure, and none needs more registers than the occupancy
it is meant to run at.  All of them are bookkeeping: a lane per block, table,
handle or entry does a few dependent loads (a binary search in
table_block_first or seg_first, a running sum read back, a key compare) that
only other waves can hide, so every one is held to full occupancy, 8 waves per
SIMD, 512 registers a lane / 8 = 64 VGPRs.  LDS: the scans keep
one word per wave (32 bytes), the sort's tile 256 {word, entry, segment}
triples (4,096 bytes); 8 workgroups of the largest are 32 KiB of the CU's 160,
so LDS never limits them.  Reads only the register, scratch and LDS figures of
the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> (LDS bytes a workgroup may use, VGPR cap, workgroups that share a CU)
KERNELS = {"tw_check_tables_kernel": (0, 64, 8), "tw_scan_tiles_kernel": (32, 64, 8),
           "tw_plan_tile_kernel": (32, 64, 8), "tw_plan_apply_kernel": (0, 64, 8),
           "tw_filter_tile_kernel": (32, 64, 8), "tw_filter_emit_kernel": (0, 64, 8),
           "tw_filter_tables_kernel": (0, 64, 8), "tw_metaindex_kernel": (0, 64, 8), "tw_place_kernel": (0, 64, 8),
           "seg_check_kernel": (0, 64, 8), "seg_tile_sort_kernel": (4096, 64, 8), "seg_merge_kernel": (0, 64, 8),
           "seg_len_kernel": (32, 64, 8), "seg_scan_kernel": (32, 64, 8), "seg_emit_kernel": (32, 64, 8)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_table_write_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "table_write_kernels.hip")
    s_file = tmp_path / "table_write_kernels.s"
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
    assert len([s for s in scratch if "_kernel" in s]) == len(KERNELS)  # every kernel of the file is listed above
    for k, (lds_bytes, vgpr_cap, per_cu) in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert per_cu * max(lds_bytes, 1) <= 160 * 1024
        assert vgprs[syms[0]] <= vgpr_cap, (k, vgprs[syms[0]])
