"""Codegen guard (CPU; needs hipcc) for the memtable flush's kernels
(lsbm_amd/csrc/memtable_kernels.hip): none of them spills, and none needs more
registers than the occupancy its LDS use admits.  The walks are chains of
dependent byte loads and the merge passes chains of dependent key loads that
only other waves can hide, so every kernel is held to full occupancy.  The
largest LDS user is the tile sort: 256 sort words of 8 bytes and 256 entry
indices of 4 bytes, 3,072 bytes a workgroup of 4 waves.  The CU's 160 KiB admit
163,840 / 3,072 = 53 such workgroups, far more than the 8 workgroups (32 waves,
8 per SIMD) a CU can hold; the scans' 32-byte rows admit more still, and the
other kernels use no LDS.  So LDS never limits, 8 waves per SIMD is the
target, and 512 registers a lane divided by 8 waves caps every kernel at 64
VGPRs.  Reads only the register, scratch and LDS figures of the compiler's
listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> LDS bytes a workgroup may use
KERNELS = {"wb_scan_kernel": 0, "wb_decode_kernel": 0, "mem_check_kernel": 0, "mem_tile_sort_kernel": 3072,
           "mem_merge_kernel": 0, "mem_len_kernel": 32, "mem_scan_kernel": 32, "mem_emit_kernel": 32}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_memtable_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "memtable_kernels.hip")
    s_file = tmp_path / "memtable_kernels.s"
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
    for k, lds_bytes in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        # 8 workgroups of 4 waves fit the CU's 160 KiB of LDS: 8 waves per SIMD
        assert 8 * max(lds_bytes, 1) <= 160 * 1024
        assert vgprs[syms[0]] <= 64, (k, vgprs[syms[0]])
