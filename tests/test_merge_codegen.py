"""Codegen guard (CPU; needs hipcc) for the compaction merge's kernels
(lsbm_amd/csrc/merge_kernels.hip): none of them spills, and none needs more
registers than the occupancy its LDS use admits.  The rank kernel's binary
searches are chains of dependent key loads that only other waves can hide, so
the kernels are held to full occupancy: the largest LDS user (the gather's
per-wave rows, about 4 KiB a workgroup of 4 waves) admits 8 workgroups of the
CU's 160 KiB many times over, that is 8 waves per SIMD, which 512 registers a
lane divided by 8 waves caps at 64 VGPRs.  Reads only the register and scratch
figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("merge_init_kernel", "merge_check_kernel", "merge_sample_kernel", "merge_rank_kernel",
           "merge_flag_kernel", "merge_scan_kernel", "merge_emit_kernel", "merge_gather_kernel")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_merge_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "merge_kernels.hip")
    s_file = tmp_path / "merge_kernels.s"
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
    for k in KERNELS:
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        # 8 waves per SIMD (the LDS rows admit 8 workgroups per CU and more)
        assert vgprs[syms[0]] <= 64, (k, vgprs[syms[0]])
