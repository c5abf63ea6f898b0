"""Codegen guard (CPU; needs hipcc) for the block builder's kernels
(lsbm_amd/csrc/block_build_kernels.hip): none of them spills.  The build and
index kernels hold a block's 64 entries in registers between the sizing pass
and the copy; a spill would put scratch traffic into the copy loop's vmcnt
queue.  Reads only the register and scratch figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("plan_sizes_kernel", "plan_links_kernel", "plan_chain_kernel", "plan_scan_kernel", "plan_emit_kernel",
           "block_build_kernel", "index_build_kernel")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_block_build_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "block_build_kernels.hip")
    s_file = tmp_path / "block_build_kernels.s"
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
        # 4 waves per SIMD at the least (the LDS tiles admit 4 workgroups per CU)
        assert vgprs[syms[0]] <= 128, (k, vgprs[syms[0]])
