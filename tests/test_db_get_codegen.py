"""Codegen guard (CPU; needs hipcc) for the kernels of the batched Get
(lsbm_amd/csrc/get_kernels.hip): none of them spills, and none needs more
registers than full occupancy admits.  The binary searches are chains of
dependent key loads that only other waves can hide, so every kernel is held to
8 waves per SIMD: 512 registers a lane divided by 8 caps each at 64 VGPRs.  No
kernel here declares LDS, so LDS never limits.  Reads only the register,
scratch and LDS figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> LDS bytes a workgroup may use
KERNELS = {"get_offsets_kernel": 0, "lookup_check_kernel": 0, "lookup_keys_kernel": 0, "mem_get_kernel": 0,
           "run_check_kernel": 0, "find_file_kernel": 0, "save_check_kernel": 0, "save_value_kernel": 0,
           "slices_gather_kernel": 0}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_get_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "get_kernels.hip")
    s_file = tmp_path / "get_kernels.s"
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
        assert vgprs[syms[0]] <= 64, (k, vgprs[syms[0]])
