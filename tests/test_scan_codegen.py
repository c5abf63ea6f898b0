"""Codegen guard (CPU; needs hipcc) for the kernels of the batched range scan
(lsbm_amd/csrc/iter_kernels.hip): none of them spills, and none needs more
registers than full occupancy admits.  The binary searches of the range kernel
are chains of dependent key loads that only other waves can hide, and the plan
kernels stream the entries twice, so every kernel is held to 8 waves per SIMD:
512 registers a lane divided by 8 caps each at 64 VGPRs.  The plan kernels keep
one row of wave totals in LDS (and the flag kernel its candidate word), the
output kernel two rows of 64 offsets per wave.  Reads only the register,
scratch and LDS figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
WAVES = 4
# kernel -> LDS bytes a workgroup declares
KERNELS = {"iter_offsets_kernel": 0, "iter_check_kernel": 0,
           "iter_flag_kernel": 8 * 3 * WAVES + 8,        # lds[waves][3], s_cand
           "iter_scan_kernel": 8 * WAVES + 8 * 6,        # lds[waves], s_carry[6]
           "iter_emit_kernel": 8 * 3 * WAVES,            # lds[waves][3]
           "iter_range_kernel": 0,
           "iter_emit_out_kernel": 8 * WAVES * (65 + 64)}  # s_out[waves][65], s_src[waves][64]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_iter_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "iter_kernels.hip")
    s_file = tmp_path / "iter_kernels.s"
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
    kernels = [s for s in scratch if "_kernel" in s]
    assert len(kernels) == len(KERNELS), sorted(kernels)  # every kernel of the file is listed above
    for k, lds_bytes in KERNELS.items():
        syms = [s for s in scratch if k + "E" in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert vgprs[syms[0]] <= 64, (k, vgprs[syms[0]])
