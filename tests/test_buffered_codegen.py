"""Codegen guard (CPU; needs hipcc) for the probe plan's kernels
(lsbm_amd/csrc/probe_kernels.hip): none of them spills, none uses LDS, and none
needs more registers than the occupancy it is meant to run at.  The count, the
first-check and the emit kernel are one lane per query: a chain of dependent
loads per lane (a key offset, the key's bytes against the cursor's, one
candidate byte per slot) that only other waves can hide; the two check kernels
are one load or two per lane.  All are therefore held to full occupancy, 8
waves per SIMD, 512 registers a lane / 8 = 64 VGPRs, the rule of
test_log_read_codegen.py.  Reads only the register, scratch and LDS figures of
the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> (LDS bytes a workgroup may use, VGPR cap)
KERNELS = {"probe_check_kernel": (0, 64), "probe_cand_check_kernel": (0, 64), "probe_count_kernel": (0, 64),
           "probe_first_check_kernel": (0, 64), "probe_emit_kernel": (0, 64)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_probe_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "probe_kernels.hip")
    s_file = tmp_path / "probe_kernels.s"
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
    assert len([s for s in scratch if "probe_" in s]) == len(KERNELS)  # every kernel of the file is listed above
    for k, (lds_bytes, vgpr_cap) in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert vgprs[syms[0]] <= vgpr_cap, (k, vgprs[syms[0]])
