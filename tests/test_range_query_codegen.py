"""Codegen guard (CPU; needs hipcc) for the range query's kernels
(lsbm_amd/csrc/range_kernels.hip): none of them spills, none uses LDS, and none
needs more registers than the occupancy it is meant to run at.

The plan, the first-check and the emit kernel are one lane per query: a chain
of dependent loads per lane (the slot table, a run's offsets, a bound's bytes
against the query's) that only other waves can hide.  The count kernel is one
wave per pair, and a pair is a short dependent chain too (three search steps,
then an offset load and a key load per 64 entries), so it also lives on the
number of waves a SIMD holds.  The reduce kernel is a short loop of loads per
lane; the two check kernels are a load or two per lane.  All are therefore held
to full occupancy, 8 waves per SIMD, 512 registers a lane / 8 = 64 VGPRs, the
rule of test_buffered_codegen.py.  Reads only the register, scratch and LDS
figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> (LDS bytes a workgroup may use, VGPR cap)
KERNELS = {"range_check_kernel": (0, 64), "range_plan_kernel": (0, 64), "range_first_check_kernel": (0, 64),
           "range_emit_kernel": (0, 64), "range_index_check_kernel": (0, 64), "range_count_kernel": (0, 64),
           "range_reduce_kernel": (0, 64)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_range_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "range_kernels.hip")
    s_file = tmp_path / "range_kernels.s"
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
    assert len([s for s in scratch if "range_" in s]) == len(KERNELS)  # every kernel of the file is listed above
    for k, (lds_bytes, vgpr_cap) in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert vgprs[syms[0]] <= vgpr_cap, (k, vgprs[syms[0]])
