"""Codegen guard (CPU; needs hipcc) for the batched VersionEdit's kernels
(lsbm_amd/csrc/manifest_kernels.hip): none of them spills, none uses more LDS
than its stated figure, and none needs more registers than the occupancy it is
meant to run at.  Every kernel is a chain of a few dependent loads per lane (a
group's varint bytes one after the other, a binary search in the records'
running lengths or the edits' running counts, the next-pointer of a
next-pointer) that only other waves can hide, so all are held to full
occupancy: 8 waves per SIMD, 512 registers a lane / 8 = 64 VGPRs, the
condition of tests/test_log_read_codegen.py.  The kernels that sum over a
workgroup use 32 bytes of wave totals; no kernel stages bytes in LDS.  Reads
only the register, scratch and LDS figures of the compiler's listing.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel -> (LDS bytes a workgroup may use, VGPR cap)
KERNELS = {"mf_dec_first_kernel": (32, 64), "mf_dec_parse_kernel": (0, 64), "mf_dec_round_kernel": (0, 64),
           "mf_dec_verdict_kernel": (0, 64), "mf_dec_flag_kernel": (32, 64), "mf_dec_scan_kernel": (32, 64),
           "mf_dec_publish_kernel": (0, 64), "mf_dec_check_kernel": (0, 64), "mf_dec_items_kernel": (32, 64),
           "mf_dec_tail_kernel": (0, 64), "mf_scan_sum_kernel": (32, 64), "mf_scan_tiles_kernel": (32, 64),
           "mf_scan_apply_kernel": (32, 64), "mf_enc_size_kernel": (0, 64), "mf_enc_owner_kernel": (0, 64),
           "mf_enc_edit_kernel": (0, 64), "mf_enc_publish_kernel": (0, 64), "mf_enc_check_kernel": (0, 64),
           "mf_enc_edits_kernel": (0, 64), "mf_enc_dels_kernel": (0, 64), "mf_enc_news_kernel": (0, 64)}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_manifest_kernels_do_not_spill(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "manifest_kernels.hip")
    s_file = tmp_path / "manifest_kernels.s"
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
    assert len([s for s in scratch if "mf_" in s]) == len(KERNELS)  # every kernel of the file is listed above
    for k, (lds_bytes, vgpr_cap) in KERNELS.items():
        syms = [s for s in scratch if k in s]
        assert len(syms) == 1, (k, sorted(scratch))
        assert scratch[syms[0]] == 0, (k, scratch[syms[0]])
        assert lds[syms[0]] <= lds_bytes, (k, lds[syms[0]])
        assert vgprs[syms[0]] <= vgpr_cap, (k, vgprs[syms[0]])
