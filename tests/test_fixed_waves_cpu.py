"""The fixed kernel at 8 and 4 waves per workgroup (crc32c_kernels.hip's
kWavesPerWg template parameter, crc32c_engine.cc fixed_waves_for): what can be
checked without a device.

* The queue protocol does not depend on W: WgQueue<W> is the one template, and
  its CPU restatements (tests/test_queue_schedule.py for the full queue,
  tests/test_queue_tail_schedule.py for the late start) run here at W = 8 and 4
  with the seeds, group counts, K0 and ring sizes those files use at 16.
* Codegen: an 8-wave workgroup must fit a CU at 2 waves per SIMD (<= 256
  VGPRs), a 4-wave one at 1 (<= 512), and either in the CU's 160 KiB of LDS.
  (tests/test_codegen.py's no-spill test covers the new symbols by name.)
* lsbm_test_fixed_waves takes 16, 8, 4 and -1, refuses anything else, and needs
  no device.
"""
import os
import random
import re
import shutil
import subprocess

import pytest

import test_queue_schedule as full
import test_queue_tail_schedule as tail

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NWG = {8: (2, 24), 4: (8, 2, 24)}  # the workgroup counts the two files use at 16, and the one they use at 4


@pytest.mark.parametrize("W", [8, 4])
@pytest.mark.parametrize("ring", [4, 2])
@pytest.mark.parametrize("K0", [1, 2, 5, "rows"])
def test_tail_queue_every_group_once(W, ring, K0):
    for nwg in NWG[W]:
        nwaves = nwg * W
        if K0 == "rows":
            cases = [(rows, rows * nwaves - d) for rows in (1, 3, 6) for d in (0, 1, nwaves - 1) if rows * nwaves - d > 0]
        else:
            cases = [(K0, ng) for ng in tail._ngroups_cases(K0, nwaves, W)]
        for k0, ng in cases:
            for seed in range(6):
                seen, items, claims = tail.simulate(ng, nwg, W, k0, ring, seed * 131 + ng)
                assert all(s == 1 for s in seen), (ng, nwg, W, k0, ring, seed)
                if K0 == "rows":
                    assert items == 0
                assert claims == items + 8 * nwg


@pytest.mark.parametrize("W", [8, 4])
@pytest.mark.parametrize("lead,ring", [(1, 4), (1, 2), (1, 3), (1, 8)])
def test_full_queue_every_group_once(W, lead, ring):
    """tests/test_queue_schedule.py's test_every_group_once, its seeds, workgroup
    and group counts, with W fixed."""
    for seed in range(150):
        r = random.Random(seed * 31 + lead * 7 + ring)
        r.choice([1, 2, 4, 16])  # (that test's draw of W: the same stream of draws after it)
        nwg = r.choice([1, 2, 8, 24])
        nw = nwg * W
        ng = r.choice([0, 1, nw, nw + 1, nw + W * 8 * 3 + 5, r.randrange(1, 4000)])
        seen = full.simulate(ng, nwg, W, lead, ring, seed)
        assert all(s == 1 for s in seen), (ng, nwg, W, lead, ring, seed)
        if ng and ring == 4:  # K0 = 1 is the same protocol in the late start's restatement
            assert tail.simulate(ng, nwg, W, 1, ring, seed)[0] == seen


def _metadata(asm):
    """{kernel symbol: {field: int}} from the assembly's amdhsa.kernels notes."""
    out = {}
    notes = asm[asm.index("amdhsa.kernels:"):]
    for entry in re.split(r"(?m)^  - ", notes)[1:]:  # one list item per kernel; its own keys sit at 4 spaces
        f = dict(re.findall(r"(?m)^(?:    )?\.(\w+):[ \t]+(\S+)[ \t]*$", entry))
        if "name" not in f:  # (amdhsa.version's items, behind the kernels)
            continue
        out[f["name"]] = {k: int(f[k]) for k in ("vgpr_count", "agpr_count", "group_segment_fixed_size",
                                                 "max_flat_workgroup_size", "private_segment_fixed_size")}
    return out


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_fat_wave_kernels_fit_one_workgroup_per_cu(tmp_path):
    src = os.path.join(REPO, "lsbm_amd", "csrc", "crc32c_kernels.hip")
    s_file = tmp_path / "crc32c_kernels.s"
    # the product's flags (lsbm_amd/csrc/Makefile HIPFLAGS + KERNEL_FLAGS)
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17",
                    "-w", "-fvisibility=hidden", "-munsafe-fp-atomics", "-mllvm",
                    "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-S", "-o", str(s_file), src],
                   check=True, timeout=900)
    md = _metadata(s_file.read_text())
    # crc32c_fixed_kernel<bool, rows, waves>: ...ILb{0,1}ELj{rows}ELj{waves}EE...
    found = {}
    for sym, f in md.items():
        m = re.search(r"crc32c_fixed_kernelILb([01])ELj(\d+)ELj(\d+)EE", sym)
        if m and "vgpr_count" in f:
            found[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = f
    fat = {k: f for k, f in found.items() if k[2] != 16}
    for init in (0, 1):
        for rows in (32, 512):
            assert (init, rows, 16) in found and (init, rows, 8) in found, sorted(found)
        assert (init, 0, 16) in found
    assert all(k[1] in (32, 512) for k in fat), sorted(fat)  # the generic-rows kernel stays at 16 waves
    for (init, rows, waves), f in sorted(fat.items()):
        print((init, rows, waves), f)
        assert waves in (8, 4)
        assert f["max_flat_workgroup_size"] == waves * 64
        assert f["vgpr_count"] <= (256 if waves == 8 else 512), ((init, rows, waves), f)
        assert f["group_segment_fixed_size"] <= 160 * 1024, ((init, rows, waves), f)
        assert f["private_segment_fixed_size"] == 0, ((init, rows, waves), f)


def test_hook_arguments(product_lib):
    lib = product_lib
    try:
        for ok in (16, 8, -1):
            assert lib.lsbm_test_fixed_waves(ok) == 0, ok
        for bad in (0, 3, 32):
            assert lib.lsbm_test_fixed_waves(bad) == -1, bad
        assert lib.lsbm_test_fixed_waves(4) == 0
    finally:
        lib.lsbm_test_fixed_waves(-1)
