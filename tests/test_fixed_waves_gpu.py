"""The fixed kernel at 16, 8 and 4 waves per workgroup (lsbm_test_fixed_waves)
under the three schedules (lsbm_test_fixed_queue 0 static, 1 full queue, 2 tail
queue): every CRC equals the oracle's, whatever the wave count and schedule.

4 KiB blocks (rows 32), stride 4096 and 4112, without init unmasked and with
init masked, with the tail path's minimum lowered to 2 rows and its tail to 1
(lsbm_test_fixed_tail(2, 1)):
  * n = 1, 7, 8, 9: one group, short and full, and a second one of one block;
  * n = 8 W CUs - 1, 8 W CUs, 8 W CUs + 1 for every wave count W: one row of
    the launch at W waves, its last group short, and one block more, which at
    W waves is a second row (K0 = 1, one item with one slot filled);
  * n = 8 (16 CUs) 2 + 8 16 5 + 3: two static rows at 16 waves (four at 8), a
    tail of several items, a short last group and a last item with empty slots.
Every n runs at every wave count.  64 KiB blocks (rows 512): n = 1, 9 and
8 8 3 + 5 on the static path.  Any other row count stays on the 16-wave kernel
(launch_fixed refuses it at another count): len 256, stride 272 with the hook
at 8.  The oracle's CRCs are computed once per geometry for the largest batch.
"""
import numpy as np
import pytest

from golden.splitmix import stream_bytes

pytestmark = pytest.mark.gpu

WAVES = (16, 8, 4)


def _restore(lib):
    lib.lsbm_test_fixed_waves(-1)
    lib.lsbm_test_fixed_queue(-1)
    lib.lsbm_test_fixed_tail(-1, -1)


def _check(torch, lib, d, di, want_d, stride, length, sizes):
    from lsbm_amd import engine
    for use_init, masked in ((False, False), (True, True)):
        want = want_d[(use_init, masked)]
        for n in sizes:
            first = None
            for waves in WAVES:
                assert lib.lsbm_test_fixed_waves(waves) == 0
                for mode in (0, 1, 2):
                    assert lib.lsbm_test_fixed_queue(mode) == 0
                    out = torch.zeros(n, dtype=torch.int32, device="cuda")
                    engine.crc32c_fixed(d, stride, length, n, init=di[:n] if use_init else None, masked=masked, out=out)
                    bad = int((out != want[:n]).sum())
                    assert bad == 0, (length, stride, n, waves, mode, use_init, bad)
                    if first is None:
                        first = out
                    assert torch.equal(out, first), (length, stride, n, waves, mode, use_init)
    torch.cuda.synchronize()
    assert lib.lsbm_test_queue_pool_busy(0) == 0


def _case(torch, oracle, seed, stride, length, n_max):
    data = stream_bytes(seed, 0, (n_max - 1) * stride + length)
    init = np.random.default_rng(seed).integers(0, 2**32, size=n_max, dtype=np.uint64).astype(np.uint32)
    want = {(False, False): oracle.batch_fixed(data, stride, length, n_max, None, False),
            (True, True): oracle.batch_fixed(data, stride, length, n_max, init, True)}
    d = torch.from_numpy(data).to("cuda")
    di = torch.from_numpy(init).view(torch.int32).to("cuda")
    return d, di, {k: torch.from_numpy(v.view(np.int32)).to("cuda") for k, v in want.items()}


@pytest.mark.parametrize("stride", [4096, 4112])
def test_4k_blocks_every_wave_count_and_schedule(torch_cuda, product_lib, oracle, stride):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_tail = 8 * (16 * cus) * 2 + 8 * 16 * 5 + 3
    sizes = [1, 7, 8, 9] + [8 * w * cus + d for w in WAVES for d in (-1, 0, 1)] + [n_tail]
    d, di, want_d = _case(torch, oracle, 0xFA7 + stride, stride, 4096, n_tail)
    try:
        assert product_lib.lsbm_test_fixed_tail(2, 1) == 0
        _check(torch, product_lib, d, di, want_d, stride, 4096, sizes)
    finally:
        _restore(product_lib)


def test_64k_blocks_every_wave_count_and_schedule(torch_cuda, product_lib, oracle):
    torch = torch_cuda
    sizes = [1, 9, 8 * 8 * 3 + 5]
    d, di, want_d = _case(torch, oracle, 0xFA7512, 65536, 65536, max(sizes))
    try:
        _check(torch, product_lib, d, di, want_d, 65536, 65536, sizes)
    finally:
        _restore(product_lib)


def test_other_row_counts_stay_on_sixteen_waves(torch_cuda, product_lib, oracle):
    torch = torch_cuda
    from lsbm_amd import engine
    n, length, stride = 1000, 256, 272
    d, di, want_d = _case(torch, oracle, 0xFA7256, stride, length, n)
    try:
        assert product_lib.lsbm_test_fixed_waves(8) == 0
        for (use_init, masked), want in want_d.items():
            out = torch.zeros(n, dtype=torch.int32, device="cuda")
            engine.crc32c_fixed(d, stride, length, n, init=di if use_init else None, masked=masked, out=out)
            assert torch.equal(out, want), (use_init, masked)
        torch.cuda.synchronize()
        assert product_lib.lsbm_test_queue_pool_busy(0) == 0
    finally:
        _restore(product_lib)
