"""The fixed kernel's tail queue (crc32c_engine.cc mode 2, crc32c_units.h WgQueue
own_rows): the first K0 rows of a launch are the static interleave's, the last
rows are handed out through the cross-XCC queue.

The test hook lowers the tail path's minimum to 2 rows (groups per wave) and
sets the tail to 1 or 2 rows, so batches of 2, 3 and 5 rows reach it with
K0 = 1 .. 4.  Batch sizes sit around 8 * nwaves * rows blocks: exactly on it,
one less (the last static row's last group is short), one more (one queue item
of one block), + 9 (a second, short group), and a size with several items and
n % 8 != 0.  Every block must equal the oracle, whose CRCs are computed once per
geometry for the largest batch (a block's CRC does not depend on the batch), and
so must the static schedule (0) and the full queue (1) on the same buffer.
The queue's heads come from the device's pool of head sets, which the last
workgroup of a launch hands back zeroed (pool 1: every set must be free again
once the launches have ended, and launch after launch reuses them), or from
per-call scratch (pool 0, what a launch gets when no set is free)."""
import numpy as np
import pytest

from golden.splitmix import stream_bytes

pytestmark = pytest.mark.gpu

ROWS = {128: (2, 3, 5), 256: (2, 3, 5), 4096: (2, 3)}
EXTRA = 8 * 16 * 5 + 3  # five items and a partial group past the static rows


def _sizes(nwaves, rows):
    n0 = 8 * nwaves * rows
    return [n0, n0 - 1, n0 + 1, n0 + 9, n0 + EXTRA]


@pytest.fixture(scope="module")
def nwaves(torch_cuda):
    return torch_cuda.cuda.get_device_properties(0).multi_processor_count * 16


@pytest.fixture(scope="module", params=[128, 256, 4096])
def case(request, torch_cuda, oracle, nwaves):
    """One buffer per geometry, and the oracle's CRCs of its blocks: (no init,
    unmasked) and (init, masked)."""
    torch = torch_cuda
    length = request.param
    stride = length + 16 if length < 4096 else length
    n_max = 8 * nwaves * max(ROWS[length]) + EXTRA
    data = stream_bytes(0x7A11 + length, 0, (n_max - 1) * stride + length)
    init = np.random.default_rng(length).integers(0, 2**32, size=n_max, dtype=np.uint64).astype(np.uint32)
    want = {(False, False): oracle.batch_fixed(data, stride, length, n_max, None, False),
            (True, True): oracle.batch_fixed(data, stride, length, n_max, init, True)}
    d = torch.from_numpy(data).to("cuda")
    di = torch.from_numpy(init).view(torch.int32).to("cuda")
    want_d = {k: torch.from_numpy(v.view(np.int32)).to("cuda") for k, v in want.items()}
    return length, stride, d, di, want_d


@pytest.mark.parametrize("use_init,masked", [(False, False), (True, True)])
@pytest.mark.parametrize("tail", [1, 2])
@pytest.mark.parametrize("pool", [1, 0])
def test_tail_queue_matches_oracle_and_other_schedules(torch_cuda, product_lib, nwaves, case, pool, tail, use_init,
                                                       masked):
    torch = torch_cuda
    from lsbm_amd import engine
    length, stride, d, di, want_d = case
    want = want_d[(use_init, masked)]
    try:
        assert product_lib.lsbm_test_fixed_tail(2, tail) == 0
        assert product_lib.lsbm_test_queue_pool(pool) == 0
        for rows in ROWS[length]:
            for n in _sizes(nwaves, rows):
                got = {}
                for mode in (2, 0, 1):
                    assert product_lib.lsbm_test_fixed_queue(mode) == 0
                    out = torch.zeros(n, dtype=torch.int32, device="cuda")
                    engine.crc32c_fixed(d, stride, length, n, init=di[:n] if use_init else None,
                                        masked=masked, out=out)
                    got[mode] = out
                bad = int((got[2] != want[:n]).sum())
                assert bad == 0, (length, rows, n, tail, bad)
                assert torch.equal(got[0], got[2]) and torch.equal(got[1], got[2]), (length, rows, n, tail)
        torch.cuda.synchronize()
        assert product_lib.lsbm_test_queue_pool_busy(0) == 0
    finally:
        product_lib.lsbm_test_fixed_tail(-1, -1)
        product_lib.lsbm_test_queue_pool(1)
        product_lib.lsbm_test_fixed_queue(-1)
