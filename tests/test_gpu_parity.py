"""GPU parity: every kernel result through the C ABI == the oracle, bit for bit.

The oracle (oracle/crc32c_oracle.c) is pinned to lsbm's own util/crc32c.cc by
tests/test_oracle.py.  Small/medium cases are checked block-for-block; the
full-size benchmark configs are checked on sampled blocks plus
size-independent properties (two independent kernels agree on every block;
known golden blocks of each config buffer).
"""
import functools

import numpy as np
import pytest

from golden.splitmix import printable_bytes, stream_bytes

pytestmark = pytest.mark.gpu


def _dev(torch, arr, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if dtype is not None:
        t = t.view(dtype)
    return t.to("cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- fixed-stride
@pytest.mark.parametrize("length,stride,n", [
    (128, 128, 1), (128, 128, 9), (256, 256, 17), (512, 640, 33), (4096, 4096, 1),
    (4096, 4096, 7), (4096, 4096, 1000), (4096, 8192, 129), (8192, 8192, 65),
    (65536, 65536, 24), (384, 384, 100), (1152, 1280, 50), (640, 640, 41),
])
@pytest.mark.parametrize("use_init,masked", [(False, False), (True, False), (False, True)])
def test_fixed_fast_path(torch_cuda, oracle, length, stride, n, use_init, masked):
    torch = torch_cuda
    from lsbm_amd import engine
    nbytes = (n - 1) * stride + length
    data = stream_bytes(length * 131 + n + stride, 0, nbytes)
    rng = np.random.default_rng(length + n)
    init = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32) if use_init else None
    d = _dev(torch, data)
    di = _dev(torch, init, torch.int32) if use_init else None
    got = _u32(engine.crc32c_fixed(d, stride, length, n, init=di, masked=masked))
    want = oracle.batch_fixed(data, stride, length, n, init, masked)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("use_init,masked", [(False, False), (True, True)])
def test_fixed_batch_split_into_launches(torch_cuda, oracle, use_init, masked):
    """A batch of >= 2 x LSBM_FIXED_SPLIT_BLOCKS (default 1M) blocks goes as
    several launches (crc32c_engine.cc lsbm_crc32c_fixed_dev); every block,
    the launch boundaries included, matches the oracle."""
    torch = torch_cuda
    from lsbm_amd import engine
    length, n = 128, 3 * (1 << 20) + 77  # launches of 1M, 1M and 1M + 77 blocks
    data = stream_bytes(4242, 0, n * length)
    rng = np.random.default_rng(5)
    init = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32) if use_init else None
    d = _dev(torch, data)
    di = _dev(torch, init, torch.int32) if use_init else None
    got = _u32(engine.crc32c_fixed(d, length, length, n, init=di, masked=masked))
    want = oracle.batch_fixed(data, length, length, n, init, masked)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [131_072 + 3, 300_001, 1_048_576])
@pytest.mark.parametrize("use_init,masked", [(False, False), (True, True)])
def test_fixed_cross_xcc_queue(torch_cuda, oracle, product_lib, n, use_init, masked):
    """The fixed kernel's cross-XCC work queue (crc32c_units.h): past the first
    row every group is claimed at run time from the per-XCC heads, the fast
    XCDs taking the slow ones' last groups.  Every block (the stealing tail
    and a partial last group included) matches the oracle, with the queue on
    and with the static interleave, and the two agree."""
    torch = torch_cuda
    from lsbm_amd import engine
    length, stride = 256, 272
    data = stream_bytes(0x51DE + n, 0, (n - 1) * stride + length)
    rng = np.random.default_rng(n)
    init = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32) if use_init else None
    d = _dev(torch, data)
    di = _dev(torch, init, torch.int32) if use_init else None
    want = oracle.batch_fixed(data, stride, length, n, init, masked)
    try:
        for on in (1, 0, 1):
            assert product_lib.lsbm_test_fixed_queue(on) == 0
            got = _u32(engine.crc32c_fixed(d, stride, length, n, init=di, masked=masked))
            assert np.array_equal(got, want), on
    finally:
        product_lib.lsbm_test_fixed_queue(-1)


@pytest.mark.parametrize("length,stride,n,shift", [
    (4118, 4118, 64, 0), (4117, 4123, 31, 0), (1, 1, 100, 0), (0, 16, 5, 0), (100, 100, 77, 0),
    (4096, 4096, 20, 3), (4096, 4100, 20, 0), (70000, 70001, 5, 1), (3, 5, 1000, 0),
])
def test_fixed_general_geometry(torch_cuda, oracle, length, stride, n, shift):
    torch = torch_cuda
    from lsbm_amd import engine
    nbytes = (n - 1) * stride + length + shift
    data = stream_bytes(777 + length, 0, nbytes)
    d = _dev(torch, data)[shift:]  # misaligned base
    got = _u32(engine.crc32c_fixed(d, stride, length, n))
    want = oracle.batch_fixed(data[shift:], stride, length, n)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- ragged
def _ragged_case(seed, n, max_len, gap_max=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n)
    lens[rng.random(n) < 0.05] = 0
    gaps = rng.integers(0, gap_max + 1, size=n) if gap_max else np.zeros(n, dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    pos = int(rng.integers(0, 16))
    for i in range(n):
        pos += int(gaps[i])
        offs[i] = pos
        pos += int(lens[i])
    offs[n] = pos
    # offsets array is [start_i] + end of last; with gaps the extents are
    # [offs[i], offs[i]+lens[i]) -- express them as a dense extent list instead
    starts = offs[:n]
    ends = starts + lens
    return starts, ends, pos


@pytest.mark.parametrize("seed,n,max_len", [(1, 1, 10), (2, 100, 300), (3, 1000, 5000),
                                            (4, 300, 70000), (5, 4096, 129), (6, 17, 4)])
@pytest.mark.parametrize("use_init,masked", [(False, False), (True, True)])
def test_ragged_dense(torch_cuda, oracle, seed, n, max_len, use_init, masked):
    torch = torch_cuda
    from lsbm_amd import engine
    starts, ends, total = _ragged_case(seed, n, max_len)
    offs = np.concatenate([starts, ends[-1:]]).astype(np.int64)
    data = stream_bytes(seed * 1000, 0, total + 64)
    rng = np.random.default_rng(seed)
    init = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32) if use_init else None
    got = _u32(engine.crc32c_batch(_dev(torch, data), _dev(torch, offs),
                                   init=_dev(torch, init, torch.int32) if use_init else None,
                                   masked=masked))
    want = oracle.batch_offsets(data, offs.astype(np.uint64), init, masked)
    assert np.array_equal(got, want)


def test_ragged_unsorted_overlapping_extents(torch_cuda, oracle):
    """offsets need not be monotone; extents may overlap or be empty (e < s -> empty)."""
    torch = torch_cuda
    from lsbm_amd import engine
    data = stream_bytes(4242, 0, 200000)
    rng = np.random.default_rng(9)
    offs = rng.integers(0, 200000, size=5001).astype(np.int64)
    got = _u32(engine.crc32c_batch(_dev(torch, data), _dev(torch, offs)))
    want = np.empty(5000, dtype=np.uint32)
    for i in range(5000):
        s, e = int(offs[i]), int(offs[i + 1])
        want[i] = oracle.value(data[s:max(s, e)].tobytes())
    assert np.array_equal(got, want)


def test_ragged_matches_fixed_on_same_blocks(torch_cuda):
    torch = torch_cuda
    from lsbm_amd import engine
    n, L = 4096, 4096
    d = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, 123)
    offs = torch.arange(0, (n + 1) * L, L, dtype=torch.int64, device="cuda")
    a = engine.crc32c_fixed(d, L, L, n)
    b = engine.crc32c_batch(d, offs)
    assert torch.equal(a, b)


def _skewed_offsets(seed, n, base=5):
    """Mostly 0-600-B blocks, 1% of 10-100 KB: equal block counts per wave
    would leave some waves with several times the mean bytes."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 600, size=n)
    big = rng.random(n) < 0.01
    lens[big] = rng.integers(10_000, 100_000, size=int(big.sum()))
    return (np.concatenate([[0], np.cumsum(lens)]) + base).astype(np.int64)


@pytest.mark.parametrize("kind", ["offsets", "extents", "verify"])
def test_ragged_byte_balanced_ranges_skewed(torch_cuda, oracle, kind):
    """>= 16 blocks per wave: general batches cut the waves' ranges by bytes
    (a 32-ary search over the block starts, crc32c_kernels.hip byte_ranges);
    every block is computed exactly once whatever the cut."""
    torch = torch_cuda
    from lsbm_amd import engine
    n = 300_000
    offs = _skewed_offsets(21, n)
    data = stream_bytes(21, 0, int(offs[-1]) + 64)
    want = oracle.batch_offsets(data, offs.astype(np.uint64), None, kind == "verify")
    d = _dev(torch, data)
    if kind == "offsets":
        got = _u32(engine.crc32c_batch(d, _dev(torch, offs)))
    elif kind == "extents":
        ext = np.stack([offs[:-1], offs[1:] - offs[:-1]], 1).reshape(-1)
        got = _u32(engine.crc32c_extents(d, _dev(torch, ext)))
    else:
        exp = want.copy()
        flip = np.random.default_rng(5).choice(n, size=97, replace=False)
        exp[flip] ^= 0x10
        ok, nbad = engine.crc32c_verify(d, _dev(torch, offs), _dev(torch, exp, torch.int32),
                                        masked=True)
        assert int(nbad.item()) == 97  # each block checked exactly once
        assert set(np.nonzero(ok.cpu().numpy() == 0)[0].tolist()) == set(flip.tolist())
        return
    assert np.array_equal(got, want)


_CHUNKED_N = 8 * 128 * 4096 + 12289  # kMinChunks x kChunkBlocks x 4,096 waves, and a partial


@functools.lru_cache(maxsize=1)
def _chunked_case():
    n = _CHUNKED_N
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 100, size=n)
    big = rng.random(n) < 0.0005
    lens[big] = rng.integers(10_000, 100_000, size=int(big.sum()))
    offs = (np.concatenate([[0], np.cumsum(lens)]) + 3).astype(np.int64)
    return lens, offs, stream_bytes(n, 0, int(offs[-1]) + 64)


@pytest.mark.parametrize("kind", ["offsets", "extents_shuffled", "verify"])
def test_ragged_chunked_sweep_exact(torch_cuda, oracle, kind):
    """General batches of >= 8 chunks of 128 blocks per wave are swept chunk
    by chunk, each chunk cut into byte-balanced ranges by range_bounds_kernel
    (crc32c_engine.cc run_ragged).  Blocks of 10-100 KB among 0-100-B ones
    span several ranges' worth of bytes, so some ranges are empty (a wave's
    first one included); with shuffled extents the starts are unsorted and the
    ranges merely unbalanced.  Every block computed once and right."""
    torch = torch_cuda
    from lsbm_amd import engine
    n = _CHUNKED_N
    lens, offs, data = _chunked_case()
    want = oracle.batch_offsets(data, offs.astype(np.uint64), None, kind == "verify")
    d = _dev(torch, data)
    rng = np.random.default_rng(7)
    if kind == "offsets":
        got = _u32(engine.crc32c_batch(d, _dev(torch, offs)))
    elif kind == "extents_shuffled":
        order = rng.permutation(n)
        ext = np.stack([offs[:-1][order], lens[order]], 1).reshape(-1).astype(np.int64)
        got = np.empty(n, dtype=np.uint32)
        got[order] = _u32(engine.crc32c_extents(d, _dev(torch, ext)))
    else:
        exp = want.copy()
        flip = rng.choice(n, size=131, replace=False)
        exp[flip] ^= 0x4
        ok, nbad = engine.crc32c_verify(d, _dev(torch, offs), _dev(torch, exp, torch.int32),
                                        masked=True)
        assert int(nbad.item()) == 131  # each block checked exactly once
        assert set(np.nonzero(ok.cpu().numpy() == 0)[0].tolist()) == set(flip.tolist())
        return
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mode", ["extents", "sst_crcs"])
def test_ragged_units_gigabytes_apart(torch_cuda, oracle, mode):
    """Consecutive blocks ~3 GiB apart: a round's units do not fit one 2 GiB
    buffer window, so the units kernel takes one window per pass (rows are
    loaded through bounded buffer descriptors, crc32c_kernels.hip)."""
    torch = torch_cuda
    from lsbm_amd import engine, table
    total = (3 << 30) + (40 << 20)
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, 606)
    rng = np.random.default_rng(31)
    n = 3000
    lens = rng.integers(0, 9000, size=n)
    starts = np.where(np.arange(n) % 3 == 1, 3 << 30, 7) + np.arange(n) * 251 * 40
    starts = starts + rng.integers(0, 64, size=n)
    ext = np.stack([starts, lens], 1).reshape(-1).astype(np.int64)
    try:
        if mode == "extents":
            want = np.array([oracle.value(stream_bytes(606, int(s), int(l)).tobytes())
                             for s, l in zip(starts, lens)], dtype=np.uint32)
            got = _u32(engine.crc32c_extents(d, _dev(torch, ext)))
        else:  # WriteRawBlock's crc of block || type, the type byte being the byte after the block
            types = rng.integers(0, 2, size=n).astype(np.uint8)
            want = np.array([oracle.mask(oracle.extend(oracle.value(stream_bytes(606, int(s), int(l)).tobytes()),
                                                       bytes([int(t)])))
                             for s, l, t in zip(starts, lens, types)], dtype=np.uint32)
            out, nbad = table.trailer_crcs(d, _dev(torch, ext), _dev(torch, types))
            assert int(nbad.item()) == 0
            got = _u32(out)
        assert np.array_equal(got, want)
    finally:
        del d
        torch.cuda.empty_cache()


@pytest.mark.parametrize("order", ["random", "descending"])
def test_ragged_unsorted_starts_tile_exactly(torch_cuda, oracle, order):
    """The byte cut on a batch whose starts are not sorted: the search is
    monotone in its target for any array, so the ranges still tile [0, n)
    (no block twice: verify's failure count is exact)."""
    torch = torch_cuda
    from lsbm_amd import engine
    n = 100_000
    rng = np.random.default_rng(17)
    if order == "random":  # starts jitter around a rising line: e < s (empty) in ~1/4
        offs = np.arange(n + 1, dtype=np.int64) * 30 + rng.integers(0, 400, size=n + 1)
    else:  # every block empty but the last; key(n) > key(0), the search runs over a reversed array
        offs = (n - np.arange(n + 1, dtype=np.int64)) * 30
        offs[n] = offs[0] + 1
    data = stream_bytes(17, 0, int(offs.max()) + 16)
    want = np.empty(n, dtype=np.uint32)
    for i in range(n):
        s, e = int(offs[i]), int(offs[i + 1])
        want[i] = oracle.value(data[s:max(s, e)].tobytes())
    exp = want.copy()
    flip = rng.choice(n, size=41, replace=False)
    exp[flip] ^= 1
    ok, nbad = engine.crc32c_verify(_dev(torch, data), _dev(torch, offs),
                                    _dev(torch, exp, torch.int32))
    assert int(nbad.item()) == 41
    assert set(np.nonzero(ok.cpu().numpy() == 0)[0].tolist()) == set(flip.tolist())


# ---------------------------------------------------------------- verify
def test_verify_detects_single_byte_flips(torch_cuda, oracle):
    torch = torch_cuda
    from lsbm_amd import engine
    starts, ends, total = _ragged_case(11, 2000, 6000)
    offs = np.concatenate([starts, ends[-1:]]).astype(np.int64)
    data = stream_bytes(11, 0, total + 16)
    expect = oracle.batch_offsets(data, offs.astype(np.uint64), masked=True)
    d = _dev(torch, data)
    do = _dev(torch, offs)
    ok, nbad = engine.crc32c_verify(d, do, _dev(torch, expect, torch.int32), masked=True)
    assert int(nbad.item()) == 0 and bool(ok.all())
    rng = np.random.default_rng(3)
    bad = set()
    for i in rng.choice(2000, size=50, replace=False):
        if ends[i] > starts[i]:
            pos = int(rng.integers(starts[i], ends[i]))
            d[pos] ^= 1 << int(rng.integers(0, 8))
            bad.add(int(i))
    ok, nbad = engine.crc32c_verify(d, do, _dev(torch, expect, torch.int32), masked=True)
    okh = ok.cpu().numpy()
    assert int(nbad.item()) == len(bad)
    assert set(np.nonzero(okh == 0)[0].tolist()) == bad


# ---------------------------------------------------------------- SSTable trailers
def test_sst_seal_matches_reference_trailers(torch_cuda, golden):
    torch = torch_cuda
    from lsbm_amd import table
    blocks = golden["sst_blocks"]
    handles, total = table.layout_blocks([b["len"] for b in blocks])
    img = np.zeros(total, dtype=np.uint8)
    for i, b in enumerate(blocks):
        off = handles[2 * i]
        img[off:off + b["len"]] = printable_bytes(b["seed"], b["len"])
    d = _dev(torch, img)
    dh = _dev(torch, handles.astype(np.int64))
    types = _dev(torch, np.array([b["type"] for b in blocks], dtype=np.uint8))
    table.seal_blocks(d, dh, types)
    out = d.cpu().numpy()
    for i, b in enumerate(blocks):
        t0 = handles[2 * i] + b["len"]
        assert out[t0:t0 + 5].tobytes().hex() == b["trailer_hex"], i
    st, ok = table.verify_status(d, dh)
    assert st.ok() and bool(ok.all())
    # ReadBlock: a flipped payload byte or type byte -> Corruption
    d[int(handles[2 * 5]) + 100] ^= 0x20
    d[int(handles[2 * 9] + blocks[9]["len"])] ^= 0x01  # the type byte
    st, ok = table.verify_status(d, dh)
    assert st.IsCorruption() and st.ToString() == "Corruption: block checksum mismatch"
    assert set(np.nonzero(ok.cpu().numpy() == 0)[0].tolist()) == {5, 9}


def test_sst_random_layout_roundtrip(torch_cuda, oracle):
    torch = torch_cuda
    from lsbm_amd import table
    rng = np.random.default_rng(21)
    sizes = rng.integers(0, 9000, size=3000)
    handles, total = table.layout_blocks(sizes)
    img = stream_bytes(21, 0, total)
    types = rng.integers(0, 2, size=3000).astype(np.uint8)
    d = _dev(torch, img)
    dh = _dev(torch, handles.astype(np.int64))
    table.seal_blocks(d, dh, _dev(torch, types))
    out = d.cpu().numpy()
    for i in rng.choice(3000, size=200, replace=False):
        off, n = int(handles[2 * i]), int(sizes[i])
        crc = oracle.extend(oracle.value(out[off:off + n].tobytes()), bytes([types[i]]))
        assert out[off + n] == types[i]
        assert int.from_bytes(out[off + n + 1:off + n + 5].tobytes(), "little") == oracle.mask(crc)
    ok, nbad = table.verify_blocks(d, dh)
    assert int(nbad.item()) == 0


# ---------------------------------------------------------------- host-staged
def test_host_staged_batch(torch_cuda, oracle):
    from lsbm_amd import engine
    starts, ends, total = _ragged_case(31, 20000, 12000)
    offs = np.concatenate([starts, ends[-1:]]).astype(np.uint64)
    data = stream_bytes(31, 0, total)
    init = np.random.default_rng(0).integers(0, 2**32, size=20000,
                                              dtype=np.uint64).astype(np.uint32)
    got = engine.crc32c_batch_host(data, offs, init=init, masked=True)
    want = oracle.batch_offsets(data, offs, init, masked=True)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- generator
def test_fill_splitmix64_matches_numpy(torch_cuda):
    torch = torch_cuda
    from lsbm_amd import engine
    for n, seed in [(1 << 20, 0x5EED0000), (1000003, 77)]:
        d = torch.empty(n, dtype=torch.uint8, device="cuda")
        engine.fill_splitmix64(d, seed)
        assert np.array_equal(d.cpu().numpy(), stream_bytes(seed, 0, n))


# ---------------------------------------------------------------- full-size configs
from golden.xorfold import xor_fold_rows  # noqa: E402


def crc_linearity_holds(oracle, d, crc, L, n):
    """Every one of the n CRCs checked at once, at full size: for blocks of one
    length L, Value(b) = raw(b) ^ Value(0^L) with raw linear over GF(2), so the
    XOR of all n CRCs equals Value(XOR of all n blocks), ^ Value(0^L) when n is
    even.  One 4-byte compare against the oracle over the XOR-folded block
    (folded on the device) covers every block of the batch."""
    import torch
    xb = xor_fold_rows(d[:n * L].view(torch.int64).view(n, L // 8)).cpu().numpy().view(np.uint8)
    xc = int(xor_fold_rows(crc[:n].view(torch.int32).view(n, 1)).cpu().numpy().view(np.uint32)[0])
    want = oracle.value(xb.tobytes()) ^ (oracle.value(bytes(L)) if n % 2 == 0 else 0)
    return xc == want


def _config_fixed(torch, oracle, golden, name, seed, L, n, check_ragged_blocks):
    from lsbm_amd import engine
    d = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, seed)
    crc = engine.crc32c_fixed(d, L, L, n)
    got = _u32(crc)
    for g in golden["config_blocks"]:
        if g["config"] == name:
            assert got[g["block"]] == g["value"], g
    rng = np.random.default_rng(seed)
    for b in rng.choice(n, size=256, replace=False):
        assert got[b] == oracle.value(stream_bytes(seed, int(b) * L, L).tobytes()), b
    # an independent kernel (ragged path, aligned frame, A^-z tail fix) agrees
    m = min(n, check_ragged_blocks)
    offs = torch.arange(0, (m + 1) * L, L, dtype=torch.int64, device="cuda")
    other = engine.crc32c_batch(d, offs)
    assert torch.equal(other, crc[:m])
    del other, offs
    # all n CRCs at once, against the oracle, by linearity
    assert crc_linearity_holds(oracle, d, crc, L, n)
    crc[n // 3] ^= 1  # (and the check sees a single wrong CRC)
    assert not crc_linearity_holds(oracle, d, crc, L, n)
    del d, crc
    torch.cuda.empty_cache()


def test_config2_full_1M_x_4KiB(torch_cuda, oracle, golden):
    _config_fixed(torch_cuda, oracle, golden, "cfg2_4k", 0x5EED0000, 4096, 1 << 20, 1 << 20)


def test_config3_full_1M_x_64KiB(torch_cuda, oracle, golden):
    _config_fixed(torch_cuda, oracle, golden, "cfg3_64k", 0x5EED0001, 65536, 1 << 20, 1 << 16)


def test_config5_all_eight_shards(torch_cuda, oracle, golden):
    """Config 5 (BASELINE.json configs[4]): 80M x 4 KiB over 8 ranks, rank r
    holding global blocks [10M r, 10M (r + 1)).  The 8-GPU bench is the
    driver's, so here every shard runs in turn on the one GPU through bench.py's
    own shard code (the fill from word 512 lo, lsbm_crc32c_fixed_dev over 10M
    blocks): the reference's CRCs either side of every shard boundary
    (golden cfg5_shards, from the reference's Extend), 64 sampled blocks per
    shard against the oracle by global index, and all 10M CRCs of every shard
    by linearity -- every one of the 80M CRCs is covered."""
    torch = torch_cuda
    from lsbm_amd import engine
    n, L, seed = 10_000_000, 4096, 0x5EED0000
    want = {g["block"]: g["value"] for g in golden["config_blocks"] if g["config"] == "cfg5_shards"}
    assert len(want) == 15
    d = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    crc = torch.empty(n, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(5)
    seen = 0
    for r in range(8):
        lo = r * n
        engine.fill_splitmix64(d, seed + lo * (L // 8))  # (bench.py main: the same expression)
        engine.crc32c_fixed(d, L, L, n, out=crc)
        got = _u32(crc)
        for b, v in want.items():
            if lo <= b < lo + n:
                assert got[b - lo] == v, (r, b)
                seen += 1
        for i in rng.choice(n, size=64, replace=False):
            assert got[i] == oracle.value(stream_bytes(seed, (lo + int(i)) * L, L).tobytes()), (r, int(i))
        assert crc_linearity_holds(oracle, d, crc, L, n), r
    assert seen == 15
    del d, crc
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- C++ host layer
@pytest.mark.parametrize("small,auto_lock", [("", "1"), ("", "0"), ("zc", "1")],
                         ids=["small-dma-auto-lock", "staged", "small-zero-copy"])
def test_cpp_table_layer_seal_verify(torch_cuda, tmp_path, small, auto_lock):
    """include/lsbm/table_checksum.h used from C++ the way table/ would: small
    jobs with pageable images page-locked per call (default) or staged
    (LSBM_AUTO_LOCK=0), page-locked ones DMA-ed whole or read in place
    (LSBM_SMALL_LOCKED=zc); a read-only mmap of a table file verified."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "table_gpu_test"
    libdir = os.path.join(repo, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(repo, "include"), "-I", "/opt/rocm/include",
                    os.path.join(repo, "tests", "cpp", "table_gpu_test.cc"), "-L", libdir,
                    "-llsbm_crc32c", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["LSBM_AUTO_LOCK"] = auto_lock
    if small:
        env["LSBM_SMALL_LOCKED"] = small
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK")


@pytest.mark.parametrize("pinned,zero_copy_mb,small,auto_lock",
                         [(0, 64, "", "0"), (0, 64, "", "1"), (1, 64, "", "1"), (1, 64, "zc", "1"), (1, 0, "", "1")],
                         ids=["pageable-staged", "pageable-auto-locked", "locked-small-dma", "locked-small-zero-copy",
                              "locked-chunks"])
def test_cpp_concurrent_table_callers(torch_cuda, tmp_path, pinned, zero_copy_mb, small, auto_lock):
    """4 threads each sealing their own 16 MiB table, one table per call
    (tests/cpp/concurrent_seal_test.cc): trailers byte-identical to the same
    calls made one after another and to util/crc32c.h's WriteRawBlock pattern,
    concurrent verify finds every block good and exactly one flipped block
    per table, and the concurrent calls take measurably less wall time (each
    caller leases its own session of the device) -- staged pageable images
    (LSBM_AUTO_LOCK=0), where one caller's host copy leaves PCIe idle part of
    the time.  Page-locked images, and pageable ones page-locked for the call
    (the default for small jobs), are DMA-ed in place (each table whole, or, small=zc, read by the kernel
    in place; or, zero_copy_mb=0, in chunks through the pipeline): one caller
    alone already runs near the PCIe ceiling (profiles/r04/), so there
    concurrency must only not cost anything."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "concurrent_seal_test"
    libdir = os.path.join(repo, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(repo, "include"), "-I", "/opt/rocm/include",
                    os.path.join(repo, "tests", "cpp", "concurrent_seal_test.cc"), "-L", libdir,
                    "-llsbm_crc32c", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["LSBM_AUTO_LOCK"] = auto_lock
    if small:
        env["LSBM_SMALL_LOCKED"] = small
    r = subprocess.run([str(exe), "4", "8", str(pinned), str(zero_copy_mb)], capture_output=True, text=True,
                       timeout=120, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
    speedup = float(r.stdout.split("speedup=")[1].split()[0])
    # (page-locked: 1.05-1.18 once the registrations of disjoint images ran in
    # parallel, profiles/r05/lock_parallel/; 0.80 while they were serialised)
    assert speedup >= (1.1 if pinned == 0 and auto_lock == "0" else 0.9), r.stdout


@pytest.mark.parametrize("auto_lock", ["1", "0"], ids=["auto-lock", "staged"])
def test_cpp_concurrent_callers_on_shared_pages(torch_cuda, oracle, tmp_path, auto_lock):
    """8 threads seal and verify (writable char*, page-locked per call) small
    pageable table images packed back to back in ONE allocation, so that
    neighbours share pages, over 6 rounds of shuffled call orders
    (tests/cpp/shared_page_seal_test.cc): every trailer equals the oracle's
    WriteRawBlock trailer and nothing else changed, every verify passes and a
    flipped byte fails exactly its block, no per-call lock outlives its call,
    and later serial and whole-batch calls on the same memory still succeed
    (the per-call locks' check -> register -> unregister
    is serialised against every other call's locks)."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "shared_page_seal_test"
    libdir = os.path.join(repo, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(repo, "include"), "-I", "/opt/rocm/include",
                    os.path.join(repo, "tests", "cpp", "shared_page_seal_test.cc"), "-L", libdir,
                    "-llsbm_crc32c", "-L", "/opt/rocm/lib", "-lamdhip64", "-ldl",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    env = dict(os.environ, LSBM_AUTO_LOCK=auto_lock)
    r = subprocess.run([str(exe), os.path.join(repo, "oracle", "liboracle_crc32c.so"), "8", "192", "6"],
                       capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
    fields = dict(kv.split("=") for kv in r.stdout.split()[1:])
    assert int(fields["shared_pages"]) > 100
    assert int(fields["pooled"]) > 0  # (lsbm_host_register'd images beside their neighbours' calls)
    if auto_lock == "1":
        assert int(fields["locked_calls"]) > 0  # (some calls did lock their pages)
    else:
        assert int(fields["locked_calls"]) == 0


def test_cpp_pinned_staging_stays_within_the_budget(torch_cuda, tmp_path):
    """a device's sessions (up to 8, 4 stages each) used to keep
    their page-locked staging until shutdown.  With LSBM_PINNED_MB=8 and every
    call staged (LSBM_AUTO_LOCK=0), 6 concurrent callers' sessions grow their
    buffers, and once the leases are released the pinned bytes are back under
    the budget plus the last session's; later calls grow them again and stay
    correct; shutdown frees everything (tests/cpp/pinned_budget_test.cc)."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "pinned_budget_test"
    libdir = os.path.join(repo, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(repo, "include"), "-I", "/opt/rocm/include",
                    os.path.join(repo, "tests", "cpp", "pinned_budget_test.cc"), "-L", libdir,
                    "-llsbm_crc32c", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    env = dict(os.environ, LSBM_PINNED_MB="8", LSBM_AUTO_LOCK="0")
    r = subprocess.run([str(exe), "6"], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.strip().splitlines()[-1].startswith("OK"), r.stdout


def test_level2_binding_over_the_reference_table_code(torch_cuda):
    """integration/leveldb_gpu_checksum.h, linked with the reference's own
    table/ and util/ objects (oracle/Makefile gpubind, built in the build
    container): GPU-sealed trailers equal WriteRawBlock's, the reference's
    ReadBlock accepts every block, and VerifyBlocksOnGpu fails a flipped byte
    with ReadBlock's status.  Skipped where the binary was not built."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                       "gpu_binding")
    if not os.access(exe, os.X_OK):
        pytest.skip("oracle/_ref/gpu_binding not built (needs /root/reference at build time)")
    from test_ref_link import ref_env
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=ref_env())
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout


def test_gpu_sealed_table_builder_matches_the_reference_table_builder(torch_cuda):
    """integration/gpu_table_builder.h over the reference's own BlockBuilder,
    FilterBlockBuilder, BlockHandle / Footer and comparators (oracle/Makefile
    gputable, built in the build container): compaction-shaped internal-key
    streams (db_bench user keys, 100-B values) cut into 16 MiB tables with a
    bloom filter, lsbm's default 8 MiB with none, 16 KiB blocks with snappy
    requested, a 37-entry and an empty table.  Each table's trailers are
    reserved and sealed by ONE SealBlocks call at Finish (page-locked in place),
    and the file is byte-identical to the unmodified TableBuilder's (whose
    trailers come from the reference's own util/crc32c.cc, block by block); the
    reference's Table::Open / ReadBlock with verify_checksums reads every entry
    back.  Then the read side (integration/gpu_table_reader.h): the reference's
    Table::Open + iteration with verify_checksums against OpenVerifiedTable
    (the file read once, ONE VerifyBlocks call over its data blocks, iteration
    from memory): the same entries, the same status for a flipped data-block
    byte, and neither checks the filter block.  Last, the device made to fail
    (lsbm_test_fail_host_pipeline) under Finish and under OpenVerifiedTable:
    the builder still returns OK with a byte-identical file (its trailers
    computed on the CPU, integration/gpu_fallback.h) and the reader returns
    the reference's statuses.  Skipped where the binary was not built."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                       "gpu_table_builder")
    if not os.access(exe, os.X_OK):
        pytest.skip("oracle/_ref/gpu_table_builder not built (needs /root/reference at build time)")
    from test_ref_link import ref_env
    r = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=300, env=ref_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.strip().splitlines()[-1].startswith("OK"), r.stdout
    assert r.stdout.count("identical=1") == 3 + 3 + 3 + 1 + 1 + 1
    # a device that cannot seal or verify: the CPU fallback, same bytes, same statuses
    assert "device failure:" in r.stdout and "injected fault" in r.stdout


def test_compaction_end_to_end_with_both_gpu_ends_matches_the_reference(torch_cuda):
    """One compaction as DoCompactionWork runs it with paranoid_checks
    (tests/cpp/ref_compaction_gpu.cc, oracle/Makefile gpucompact): 4 overlapping
    16 MiB input tables merged by the reference's MergingIterator into 16 MiB
    output tables.  The reference's way (verified input iterators, TableBuilder)
    and with the two GPU ends (OpenVerifiedTable inputs: one VerifyBlocks per
    input; GpuTableBuilder outputs: one SealBlocks per output) write
    byte-identical output tables, three rounds.  Skipped where the binary was
    not built."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                       "gpu_compaction")
    if not os.access(exe, os.X_OK):
        pytest.skip("oracle/_ref/gpu_compaction not built (needs /root/reference at build time)")
    from test_ref_link import ref_env
    r = subprocess.run([exe, "4", "16", "16"], capture_output=True, text=True, timeout=300, env=ref_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("OK") and "FAIL" not in r.stdout, r.stdout
    f = dict(kv.split("=") for kv in last.split()[1:])
    assert int(f["outputs"]) >= 4 and f["identical"] == f["outputs"]
    assert int(f["input_blocks_verified"]) > 16000


def test_db_bench_gpu_tables(torch_cuda, tmp_path):
    """Config 1 end to end (BASELINE.json configs[0]):
    lsbm's own db_bench, 1M writes, as shipped and as the Level-2 build
    (oracle/Makefile dbbench_gpu: the same sources with
    integration/table_builder_gpu.cc in place of table/table_builder.o and
    Extend / Hash from liblsbm_crc32c.so), so every table lsbm's memtable
    flushes and compactions write is sealed by one SealBlocks call on the GPU.
    The reference-only checker (tests/cpp/db_verify.cc) reads every block of
    every finished table and every WAL / MANIFEST record of the GPU-written
    database with the reference's own CRC code, and opening it with
    paranoid_checks gives the same content digest as the reference's database.
    Finished tables that both runs wrote are byte-identical.  Skipped where the
    binaries were not built."""
    import hashlib
    import os
    import subprocess
    from test_ref_link import db_bench_args, db_verify, ref_env
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
    if not all(os.access(os.path.join(ref, x), os.X_OK) for x in ("db_bench", "db_bench_gpu", "db_verify")):
        pytest.skip("oracle/_ref/db_bench* not built (needs /root/reference at build time)")
    runs = {}
    for name in ("db_bench", "db_bench_gpu"):
        db = tmp_path / name
        db.mkdir()
        env = ref_env(LSBM_TABLE_STATS="1")
        r = subprocess.run([os.path.join(ref, name)] + db_bench_args(str(db), 1_000_000),
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("separate")]
        rc, v = db_verify(os.path.join(ref, "db_verify"), str(db))
        assert rc == 0 and v["table_errors"] == 0 and v["log_errors"] == 0 and v["tables"] >= 8, v
        rc, o = db_verify(os.path.join(ref, "db_verify"), str(db), str(tmp_path / (name + "_open")))
        assert rc == 0 and o["open_error"] == "", o
        stats = [ln for ln in r.stderr.splitlines() if ln.startswith("lsbm_table_stats")]
        hashes = {}
        for f in sorted(os.listdir(db)):
            if f.endswith(".ldb"):
                b = (db / f).read_bytes()
                if len(b) >= 48 and b[-8:] == bytes.fromhex("57fb808b247547db"):  # a finished table
                    hashes.setdefault(hashlib.sha256(b).hexdigest(), []).append(f)
        runs[name] = dict(line=line, verify=v, digest=(o["live"], o["digest"]), stats=stats, hashes=hashes)
        print(name, line, v, o["live"], o["digest"], stats)
    assert runs["db_bench_gpu"]["digest"] == runs["db_bench"]["digest"]
    # the GPU build sealed its tables on the GPU, the reference build has no such code
    st = runs["db_bench_gpu"]["stats"]
    assert st and int(st[0].split("tables_sealed_on_gpu=")[1].split()[0]) >= runs["db_bench_gpu"]["verify"]["tables"]
    assert not runs["db_bench"]["stats"]
    common = set(runs["db_bench"]["hashes"]) & set(runs["db_bench_gpu"]["hashes"])
    print("finished tables byte-identical in both runs:", len(common), "of", len(runs["db_bench_gpu"]["hashes"]))
    assert len(common) >= 1


def test_db_check_gpu_matches_the_reference_on_a_db_bench_database(torch_cuda, tmp_path):
    """A whole lsbm database, written by the reference's own db_bench (config
    1, 1M writes), checked two ways: tools/db_check_gpu.cc (this repo's layers
    only: every table's blocks in ONE VerifyTables call, each log through
    BatchReader) and oracle/_ref/db_verify (the reference's ReadBlock and
    log::Reader with its own CRC code).  Clean, both find nothing; then with
    bytes flipped in data blocks of three tables and in the WAL, both list the
    SAME failing blocks (file:offset) and the same reporter calls and dropped
    bytes, with the tables mapped read-only (staged) and read into heap
    buffers (page-locked in place).  On the clean database, every table's
    filter block is also rebuilt on the GPU from its keys (byte-identical) and
    every key probed in it (no false negatives).  Skipped where the reference binaries were
    not built."""
    import os
    import shutil
    import subprocess
    from test_ref_link import db_bench_args, db_check_gpu, db_verify
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
    if not all(os.access(os.path.join(ref, x), os.X_OK) for x in ("db_bench", "db_verify")):
        pytest.skip("oracle/_ref/db_bench, db_verify not built (needs /root/reference at build time)")
    db = tmp_path / "db"
    db.mkdir()
    r = subprocess.run([os.path.join(ref, "db_bench")] + db_bench_args(str(db), 1_000_000),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rc, v = db_verify(os.path.join(ref, "db_verify"), str(db))
    g = db_check_gpu(str(db), "0", tmp_path, "--filters")
    print("clean", v, g)
    assert rc == 0 and v["bad_blocks"] == [] and g["bad_blocks"] == []
    assert (g["tables"], g["blocks"], g["records"]) == (v["tables"], v["blocks"], v["records"])
    assert g["log_corruptions"] == v["log_errors"] == 0
    # every table's filter block rebuilt on the GPU from its own keys: byte-identical,
    # and no key of the table is ever filtered out
    assert g["filters_rebuilt"] == g["filters_identical"] == g["tables"] and g["filter_tables_skipped"] == 0, g
    assert g["keys_probed"] == v["entries"] and g["false_negatives"] == 0, g
    # corrupt a copy: one byte in the data region of three finished tables
    # (inside some data block or its trailer), one in the middle of the WAL
    bad = tmp_path / "bad"
    shutil.copytree(db, bad)
    finished = sorted(f for f in os.listdir(bad) if f.endswith(".ldb") and os.path.getsize(bad / f) > (1 << 20)
                      and (bad / f).read_bytes()[-8:] == bytes.fromhex("57fb808b247547db"))
    assert len(finished) >= 3
    for k, f in enumerate(finished[:3]):
        b = bytearray((bad / f).read_bytes())
        for at in (4096 * (k + 1) + 7, len(b) // 3 + 1000 * k):
            b[at] ^= 0x10
        (bad / f).write_bytes(bytes(b))
    logs = [f for f in os.listdir(bad) if f.endswith(".log") and os.path.getsize(bad / f) > 100_000]
    assert logs
    b = bytearray((bad / logs[0]).read_bytes())
    b[len(b) // 2] ^= 0x01
    (bad / logs[0]).write_bytes(bytes(b))
    rc, v = db_verify(os.path.join(ref, "db_verify"), str(bad))
    assert len(v["bad_blocks"]) == 6, v
    for read in ("mmap", "heap"):  # (read-only mappings staged; heap images page-locked in place)
        g = db_check_gpu(str(bad), "0", tmp_path, *(["--read=heap"] if read == "heap" else []))
        print("corrupted", read, v, g)
        assert sorted(g["bad_blocks"]) == sorted(v["bad_blocks"])
        assert g["log_corruptions"] == v["log_errors"] >= 1
        assert g["dropped_bytes"] == v["dropped_bytes"] and g["records"] == v["records"]


def test_cpp_block_compression_layer(torch_cuda, tmp_path):
    """include/lsbm/block_compression.h from C++: WriteBlock's compression and
    12.5% rule against the snappy oracle, ReadBlock's decompression and its
    Corruption statuses, then SealBlocks / VerifyBlocks over the result."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "compression_gpu_test"
    libdir = os.path.join(repo, "lsbm_amd")
    odir = os.path.join(repo, "oracle")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(repo, "include"),
                    os.path.join(repo, "tests", "cpp", "compression_gpu_test.cc"), "-L", libdir,
                    "-llsbm_crc32c", "-L", odir, "-loracle_snappy",
                    "-Wl,-rpath," + libdir + ":" + odir, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK")


def test_host_staged_pinned_source_and_chunking(torch_cuda, oracle):
    """A page-locked source is DMA-ed directly (no gather); > 64 MiB spans chunks."""
    torch = torch_cuda
    from lsbm_amd import engine
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 70000, size=3000)
    offs = np.zeros(3001, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    total = int(offs[-1])
    src = torch.empty(total + 7, dtype=torch.uint8, pin_memory=True)
    h = src.numpy()
    h[:] = stream_bytes(78, 0, total + 7)
    view = h[7:]  # odd start inside the pinned allocation
    got = engine.crc32c_batch_host(view, offs, masked=True)
    want = oracle.batch_offsets(view, offs, masked=True)
    assert np.array_equal(got, want)


def test_fixed_batch_replays_in_a_hip_graph(torch_cuda, oracle):
    """lsbm_crc32c_fixed_dev only enqueues (no alloc / sync), so it can be
    captured into a graph (torch.cuda.CUDAGraph = hipGraph) and replayed."""
    torch = torch_cuda
    from lsbm_amd import engine
    n, L = 4096, 4096
    d = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, 0xABC)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.crc32c_fixed(d, L, L, n, out=out, stream=torch.cuda.current_stream())
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    want = oracle.batch_fixed(stream_bytes(0xABC, 0, n * L), L, L, n)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    engine.fill_splitmix64(d, 0xABD)  # new bytes, same graph
    g.replay()
    torch.cuda.synchronize()
    want2 = oracle.batch_fixed(stream_bytes(0xABD, 0, n * L), L, L, n)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want2)


# ---------------------------------------------------------------- ragged path extras
def test_ragged_huge_blocks_and_carries(torch_cuda, oracle):
    """Blocks of 0 B .. 3 MiB mixed, so that a block's units span many rounds
    (in-wave carries) and unit shifts exceed the 512-row column tables."""
    torch = torch_cuda
    from lsbm_amd import engine
    rng = np.random.default_rng(101)
    lens = np.concatenate([rng.integers(0, 300, 40), [3 << 20, 0, 1, 200000, 65536, 65537],
                           rng.integers(0, 9000, 60), [1 << 20, 129, 128, 127]])
    rng.shuffle(lens)
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    offs += 3
    data = stream_bytes(101, 0, int(offs[-1]) + 16)
    init = rng.integers(0, 2**32, size=lens.size, dtype=np.uint64).astype(np.uint32)
    for use_init in (False, True):
        got = _u32(engine.crc32c_batch(_dev(torch, data), _dev(torch, offs),
                                       init=_dev(torch, init, torch.int32) if use_init else None))
        want = oracle.batch_offsets(data, offs.astype(np.uint64), init if use_init else None)
        assert np.array_equal(got, want)


def test_ragged_batch_replays_in_a_hip_graph(torch_cuda, oracle):
    """The ragged path is one launch with no allocation, so it is capturable."""
    torch = torch_cuda
    from lsbm_amd import engine
    starts, ends, total = _ragged_case(55, 3000, 9000)
    offs = _dev(torch, np.concatenate([starts, ends[-1:]]).astype(np.int64))
    d = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, 0xAB0)
    out = torch.zeros(3000, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.crc32c_batch(d, offs, out=out, masked=True, stream=torch.cuda.current_stream())
    for seed in (0xAB0, 0xAB1):
        engine.fill_splitmix64(d, seed)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = oracle.batch_offsets(stream_bytes(seed, 0, total + 16),
                                    offs.cpu().numpy().astype(np.uint64), masked=True)
        assert np.array_equal(_u32(out), want)


def test_two_pass_seal_and_chunked_batch_replay_in_a_hip_graph(torch_cuda, oracle):
    """Under hipGraph capture the entry points that take stream-ordered scratch
    when they run eagerly do without it: lsbm_sst_seal_dev at >= 131072 blocks
    (two passes eagerly, the one-pass seal under capture) and a >= 4.2M-block
    lsbm_crc32c_batch_dev (the chunked sweep's bounds eagerly, one range per
    wave under capture).  Both captured, replayed over new bytes, checked
    against the oracle (table/table_builder.cc:245-249, util/crc32c.cc:286-329)."""
    torch = torch_cuda
    from lsbm_amd import engine, table
    rng = np.random.default_rng(0x6A)
    # -- the seal: 140K blocks of 0..900 B
    sizes = rng.integers(0, 900, size=140_000)
    handles, total = table.layout_blocks(sizes)
    dh = _dev(torch, handles.astype(np.int64))
    types = rng.integers(0, 2, size=sizes.size).astype(np.uint8)
    dt = _dev(torch, types)
    img = torch.empty(total, dtype=torch.uint8, device="cuda")
    nbad = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        table.seal_blocks(img, dh, dt, stream=torch.cuda.current_stream(), nbad=nbad)
    off, sz = handles[0::2], handles[1::2]
    for seed in (0x6A0, 0x6A1):
        engine.fill_splitmix64(img, seed)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = img.cpu().numpy()
        src = stream_bytes(seed, 0, total)
        # payloads untouched, every trailer the reference's
        pick = np.concatenate([np.arange(64), rng.choice(sizes.size, 3000, replace=False),
                               np.arange(sizes.size - 64, sizes.size)])
        for i in pick:
            o, n = int(off[i]), int(sz[i])
            assert np.array_equal(got[o:o + n], src[o:o + n])
            crc = oracle.mask(oracle.extend(oracle.value(src[o:o + n].tobytes()), bytes([types[i]])))
            assert got[o + n] == types[i] and int.from_bytes(got[o + n + 1:o + n + 5].tobytes(), "little") == crc, i
        ok, nb = table.verify_blocks(img, dh)
        assert bool(ok.all().item()) and int(nb.item()) == 0 and int(nbad.item()) == 0
    # -- the chunked sweep's batch size: 4.5M blocks of 0..120 B
    n = 4_500_000
    lens = rng.integers(0, 121, size=n)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    offs += 1
    d = torch.empty(int(offs[-1]) + 16, dtype=torch.uint8, device="cuda")
    do = _dev(torch, offs)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        engine.crc32c_batch(d, do, out=out, stream=torch.cuda.current_stream())
    for seed in (0x6B0, 0x6B1):
        engine.fill_splitmix64(d, seed)
        out.zero_()
        g2.replay()
        torch.cuda.synchronize()
        want = oracle.batch_offsets(stream_bytes(seed, 0, d.numel()), offs.astype(np.uint64))
        assert np.array_equal(_u32(out), want)


# ---------------------------------------------------------------- config 4 (full size)
def device_windows(torch, d, starts, ends, cap=4 << 30):
    """Walk a device image's sorted blocks [starts[i], ends[i]) in windows of
    <= cap bytes: yields (b0, b1, window, base_off), window = image bytes
    [base_off, base_off + size) on the host holding blocks b0..b1-1 whole.  Two
    pinned buffers: window k + 1 is copied while the caller checks window k."""
    n = starts.size
    spans, b0 = [], 0
    while b0 < n:
        b1 = int(np.searchsorted(ends, int(starts[b0]) + cap, side="right"))
        assert b1 > b0
        spans.append((b0, b1, int(starts[b0]), int(ends[b1 - 1]) - int(starts[b0])))
        b0 = b1
    torch.cuda.synchronize()
    cap = max(m for _, _, _, m in spans) if spans else 0
    bufs = [torch.empty(max(cap, 1), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    cs = torch.cuda.Stream()
    evs = [None, None]

    def issue(k):
        _, _, a, m = spans[k]
        with torch.cuda.stream(cs):
            bufs[k % 2][:m].copy_(d[a:a + m], non_blocking=True)
            evs[k % 2] = torch.cuda.Event()
            evs[k % 2].record(cs)

    if spans:
        issue(0)
    for k, (b0, b1, a, m) in enumerate(spans):
        if k + 1 < len(spans):
            issue(k + 1)  # (its buffer's previous window has been checked)
        evs[k % 2].synchronize()
        yield b0, b1, bufs[k % 2].numpy()[:m], a
    del bufs


def oracle_over_device_windows(torch, oracle, d, offs):
    """The oracle's CRC of every block [offs[i], offs[i+1]) of device image d."""
    n = offs.size - 1
    want = np.empty(n, dtype=np.uint32)
    for b0, b1, win, a in device_windows(torch, d, offs[:-1], offs[1:]):
        want[b0:b1] = oracle.batch_offsets_mt(win, a, offs[b0:b1 + 1])
    return want


def test_oracle_window_walk_small(torch_cuda, oracle):
    """device_windows / oracle_batch_offsets_mt themselves: tiny windows over a
    ragged image give the scalar oracle's CRCs (blocks of 0 B included)."""
    torch = torch_cuda
    from lsbm_amd import engine
    rng = np.random.default_rng(41)
    lens = rng.integers(0, 3000, 5000)
    lens[::97] = 0
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    offs += 3
    d = torch.empty(int(offs[-1]) + 16, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, 0x51D0)
    want = np.empty(lens.size, dtype=np.uint32)
    for b0, b1, win, a in device_windows(torch, d, offs[:-1], offs[1:], cap=40_000):
        assert win.size <= 40_000
        want[b0:b1] = oracle.batch_offsets_mt(win, a, offs[b0:b1 + 1])
    assert np.array_equal(want, oracle.batch_offsets(d.cpu().numpy(), offs.astype(np.uint64)))
    assert np.array_equal(want, _u32(engine.crc32c_batch(d, _dev(torch, offs))))


def test_config4_full_10M_zipf(torch_cuda, oracle):
    """BASELINE.json configs[3]: 10M blocks, n = min(65536, 512 r + u), r ~ Zipf(0.99),
    densely packed from an odd start (117 GiB: extents cross 4 GiB multiples and
    2^36).  Every one of the 10M CRCs is checked against the oracle: the image
    comes back to the host in windows of <= 4 GiB (double-buffered pinned
    copies) and oracle_batch_offsets_mt recomputes the blocks lying wholly in
    each window, the blocks that straddle a window's end going with the next.
    The blocks crossing 4 GiB multiples and 2^36 are asserted to exist, and
    verify mode runs over the whole batch against the computed CRCs."""
    torch = torch_cuda
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "tools"))
    from bench_configs import zipf_lengths
    from lsbm_amd import engine
    n, seed, pad = 10_000_000, 0x5EED0003, 5
    lens = zipf_lengths(n)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    offs += pad
    total = int(offs[-1]) + 16
    assert total > (1 << 36)
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, seed)
    do = _dev(torch, offs)
    crc = engine.crc32c_batch(d, do)
    got = _u32(crc)
    cross = np.nonzero((offs[:-1] >> 32) != ((offs[1:] - 1) >> 32))[0]
    cross36 = np.nonzero((offs[:-1] >> 36) != ((offs[1:] - 1) >> 36))[0]
    assert cross.size >= 20 and cross36.size >= 1
    # a few blocks by the scalar oracle over regenerated bytes (independent of
    # the device fill and of the window copies below)
    for b in np.concatenate([cross36, [0, n - 1]]):
        blk = stream_bytes(seed, int(offs[b]), int(lens[b])).tobytes()
        assert got[b] == oracle.value(blk), int(b)
    want = oracle_over_device_windows(torch, oracle, d, offs)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    ok, nbad = engine.crc32c_verify(d, do, crc)
    assert int(nbad.item()) == 0 and bool(ok.all())
    del d, do, crc, ok
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- SSTable at real scale
def test_sst_1M_x_4118_seal_verify_roundtrip(torch_cuda, oracle):
    """1M real-size data blocks (4,118 B) laid out as a file image
    with trailers: lsbm_sst_seal_dev writes every trailer, and the sealed image
    equals, byte for byte, the unsealed one with every one of the 1M trailers
    set to [type][the oracle's Mask(Extend(Value(block), type))] (so no payload
    byte moved either); lsbm_sst_verify_dev passes all, the dense trailer CRCs
    equal the oracle's, then single-byte corruptions of payload, type and crc
    fail exactly those blocks."""
    torch = torch_cuda
    from lsbm_amd import table
    n, L, seed = 1 << 20, 4118, 0x5EED0005
    sizes = np.full(n, L, dtype=np.int64)
    handles, total = table.layout_blocks(sizes)
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    engine_fill(d, seed)
    rng = np.random.default_rng(7)
    types = rng.integers(0, 2, n).astype(np.uint8)
    dh = _dev(torch, handles.astype(np.int64))
    expect = d.cpu().numpy()
    want = oracle.sst_trailers_mt(expect, 0, handles.astype(np.uint64), types)
    ends = handles[0::2] + L
    expect[ends] = types
    for k in range(4):
        expect[ends + 1 + k] = (want >> (8 * k)).astype(np.uint8)
    nbad = table.seal_blocks(d, dh, _dev(torch, types))
    assert int(nbad.item()) == 0
    img = d.cpu().numpy()
    diff = np.nonzero(img != expect)[0]
    assert diff.size == 0, (diff.size, diff[:8].tolist())
    del expect
    sample = np.unique(np.concatenate([np.arange(32), np.arange(n - 32, n),
                                       rng.choice(n, 256, replace=False)]))
    for i in sample:
        off = int(handles[2 * i])
        blk = stream_bytes(seed, off, L).tobytes()
        assert img[off:off + L].tobytes() == blk
        crc = oracle.extend(oracle.value(blk), bytes([types[i]]))
        assert img[off + L] == types[i]
        assert int.from_bytes(img[off + L + 1:off + L + 5].tobytes(), "little") == oracle.mask(crc), i
    ok, nb = table.verify_blocks(d, dh)
    assert int(nb.item()) == 0 and bool(ok.all())
    # the dense variant returns exactly the crc fields the seal wrote
    tc, nb = table.trailer_crcs(d, dh, _dev(torch, types))
    stored = (img[ends + 1].astype(np.uint32) | (img[ends + 2].astype(np.uint32) << 8) |
              (img[ends + 3].astype(np.uint32) << 16) | (img[ends + 4].astype(np.uint32) << 24))
    assert int(nb.item()) == 0 and np.array_equal(_u32(tc), stored)
    assert np.array_equal(stored, want)
    bad = rng.choice(n, 30, replace=False)
    for j, i in enumerate(bad):
        off = int(handles[2 * i])
        pos = off + (int(rng.integers(0, L)) if j % 3 == 0 else (L if j % 3 == 1 else L + 1 + j % 4))
        d[pos] ^= 1 << (j % 8)
    ok, nb = table.verify_blocks(d, dh)
    assert int(nb.item()) == bad.size
    assert set(np.nonzero(ok.cpu().numpy() == 0)[0].tolist()) == set(bad.tolist())
    del d
    torch.cuda.empty_cache()


def engine_fill(d, seed):
    from lsbm_amd import engine
    engine.fill_splitmix64(d, seed)


def test_sst_handles_past_the_image(torch_cuda, oracle):
    """ReadBlock's "truncated block read" (table/format.cc:88-91) on the device
    ABI: a handle whose n + 5 bytes leave the image is never read or written,
    is counted, and is not ok; every other block is sealed and verified."""
    torch = torch_cuda
    from lsbm_amd import table
    rng = np.random.default_rng(12)
    sizes = rng.integers(0, 6000, 200)
    handles, total = table.layout_blocks(sizes)
    handles = handles.astype(np.int64).copy()
    img = stream_bytes(12, 0, total)
    # guard bytes after the image: must stay untouched
    guard = np.full(4096, 0xA5, dtype=np.uint8)
    full = np.concatenate([img, guard])
    d_full = _dev(torch, full)
    d = d_full[:total]
    bad = {3: (total - 2, 0), 17: (total - 10, 6), 50: (total + 100, 1), 51: (2**62, 10),
           77: (int(handles[2 * 77]), total)}
    for i, (o, sz) in bad.items():
        handles[2 * i], handles[2 * i + 1] = o, sz
    # the last block ends exactly at the image end: fits
    dh = _dev(torch, handles)
    types = rng.integers(0, 2, sizes.size).astype(np.uint8)
    nbad = table.seal_blocks(d, dh, _dev(torch, types))
    assert int(nbad.item()) == len(bad)
    out = d_full.cpu().numpy()
    assert np.array_equal(out[total:], guard)
    for i in range(sizes.size):
        if i in bad:
            continue
        off, sz = int(handles[2 * i]), int(sizes[i])
        crc = oracle.extend(oracle.value(out[off:off + sz].tobytes()), bytes([types[i]]))
        assert int.from_bytes(out[off + sz + 1:off + sz + 5].tobytes(), "little") == oracle.mask(crc)
    ok, nb = table.verify_blocks(d, dh)
    assert int(nb.item()) == len(bad)
    assert set(np.nonzero(ok.cpu().numpy() == 0)[0].tolist()) == set(bad)
    tc, nb = table.trailer_crcs(d, dh, _dev(torch, types))
    tch = _u32(tc)
    assert int(nb.item()) == len(bad)
    for i in range(sizes.size):
        if i in bad:
            assert tch[i] == 0
        else:
            off, sz = int(handles[2 * i]), int(sizes[i])
            assert tch[i] == int.from_bytes(out[off + sz + 1:off + sz + 5].tobytes(), "little")


@pytest.mark.parametrize("seed,smax,n", [(31, 130, 20000), (32, 70, 20000), (33, 5000, 20000),
                                         (34, 130, 150000), (35, 12, 150000),
                                         (36, 130, 600000), (37, 12, 1100000)])
def test_sst_seal_every_trailer_with_tiny_blocks(torch_cuda, oracle, seed, smax, n):
    """Every trailer of a table whose blocks are 0..smax bytes: all trailers
    and every byte between and after them must come out exactly right.  From
    131,072 blocks on, the CRCs go densely into scratch and every wave then
    merges its own blocks' trailers by compare-and-swap on 8-byte words that
    several tiny blocks' trailers share -- words that can straddle two waves'
    ranges (crc32c_kernels.hip crc32c_units_kernel's SstCrc epilogue); below,
    one pass."""
    torch = torch_cuda
    from lsbm_amd import table
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, smax, size=n)
    sizes[rng.random(n) < 0.1] = 4118
    handles, total = table.layout_blocks(sizes)
    img = stream_bytes(seed, 0, total + 256)
    types = rng.integers(0, 2, size=n).astype(np.uint8)
    d = _dev(torch, img)
    dh = _dev(torch, handles.astype(np.int64))
    nbad = table.seal_blocks(d[:total], dh, _dev(torch, types))
    assert int(nbad.item()) == 0
    out = d.cpu().numpy()
    want = img.copy()
    ext = np.stack([handles[0::2], handles[1::2]], 1).astype(np.uint64).reshape(-1)
    offs = np.empty(n + 1, dtype=np.uint64)
    for i in range(n):
        off, sz = int(handles[2 * i]), int(sizes[i])
        crc = oracle.mask(oracle.extend(oracle.value(img[off:off + sz].tobytes()), bytes([types[i]])))
        want[off + sz] = types[i]
        want[off + sz + 1:off + sz + 5] = np.frombuffer(int(crc).to_bytes(4, "little"), np.uint8)
    assert np.array_equal(out, want)
    ok, nb = table.verify_blocks(d[:total], dh)
    assert int(nb.item()) == 0 and bool(ok.all())


def test_host_staged_multi_device_shards(torch_cuda, oracle):
    """lsbm_crc32c_batch_host_multi: contiguous shards, one host thread per
    device.  The box has one GPU, so the shards all go to device 0 through
    concurrent threads (the engine serialises them per device); every CRC must
    still equal the oracle's."""
    from lsbm_amd import engine
    starts, ends, total = _ragged_case(41, 30000, 9000)
    offs = np.concatenate([starts, ends[-1:]]).astype(np.uint64)
    data = stream_bytes(41, 0, total)
    init = np.random.default_rng(1).integers(0, 2**32, size=30000, dtype=np.uint64).astype(np.uint32)
    for devs in ([0], [0, 0], [0, 0, 0, 0]):
        got = engine.crc32c_batch_host_multi(data, offs, devs, init=init, masked=True)
        assert np.array_equal(got, oracle.batch_offsets(data, offs, init, masked=True)), devs


@pytest.mark.parametrize("pieces", [0, 1])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_sst_claimed_pieces_ragged_sizes(torch_cuda, oracle, product_lib, order, pieces):
    """SSTable verify and dense trailer CRCs over >= 131,072 handles, under
    both schedules: one range per wave (the default) and equal-count pieces
    claimed in turn by a workgroup's waves (lsbm_test_sst_pieces(1),
    crc32c_units.h next_piece; round 6).  Here 300,001 blocks of 0-9,000 B
    (so the pieces are far from equal in bytes), handles in file order or
    shuffled, a few past the image: every trailer CRC equals the oracle's
    WriteRawBlock CRC, every verify flag is right, and the bad handles are
    counted exactly."""
    assert product_lib.lsbm_test_sst_pieces(pieces) == 0
    try:
        _sst_ragged_sizes(torch_cuda, oracle, order)
    finally:
        product_lib.lsbm_test_sst_pieces(-1)


def _sst_ragged_sizes(torch_cuda, oracle, order):
    torch = torch_cuda
    from lsbm_amd import table
    rng = np.random.default_rng(21)
    n = 300_001
    sizes = rng.integers(0, 9001, n)
    sizes[::101] = 0
    handles, total = table.layout_blocks(sizes)
    handles = handles.astype(np.int64).copy()
    bad = set(rng.choice(n, 7, replace=False).tolist())
    for i in bad:
        handles[2 * i] = total + 1 + i  # past the image: "truncated block read"
    types = rng.integers(0, 2, n).astype(np.uint8)
    perm = np.arange(n) if order == "sorted" else rng.permutation(n)
    h2 = handles.reshape(n, 2)[perm].reshape(-1).copy()
    t2 = types[perm]
    d = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    engine_fill(d, 0x5EED0021)
    img = d.cpu().numpy()[:total]
    good = np.array([p not in bad for p in perm])
    want = np.zeros(n, dtype=np.uint32)
    want[good] = oracle.sst_trailers_mt(img, 0, h2.reshape(n, 2)[good].reshape(-1).astype(np.uint64), t2[good])
    dh = _dev(torch, h2)
    tc, nb = table.trailer_crcs(d, dh, _dev(torch, t2))
    assert int(nb.item()) == len(bad)
    assert np.array_equal(_u32(tc), want)
    # the image is not sealed yet: every block fails verify (and is counted:
    # one ballot per round, one atomic per walk)
    ok, nb = table.verify_blocks(d, dh)
    assert int(nb.item()) == n and not bool(ok.any())
    # seal (the fused seal, one range per wave) then verify
    nbad = table.seal_blocks(d, dh, _dev(torch, t2))
    assert int(nbad.item()) == len(bad)
    ok, nb = table.verify_blocks(d, dh)
    assert int(nb.item()) == len(bad)
    okh = ok.cpu().numpy()
    assert np.array_equal(okh != 0, good)
    # one corrupted payload byte in a block of each half
    hi = [i for i in (n // 4, 3 * n // 4) if good[i] and h2[2 * i + 1] > 0]
    for i in hi:
        d[int(h2[2 * i]) + int(h2[2 * i + 1]) // 2] ^= 0x40
    ok, nb = table.verify_blocks(d, dh)
    assert int(nb.item()) == len(bad) + len(hi)
    assert set(np.nonzero(ok.cpu().numpy() == 0)[0].tolist()) == set(np.nonzero(~good)[0].tolist()) | set(hi)


def test_sst_handles_past_the_image_merged_seal(torch_cuda, oracle):
    """The same "truncated block read" handles (table/format.cc:88-91) at
    >= 131,072 blocks, where lsbm_sst_seal_dev computes the CRCs densely and
    each wave merges its own trailers after its last row: the merge skips
    handles past the image, writes no byte outside the fitting
    trailers and leaves the guard bytes after the image alone."""
    torch = torch_cuda
    from lsbm_amd import table
    rng = np.random.default_rng(13)
    n = 140_000
    sizes = rng.integers(0, 300, n)
    handles, total = table.layout_blocks(sizes)
    handles = handles.astype(np.int64).copy()
    img = stream_bytes(13, 0, total)
    guard = np.full(4096, 0xA5, dtype=np.uint8)
    full = np.concatenate([img, guard])
    d_full = _dev(torch, full)
    d = d_full[:total]
    bad = {5: (total - 2, 0), 70_000: (total + 100, 1), 100_001: (2**62, 10), 139_990: (total - 10, 6),
           64: (int(handles[2 * 64]), total), n - 1: (total - 4, 0)}
    orig = {i: (int(handles[2 * i]), int(handles[2 * i + 1])) for i in bad}
    for i, (o, sz) in bad.items():
        handles[2 * i], handles[2 * i + 1] = o, sz
    types = rng.integers(0, 2, n).astype(np.uint8)
    nbad = table.seal_blocks(d, _dev(torch, handles), _dev(torch, types))
    assert int(nbad.item()) == len(bad)
    out = d_full.cpu().numpy()
    assert np.array_equal(out[total:], guard)
    good = np.array([i not in bad for i in range(n)])
    offs, szs = handles[0::2][good], handles[1::2][good]
    # every fitting trailer: [type][Mask(crc(block || type))]
    assert np.array_equal(out[offs + szs], types[good])
    parts = [out[o:o + s + 1] for o, s in zip(offs, szs)]
    bo = np.zeros(len(parts) + 1, dtype=np.uint64)
    bo[1:] = np.cumsum([p.size for p in parts])
    want = oracle.batch_offsets(np.concatenate(parts), bo, masked=True)
    t = offs + szs
    stored = (out[t + 1].astype(np.uint32) | (out[t + 2].astype(np.uint32) << 8) |
              (out[t + 3].astype(np.uint32) << 16) | (out[t + 4].astype(np.uint32) << 24))
    assert np.array_equal(stored, want)
    # the bad handles' original trailer slots were never written (their
    # handles were replaced before the seal)
    for i, (o, sz) in orig.items():
        assert np.array_equal(out[o + sz:o + sz + 5], img[o + sz:o + sz + 5]), i


def test_host_pinned_ranges(torch_cuda):
    """Which host ranges the C++ layers DMA in place (host_session.cc
    host_pinned): a hipHostMalloc'd buffer and one hipHostRegister'd range
    (which reports no address range, so its buffer id decides) in whole and
    in part; not a range running past the registration, not two adjacent
    registrations with a gap, not pageable memory."""
    import ctypes
    torch = torch_cuda
    from lsbm_amd._lib import lib
    L = lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipHostRegister.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint]
    hip.hipHostUnregister.argtypes = [ctypes.c_void_p]
    pinned = torch.empty(3 << 20, dtype=torch.uint8, pin_memory=True)
    p = pinned.data_ptr()
    assert L.lsbm_test_host_pinned(p, 3 << 20) == 1
    assert L.lsbm_test_host_pinned(p + 12345, 1 << 20) == 1
    page = 4096
    raw = np.zeros(6 << 20, dtype=np.uint8)
    a = (raw.ctypes.data + page - 1) // page * page
    assert L.lsbm_test_host_pinned(a, 1 << 20) == 0  # pageable
    assert hip.hipHostRegister(a, 2 << 20, 0) == 0
    try:
        assert hip.hipHostRegister(a + (2 << 20) + page, 2 << 20, 0) == 0
        try:
            assert L.lsbm_test_host_pinned(a, 2 << 20) == 1
            assert L.lsbm_test_host_pinned(a + 777, (1 << 20) + 5) == 1
            assert L.lsbm_test_host_pinned(a, (2 << 20) + 1) == 0  # past the registration
            assert L.lsbm_test_host_pinned(a, (4 << 20) + page) == 0  # two registrations, a gap
        finally:
            hip.hipHostUnregister(a + (2 << 20) + page)
    finally:
        hip.hipHostUnregister(a)
