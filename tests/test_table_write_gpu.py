"""GPU tests of the batched table finish (include/lsbm_table_write.h;
sstable.finish_tables / write_tables, memtable.sort_segments / flush_many, and
sstable.compact and memtable.recover_all, which write through them) against
the reference-written fixtures, the host models and the one-table calls.
"""
import random

import numpy as np
import pytest

from golden import blockmodel as bm
from golden import buildmodel as bd
from golden import memcut_cases as cases
from golden import memtable_cases as mc
from golden import memtablemodel as mt
from golden import mergemodel as mm
from golden import snappy_table_cases as tc
from golden import snappytablemodel as stm
from golden import tablewritemodel as tw
from test_memcut import FIXTURE
from test_memcut_gpu import log_of, tobytes
from test_memtable_gpu import Keys, ikey
from test_sstable import Entries, _dev, _image, codec, fx  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
GUARD = 0xEE


def join(torch, tables):
    """[[(key, value)]] -> (Entries of all of them, table_first)."""
    first = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    return Entries(torch, [e for t in tables for e in t]), first


def gpu_write_tables(torch, tables, params, compression):
    from lsbm_amd import sstable
    cmp, block_size, restart_interval, bits_per_key = params
    E, first = join(torch, tables)
    return sstable.write_tables(E.keys, E.koff, E.values, E.image, _dev(torch, first), cmp, block_size,
                                restart_interval, bits_per_key, compression)


def table_of(res, t):
    return (tobytes(res.table(t)), res.table_data_handles(t).cpu().numpy().reshape(-1, 2).tolist(),
            list(res.index_handle(t)))


def outer(cmp, block_size, restart_interval, seed):
    """Entries for the tables either side of a case's, valid under its comparator."""
    if cmp == bm.INTERNAL_KEY:
        return [(mm.internal_key(b"outer%05d" % i, 500 - i), tc._random(seed + i, 30 + i % 50)) for i in range(40)]
    return tc._blocks_of_kinds("xrx", block_size, restart_interval, seed)


def check_arena(res):
    """Bases are multiples of 256 and the bytes between the tables are zero."""
    arena = res.arena.cpu().numpy()
    covered = np.zeros(arena.size, dtype=bool)
    for base, size in res.table_handles.cpu().tolist():
        assert base % 256 == 0
        covered[base:base + size] = True
    assert not arena[~covered].any()


# ---------------------------------------------------------------- write_tables


def test_three_tables_equal_the_fixture_and_the_models(torch_cuda, fx, codec):  # noqa: F811
    file_cases, _ = fx
    for name, params in tc.CASES.items():
        cmp, block_size, restart_interval, bits_per_key = params
        tables = [outer(cmp, block_size, restart_interval, 7000), tc.entries(name),
                  outer(cmp, block_size, restart_interval, 8000)[:-3]]
        res = gpu_write_tables(torch_cuda, tables, params, 1)
        check_arena(res)
        r = file_cases[name]
        data, handles, index_handle = table_of(res, 1)
        assert data == r["data"], name
        assert handles == r["data_handles"] and index_handle == r["index_handle"], name
        for t in (0, 2):
            want = stm.table_file(tables[t], cmp, block_size, restart_interval, bits_per_key, codec[0])
            got = table_of(res, t)
            assert got[0] == want[0], (name, t)
            assert got[1] == [list(h) for h in want[1]] and got[2] == list(want[2]), (name, t)
        assert res.smallest[0] == tables[0][0][0] and res.largest[2] == tables[2][-1][0]
        assert (res.smallest[1], res.largest[1]) == ((tables[1][0][0], tables[1][-1][0]) if tables[1] else (None, None))
        res = gpu_write_tables(torch_cuda, tables, params, 0)
        for t in range(3):
            want = bd.table_file(tables[t], cmp, block_size, restart_interval, bits_per_key)
            assert table_of(res, t)[0] == want[0], (name, t)


def varied_tables(n_tables):
    """Tables of one call: a one-entry table, an empty one, data ends below and
    above 16,384 (the handle varints change length), an index block that is
    kept compressed and one that stays raw."""
    small = tc._blocks_of_kinds("rx", 128, 4, 300)                        # data_end well below 16,384
    large = tc._blocks_of_kinds("x" * 160, 128, 4, 400)                   # above it
    index_comp = [(b"tenant-0001/table-orders/row-%08d" % (7 * i), b"v%03d" % i) for i in range(120)]
    index_raw = [(bytes([40 + 20 * i]) + tc._random(500 + i, 11), tc._random(600 + i, 90)) for i in range(9)]
    kinds = [[(b"only-key", b"value")], [], small, large, index_comp, index_raw]
    return [kinds[t % len(kinds)] if t < len(kinds) else tc._blocks_of_kinds("rxr"[:1 + t % 3], 128, 4, 900 + t)
            for t in range(n_tables)]


@pytest.mark.parametrize("n_tables", [1, 2, 65])
def test_write_tables_equals_write_table_of_each_slice(torch_cuda, n_tables, codec):  # noqa: F811
    """A table's bytes do not depend on its neighbours (write_table is
    write_tables of one table), and they are the host models'."""
    from lsbm_amd import sstable
    torch = torch_cuda
    tables = varied_tables(max(n_tables, 6))[:n_tables] if n_tables > 2 else varied_tables(6)[2 * n_tables:3 * n_tables]
    if n_tables > 2:  # the smallest shapes stay in
        assert tables[0] == [(b"only-key", b"value")] and tables[1] == []
    for bits_per_key in (None, 10):
        for compression in (0, 1):
            res = gpu_write_tables(torch, tables, (bm.BYTEWISE, 128, 4, bits_per_key), compression)
            check_arena(res)
            for t, entries in enumerate(tables):
                E = Entries(torch, entries)
                image, handles, index_handle = sstable.write_table(E.keys, E.koff, E.values, E.image, bm.BYTEWISE, 128,
                                                                   4, bits_per_key, compression)
                got = table_of(res, t)
                assert image.is_contiguous() and image.numel() == len(got[0])
                assert got[0] == tobytes(image), (n_tables, bits_per_key, compression, t)
                assert got[1] == handles.cpu().numpy().reshape(-1, 2).tolist() and got[2] == list(index_handle)
                want = stm.table_file(entries, bm.BYTEWISE, 128, 4, bits_per_key, codec[0]) if compression else \
                    bd.table_file(entries, bm.BYTEWISE, 128, 4, bits_per_key)
                assert got[0] == want[0], (n_tables, bits_per_key, compression, t)
                assert got[1] == [list(h) for h in want[1]] and got[2] == list(want[2])
    if n_tables == 65:  # (the last call: bloom and snappy) data ends either side of 16,384, index blocks of both types
        last = [res.table_data_handles(t).cpu().tolist()[-2:] for t in (2, 3)]
        assert last[0][0] + last[0][1] + 5 < 16384 < last[1][0] + last[1][1] + 5
        types = [tobytes(res.table(t))[res.index_handle(t)[0] + res.index_handle(t)[1]] for t in (4, 5)]
        assert types == [1, 0]


def test_host_reads_do_not_grow_with_the_tables(torch_cuda, monkeypatch):
    torch = torch_cuda
    counts = {}

    def counted(name):
        real = getattr(torch.Tensor, name)

        def call(self, *a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return real(self, *a, **kw)
        return call

    from lsbm_amd import memtable, sstable

    def reads_of(call):
        with monkeypatch.context() as m:
            counts.clear()
            for name in ("cpu", "item", "tolist"):
                m.setattr(torch.Tensor, name, counted(name))
            got = call()
            return dict(counts), got

    reads = []
    for n_tables in (1, 2, 33):
        tables = [tc._blocks_of_kinds("rxr"[:1 + t % 3], 128, 4, 100 + t) for t in range(n_tables)]
        E, first = join(torch, tables)
        first = _dev(torch, first)
        reads.append(reads_of(lambda: sstable.write_tables(E.keys, E.koff, E.values, E.image, first, bm.BYTEWISE, 128,
                                                           4, 10, 1))[0])
    assert reads[0] == reads[1] == reads[2] and sum(reads[0].values()) > 0, reads
    # recover_all: one log (no record of it is in error) cut into one, a few and many memtables
    log = log_of(torch, dict(cases.scenarios())["five_memtables"])
    reads, tables = [], []
    for write_buffer_size in (1 << 30, 160 << 10, 64 << 10):
        r, got = reads_of(lambda: memtable.recover_all(log, write_buffer_size=write_buffer_size, bits_per_key=10))
        reads.append(r)
        tables.append(len(got.flushes))
    assert tables[0] == 1 < tables[1] < tables[2] >= 5, tables
    assert reads[0] == reads[1] == reads[2] and sum(reads[0].values()) > 0, reads


# ---------------------------------------------------------------- the filter layout


def layout_inputs(names, entry_base=0):
    """Tables laid out by LAYOUT_CASES: (block_first, table_block_first, data_handles, data_end, per table
    (starts, firsts, end))."""
    block_first, tbf, handles, ends, per = [entry_base], [0], [], [], []
    for name in names:
        sizes = tw.LAYOUT_CASES[name]
        start, end = tw.starts_of(sizes)
        first = tw.firsts_of(len(sizes), block_first[-1])
        block_first += first[1:].tolist()
        tbf.append(tbf[-1] + len(sizes))
        handles += [x for s, n in zip(start.tolist(), sizes) for x in (s, n)]
        ends.append(end)
        per.append((start, first, end))
    return block_first, tbf, handles, ends, per


@pytest.mark.parametrize("name", sorted(tw.LAYOUT_CASES))
def test_filter_layout_single_and_second_of_three(torch_cuda, name):
    from lsbm_amd import bloom, sstable
    torch = torch_cuda
    for names in ([name], ["above_4k", name, "many_32"], ["none", name, "single"]):
        bf, tbf, handles, ends, per = layout_inputs(names)
        d = [_dev(torch, np.array(a, dtype=np.int64)) for a in (bf, tbf, handles, ends)]
        sizes_only = sstable.filter_layout(d[0], d[1], d[2], d[3], 10)
        want = []
        for start, first, end in per:
            nb = len(start)
            want.append(bloom.layout_filter_block(list(start) + ([end] if nb else []),
                                                  list(first) + ([first[-1]] if nb else []), 10))
        assert sizes_only.size.cpu().tolist() == [w.total_bytes for w in want], names
        assert sizes_only.count.cpu().tolist() == [len(w.filter_keys) for w in want], names
        assert sizes_only.status.cpu().tolist() == [0] * len(names)
        # windows with a gap of 3 guard bytes between them
        win, at = [], 7
        for w in want:
            win += [at, w.total_bytes]
            at += w.total_bytes + 3
        out = torch.full((at + 9,), GUARD, dtype=torch.uint8, device="cuda")
        n_filters = sum(len(w.filter_keys) for w in want)
        lay = sstable.filter_layout(d[0], d[1], d[2], d[3], 10, out, _dev(torch, np.array(win, dtype=np.int64)),
                                    n_filters)
        assert lay.status.cpu().tolist() == [0] * len(names)
        assert lay.size.cpu().tolist() == [w.total_bytes for w in want]
        keys = [k for w in want for k in w.filter_keys]
        assert lay.filter_first.cpu().tolist() == [k0 for k0, _ in keys] + [bf[-1]], names
        outs = [win[2 * t] + o for t, w in enumerate(want) for o in w.filter_out]
        assert lay.filter_out.cpu().tolist() == outs, names
        host = out.cpu().numpy()
        expect = np.full(host.size, GUARD, dtype=np.uint8)
        care = np.ones(host.size, dtype=bool)
        for t, w in enumerate(want):
            care[win[2 * t]:win[2 * t] + w.data_bytes] = False  # (the filters' own bytes: lsbm_bloom_build_dev's)
            expect[win[2 * t] + w.data_bytes:win[2 * t] + w.total_bytes] = np.frombuffer(w.trailer, np.uint8)
        assert np.array_equal(host[care], expect[care]), names
        assert (host[~care] == GUARD).all()  # (and the layout call left them alone)


# ---------------------------------------------------------------- compaction


def test_compact_batched_equals_the_fixture_and_the_loop(torch_cuda, fx, codec):  # noqa: F811
    torch = torch_cuda
    from lsbm_amd import merge, sstable
    _, comp = fx
    c = dict(tc.COMPACTION)
    cmp, max_file_size = c.pop("cmp"), c.pop("max_file_size")
    images = [_image(torch, r["data"]) for r in comp["inputs"]]
    handles = [np.array(r["data_handles"], dtype=np.int64).reshape(-1) for r in comp["inputs"]]
    want = [r["data"] for r in comp["outputs"]]
    assert len(want) >= 3
    out = sstable.compact(images, handles, max_file_size, cmp=cmp, compression=1, **c)
    assert [tobytes(o.image) for o in out] == want
    read = [stm.read_table(f, codec[1]) for f in want]  # (the handles the reference-written files hold)
    assert [o.data_handles.cpu().numpy().reshape(-1, 2).tolist() for o in out] == \
        [[list(h) for h in r["data_handles"]] for r in read]
    assert [list(o.index_handle) for o in out] == [list(r["index_handle"]) for r in read]
    out = sstable.compact(images, None, max_file_size, index_handles=[r["index_handle"] for r in comp["inputs"]],
                          cmp=cmp, compression=1, **c)
    assert [tobytes(o.image) for o in out] == want
    # compression=0: the model merge of the inputs, cut over the raw block sizes, each table the host model's file
    kept, _ = mm.merge_entries(tc.compaction_runs(), cmp, c["drop"], c["smallest_snapshot"], c["bottom_level"])
    first, sizes = bd.plan([(k, len(v)) for k, v in kept], c["block_size"], c["restart_interval"])
    table_first, _ = merge.cut_tables(first, sizes, max_file_size)
    model = [bd.table_file(kept[e0:e1], cmp, c["block_size"], c["restart_interval"], c["bits_per_key"])
             for e0, e1 in zip(table_first[:-1], table_first[1:])]
    raw = sstable.compact(images, handles, max_file_size, cmp=cmp, compression=0, **c)
    assert [tobytes(o.image) for o in raw] == [m[0] for m in model] and len(raw) >= 3
    assert [o.data_handles.cpu().numpy().reshape(-1, 2).tolist() for o in raw] == \
        [[list(h) for h in m[1]] for m in model]
    assert [list(o.index_handle) for o in raw] == [list(m[2]) for m in model]


# ---------------------------------------------------------------- the segmented sort


def check_segments(torch, keys, seg_first, label=""):
    from lsbm_amd import memtable
    K = Keys(torch, keys)
    p = memtable.sort_segments(K.keys, K.koff, _dev(torch, np.array(seg_first, dtype=np.int64)))
    want = []
    for lo, hi in zip(seg_first[:-1], seg_first[1:]):
        want += [lo + i for i in mt.skiplist_order(keys[lo:hi])]
    assert p.run_status.cpu().tolist() == [0], label
    assert p.source.cpu().tolist() == want, label
    assert p.counts.cpu().tolist() == [len(keys), sum(len(k) for k in keys)], label
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(keys[i]) for i in want])
    assert np.array_equal(p.out_key_offsets.cpu().numpy(), off), label
    return K, p


def mixed_keys(rng, n):
    return [ikey(bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 12))), rng.randrange(1, 50), rng.choice((0, 1)))
            for _ in range(n)]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_sort_segments_shapes(torch_cuda, n):
    from lsbm_amd import memtable
    rng = random.Random(0x5E65 + n)
    keys = mixed_keys(rng, n)
    cuts = sorted({c for c in (1, 255, 256, 257, n - 1) if 0 < c < n})
    K, p = check_segments(torch_cuda, keys, [0, n], "one segment")
    one = memtable.sort(K.keys, K.koff)
    assert p.source.cpu().tolist() == one.source.cpu().tolist()
    assert p.out_key_offsets.cpu().tolist() == one.out_key_offsets.cpu().tolist()
    check_segments(torch_cuda, keys, [0] + cuts + [n], "every cut")
    for c in cuts:
        check_segments(torch_cuda, keys, [0, c, n], c)
    # empty segments first, in the middle and last
    check_segments(torch_cuda, keys, [0, 0, 0] + cuts[:1] * 3 + [n, n], "empty segments")


def test_sort_segments_orders(torch_cuda):
    torch = torch_cuda
    rng = random.Random(0x0D0E)
    # 300 one-entry segments: the input order stays
    keys = mixed_keys(rng, 300)
    _, p = check_segments(torch, keys, list(range(301)), "one-entry segments")
    assert p.source.cpu().tolist() == list(range(300))
    # two adjacent segments with the same user keys and tags a global sort would interleave
    users = [b"user%03d" % i for i in range(150)]
    a = [ikey(u, 2 * i + 2) for i, u in enumerate(users)]
    b = [ikey(u, 2 * i + 1) for i, u in enumerate(users)]
    rng.shuffle(a)
    rng.shuffle(b)
    check_segments(torch, a + b, [0, 150, 300], "same user keys")
    assert mt.skiplist_order(a + b) != mt.skiplist_order(a) + [150 + i for i in mt.skiplist_order(b)]
    # no prefix in common between the segments, a long one inside each
    segs = [[ikey(bytes([65 + s]) * 40 + bytes(rng.choice(b"xyz") for _ in range(rng.randint(0, 9))),
                  rng.randrange(1, 9)) for _ in range(140 + 60 * s)] for s in range(3)]
    flat = [k for s in segs for k in s]
    check_segments(torch, flat, [0, 140, 340, 600], "own prefixes")
    # equal internal keys inside a segment: the later one first
    keys = [ikey(b"same", 9)] * 5 + [ikey(b"same", 9)] * 300
    _, p = check_segments(torch, keys, [0, 5, 305], "equal keys")
    assert p.source.cpu().tolist() == [4, 3, 2, 1, 0] + list(range(304, 4, -1))


def test_sort_segments_bad_seg_first(torch_cuda):
    from lsbm_amd import _lib, memtable
    from lsbm_amd.engine import _ptr, _stream_ptr
    torch = torch_cuda
    keys = mixed_keys(random.Random(3), 300)
    K = Keys(torch, keys)
    n = len(keys)
    L = _lib.lib()
    need = L.lsbm_memtable_sort_segments_scratch_bytes(n, 3)
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for seg_first in ([0, 200, 100, n], [0, 100, 200, n - 1], [1, 100, 200, n], [0, 100, 200, n + 1]):
        source = torch.full((n,), -5, dtype=torch.int64, device="cuda")
        seg = _dev(torch, np.array(seg_first, dtype=np.int64))
        rc = L.lsbm_memtable_sort_segments_dev(_ptr(K.keys), K.keys.numel(), _ptr(K.koff), n, _ptr(seg), 3,
                                               _ptr(source), _ptr(out_off), _ptr(counts), _ptr(status),
                                               _ptr(scratch), need, _stream_ptr(None))
        assert rc == _lib.LSBM_OK
        assert status.cpu().tolist() == [2] and counts.cpu().tolist() == [0, 0], seg_first
        assert (source == -5).all(), seg_first
    seg = _dev(torch, np.array([0, 100, 200, n], dtype=np.int64))
    call = lambda nbytes, src: L.lsbm_memtable_sort_segments_dev(  # noqa: E731
        _ptr(K.keys), K.keys.numel(), _ptr(K.koff), n, _ptr(seg), 3, _ptr(src), _ptr(out_off), _ptr(counts),
        _ptr(status), _ptr(scratch), nbytes, _stream_ptr(None))
    assert call(need - 1, source) == _lib.LSBM_ERR_INVALID
    assert call(need, seg) == _lib.LSBM_ERR_INVALID  # an output that aliases an input
    assert call(need, source) == _lib.LSBM_OK and status.cpu().tolist() == [0]
    p = memtable.sort_segments(K.keys, K.koff, seg)
    assert source.cpu().tolist() == p.source.cpu().tolist()


# ---------------------------------------------------------------- flush_many and recover_all


def same_flush(f, t, label):
    assert tobytes(f.image) == tobytes(t.image), label
    assert f.data_handles.cpu().tolist() == t.data_handles.cpu().tolist(), label
    assert tuple(f.index_handle) == tuple(t.index_handle), label
    assert (f.smallest, f.largest, f.max_sequence) == (t.smallest, t.largest, t.max_sequence), label
    assert f.status.cpu().tolist() == t.status.cpu().tolist(), label


def test_flush_many_equals_flush_of_each_slice(torch_cuda):
    from lsbm_amd import memtable
    fixture_cases, _ = mc.load()
    done = 0
    for c in fixture_cases:
        image, records = memtable.log_records(c["log"])
        n = records.numel() // 2
        if n < 5:
            continue
        done += 1
        kw = dict(block_size=c["block_size"], restart_interval=c["restart_interval"], bits_per_key=c["bits_per_key"])
        splits = [[0, n], [0, n // 2, n], [0, 1, n // 3, n // 2, n - 1, n], [0, 0, n // 2, n // 2, n, n]]
        host, pairs = tobytes(image), records.cpu().numpy().reshape(-1, 2).tolist()
        model = {}  # (lo, hi) -> the host model's file of that memtable (None without entries)
        for mem_first in splits:
            slices = list(zip(mem_first[:-1], mem_first[1:]))
            for s in slices:
                if s not in model:
                    model[s] = mt.table_file(mt.entries(host, pairs[s[0]:s[1]])[0], c["block_size"],
                                             c["restart_interval"], c["bits_per_key"])
            for compression in (0, 1):
                got = memtable.flush_many(image, records, mem_first, compression=compression, **kw)
                want = [memtable.flush(image, records[2 * lo:2 * hi].contiguous(), compression=compression, **kw)
                        for lo, hi in slices]
                want = [w for w in want if w.image is not None]
                assert len(got) == len(want) >= 1, (c["name"], mem_first)
                for f, t in zip(got, want):
                    same_flush(f, t, (c["name"], mem_first, compression))
                if compression == 0:
                    assert [tobytes(f.image) for f in got] == [model[s] for s in slices if model[s] is not None], \
                        (c["name"], mem_first)
    assert done


def flushes_of(image, bounds, **kw):
    """memtable.flush of each slice [lo, hi) of log.read_records' records; memtables without entries are dropped."""
    from lsbm_amd import log as lg
    from lsbm_amd import memtable
    r = lg.read_records(image)
    out = [memtable.flush(r.image, r.records[lo:hi].reshape(-1).contiguous(), **kw) for lo, hi in bounds]
    return [f for f in out if f.image is not None], r


@pytest.mark.parametrize("name", ["five_memtables", "too_small", "records_in_error", "cut_on_last"])
def test_recover_all_batched_equals_the_loop(torch_cuda, name):
    from lsbm_amd import memtable
    reps = dict(cases.scenarios())[name]
    log = log_of(torch_cuda, reps)
    got = memtable.recover_all(log, write_buffer_size=65536, bits_per_key=10)
    mem_first = FIXTURE["scenarios"][name]["cuts"]["recover_65536"]["mem_first"] + [len(reps)]
    want, r = flushes_of(log, zip(mem_first[:-1], mem_first[1:]), bits_per_key=10)
    assert got.mem_first == mem_first and got.status is None
    assert got.events.cpu().tolist() == r.events.cpu().tolist()
    assert len(got.flushes) == len(want)
    for f, t in zip(got.flushes, want):
        same_flush(f, t, name)


def test_recover_all_batched_paranoid_keeps_the_finished_tables_only(torch_cuda):
    from lsbm_amd import memtable
    name = "records_in_error"
    reps = dict(cases.scenarios())[name]
    s = FIXTURE["scenarios"][name]
    bad = [i for i, st in enumerate(s["status"]) if st != 0][0]
    log = log_of(torch_cuda, reps)
    torn = log.clone()
    torn[40000] ^= 0xFF
    for image in (log, torn):
        loose = memtable.recover_all(image, write_buffer_size=65536)
        got = memtable.recover_all(image, write_buffer_size=65536, paranoid=True)
        assert got.status.startswith("Corruption: ")
        # the records the loop took: up to the reader's first report, or to the first record in error
        taken = min([bad] + ([int(got.events[0][0])] if got.events.shape[0] else []))
        if image is log:
            assert got.status == "Corruption: " + memtable.STATUS_MESSAGE[s["status"][bad]]
        assert got.events.cpu().tolist() == loose.events.cpu().tolist()
        # the cut runs record by record: the cuts of a prefix are a prefix of the cuts
        k = len(got.mem_first) - 1
        assert got.mem_first == loose.mem_first[:k] + [taken] and 0 < taken < loose.mem_first[-1]
        # the memtables the whole log closes too are written, the one in progress is not
        closed = set(zip(loose.mem_first[:-2], loose.mem_first[1:-1]))
        bounds = [b for b in zip(got.mem_first[:-1], got.mem_first[1:]) if b in closed]
        want, _ = flushes_of(image, bounds)
        assert len(want) == len(got.flushes) and (image is torn or len(want) >= 1)
        for f, t in zip(got.flushes, want):
            same_flush(f, t, "paranoid")
    loose = memtable.recover_all(log, write_buffer_size=65536)
    assert 1 <= len([m for m in range(len(loose.mem_first) - 1) if loose.mem_first[m + 1] <= bad]) < len(loose.flushes)


# ---------------------------------------------------------------- errors


def guarded(torch, n, dtype):
    """n elements with 8 guard elements either side: (whole, window)."""
    fill = GUARD if dtype == torch.uint8 else -0x1111
    whole = torch.full((n + 16,), fill, dtype=dtype, device="cuda")
    return whole, whole[8:8 + n]


def guards_intact(torch, whole, n):
    fill = GUARD if whole.dtype == torch.uint8 else -0x1111
    return bool((whole[:8] == fill).all()) and bool((whole[8 + n:] == fill).all())


def test_errors_leave_the_guards_alone(torch_cuda):
    from lsbm_amd import _lib, sstable
    from lsbm_amd.engine import _ptr, _stream_ptr
    torch = torch_cuda
    raw = [100, 200, 300, 50, 60]
    raw_len = _dev(torch, np.array(raw, dtype=np.int64))
    # a table_block_first that decreases: every table BAD_INPUT, nothing else written
    types_w, types = guarded(torch, 5, torch.uint8)
    handles_w, handles = guarded(torch, 10, torch.int64)
    end_w, end = guarded(torch, 3, torch.int64)
    status_w, status = guarded(torch, 3, torch.int32)
    for tbf in ([0, 4, 2, 5], [0, 2, 4, 6], [1, 2, 4, 5]):
        sstable.pack_plan_tables(raw_len, None, _dev(torch, np.array(tbf, dtype=np.int64)), None, 5, types, handles,
                                 end, status)
        assert status.cpu().tolist() == [2, 2, 2], tbf
        assert bool((types == GUARD).all()) and bool((handles == -0x1111).all()) and bool((end == -0x1111).all())
    tbf = _dev(torch, np.array([0, 2, 2, 5], dtype=np.int64))
    first = _dev(torch, np.array([1 << 33, 7, 0], dtype=np.int64))
    sstable.pack_plan_tables(raw_len, None, tbf, first, 5, types, handles, end, status)
    assert status.cpu().tolist() == [0, 0, 0]
    assert handles.cpu().tolist() == [1 << 33, 100, (1 << 33) + 105, 200, 0, 300, 305, 50, 360, 60]
    assert end.cpu().tolist() == [(1 << 33) + 310, 7, 425] and types.cpu().tolist() == [0] * 5
    for w, n in ((types_w, 5), (handles_w, 10), (end_w, 3), (status_w, 3)):
        assert guards_intact(torch, w, n)
    # an output aliasing an input
    L = _lib.lib()
    scratch = torch.empty(64, dtype=torch.int64, device="cuda")
    assert L.lsbm_table_pack_plan_dev(_ptr(raw_len), None, 5, _ptr(tbf), 3, None, 5, _ptr(types), _ptr(raw_len),
                                      _ptr(end), _ptr(status), _ptr(scratch), 512, _stream_ptr(None)) == \
        _lib.LSBM_ERR_INVALID
    # a tail window one byte too small: NO_ROOM for that table only
    bf, tbf_l, dh, ends, per = layout_inputs(["many_256", "above_4k", "single"])
    d = [_dev(torch, np.array(a, dtype=np.int64)) for a in (bf, tbf_l, dh, ends)]
    sizes = sstable.filter_layout(d[0], d[1], d[2], d[3], 10)
    need, count = sizes.size.cpu().tolist(), int(sizes.count.sum())
    win, at = [], 8
    for t, nbytes in enumerate(need):
        win += [at, nbytes - (1 if t == 1 else 0)]
        at += nbytes + 8
    out = torch.full((at,), GUARD, dtype=torch.uint8, device="cuda")
    lay = sstable.filter_layout(d[0], d[1], d[2], d[3], 10, out, _dev(torch, np.array(win, dtype=np.int64)), count)
    assert lay.status.cpu().tolist() == [0, 1, 0]
    host = out.cpu().numpy()
    assert (host[win[2] - 8:win[4]] == GUARD).all()  # table 1's window and the guards either side of it
    assert host[win[0] + need[0] - 1] == 11 and host[win[4] + need[2] - 1] == 11  # the others are written
    fo = lay.filter_out.cpu().tolist()
    c = sizes.count.cpu().tolist()
    assert all(x == -1 for x in fo[c[0]:c[0] + c[1]]) and all(x >= 0 for x in fo[:c[0]] + fo[c[0] + c[1]:])
    meta_sizes, _ = sstable.metaindex_blocks(d[3], sizes.size)
    mwin = [8, int(meta_sizes[0]), 80, int(meta_sizes[1]) - 1, 160, int(meta_sizes[2])]
    mout = torch.full((240,), GUARD, dtype=torch.uint8, device="cuda")
    _, mst = sstable.metaindex_blocks(d[3], sizes.size, mout, _dev(torch, np.array(mwin, dtype=np.int64)))
    assert mst.cpu().tolist() == [0, 1, 0]
    mhost = mout.cpu().numpy()
    assert (mhost[mwin[0] + mwin[1]:mwin[4]] == GUARD).all() and (mhost[:8] == GUARD).all()
    want0 = b"\0\x21" + bytes([len(bd.encode_handle(ends[0], need[0]))]) + bd.FILTER_KEY + \
        bd.encode_handle(ends[0], need[0]) + b"\0\0\0\0\1\0\0\0"
    assert mhost[8:8 + mwin[1]].tobytes() == want0
    # an arena one byte short of the last footer
    tail_handles = _dev(torch, np.array([1000, 10, 1015, 20, 500, 10, 515, 20], dtype=np.int64))
    tail_end = _dev(torch, np.array([1040, 540], dtype=np.int64))
    base = _dev(torch, np.array([0, 1280], dtype=np.int64))
    tbf2 = _dev(torch, np.array([0, 1, 2], dtype=np.int64))
    data_handles = _dev(torch, np.array([0, 995, 0, 495], dtype=np.int64))
    whole = torch.full((1280 + 588 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    for short, want_status in ((0, [0, 0]), (1, [0, 1])):
        whole.fill_(GUARD)
        arena = whole[:1280 + 588 - short]
        placed = sstable.place_tables(data_handles, tbf2, tail_handles, 2, tail_end, base, arena)
        assert placed.status.cpu().tolist() == want_status
        assert placed.table_size.cpu().tolist() == [1088, 588]
        assert placed.data_handles.cpu().tolist() == [0, 995, 1280, 495]
        assert placed.tail_handles.cpu().tolist() == [1000, 10, 1015, 20, 1780, 10, 1795, 20]
        host = whole.cpu().numpy()
        assert host[1040:1088].tobytes() == bd.footer((1000, 10), (1015, 20))
        second = host[1280 + 540:1280 + 588].tobytes()
        assert second == (bd.footer((500, 10), (515, 20)) if not short else bytes([GUARD]) * 48)
        assert (host[:1040] == GUARD).all() and (host[1088:1280 + 540] == GUARD).all() and \
            (host[1280 + 588:] == GUARD).all()
