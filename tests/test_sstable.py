"""Tables with snappy-compressed blocks (include/lsbm_table_pack.h,
lsbm_amd/sstable.py).

CPU: the plain-Python model (tests/golden/snappytablemodel.py) with the snappy
oracle's compress against the files libsnappy produced
(tests/golden/snappy_tables.json + .bin, written by
make_snappy_table_fixture.py); read_table over every file; the keep rule.
GPU: the plan and pack kernels against the Python rule and numpy; write_table,
read_blocks, table_get and compact byte-exact against the fixture or the model.
"""
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the product library is loaded: see test_entry_points_check_arguments)

from golden import blockmodel as bm
from golden import buildmodel as bd
from golden import mergemodel as mm
from golden import snappy_table_cases as tc
from golden import snappytablemodel as stm

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
GUARD = 0xEE
U64 = stm.U64
RULE_RAW = list(range(18)) + [4096, (1 << 32) - 2]


def rule_pairs():
    """(raw_len, comp_len) at the rule's edges, as unsigned 64-bit numbers."""
    out = []
    for raw in RULE_RAW:
        edge = raw - raw // 8
        out += [(raw, (edge - 1) & U64), (raw, edge), (raw, 0), (raw, U64)]
    return out


@pytest.fixture(scope="module")
def fx():
    """{name: record with 'data'}, and the compaction's inputs / outputs."""
    rec = json.load(open(os.path.join(G, "snappy_tables.json")))
    blob = open(os.path.join(G, "snappy_tables.bin"), "rb").read()

    def data(r):
        return blob[r["offset"]:r["offset"] + r["length"]]

    cases = {}
    for r in rec["cases"]:
        r["data"] = data(r)
        cases[r["name"]] = r
    for r in rec["compaction"]["inputs"] + rec["compaction"]["outputs"]:
        r["data"] = data(r)
    return cases, rec["compaction"]


@pytest.fixture(scope="module")
def codec(snappy_oracle):
    """(compress, uncompress) callables of the model, from the snappy oracle."""
    def uncompress(c):
        ok, out = snappy_oracle.uncompress(c)
        return out if ok else None

    return snappy_oracle.compress, uncompress


@pytest.fixture(scope="module")
def tables(fx, codec):
    """{name: read_table of the fixture file}: computed once, read by many tests."""
    return {name: stm.read_table(r["data"], codec[1]) for name, r in fx[0].items()}


# ---------------------------------------------------------------- CPU


def test_fixture_has_every_case(fx):
    cases, comp = fx
    assert set(cases) == set(tc.CASES)
    assert len(comp["inputs"]) == 3 and len(comp["outputs"]) >= 3


def test_model_reproduces_fixture(fx, codec):
    cases, comp = fx
    for name, (cmp, block_size, restart_interval, bits_per_key) in tc.CASES.items():
        data, handles, index_handle, types = stm.table_file(tc.entries(name), cmp, block_size, restart_interval,
                                                            bits_per_key, codec[0])
        r = cases[name]
        assert data == r["data"], name
        assert [list(h) for h in handles] == r["data_handles"] and list(index_handle) == r["index_handle"], name
        assert types == r["types"], name
    c = tc.COMPACTION
    runs = tc.compaction_runs()
    for run, r in zip(runs, comp["inputs"]):
        assert stm.table_file(run, c["cmp"], c["block_size"], c["restart_interval"], c["bits_per_key"],
                              codec[0])[0] == r["data"]
    out = stm.compact(runs, c["cmp"], c["max_file_size"], c["drop"], c["smallest_snapshot"], c["bottom_level"],
                      c["block_size"], c["restart_interval"], c["bits_per_key"], codec[0])
    assert out == [r["data"] for r in comp["outputs"]]


def test_read_table_returns_entries_and_types(fx, tables):
    cases, _ = fx
    for name, r in cases.items():
        t = tables[name]
        assert t["entries"] == tc.entries(name), name
        assert t["types"] == r["types"], name
        assert [list(h) for h in t["data_handles"]] == r["data_handles"], name
    assert cases["none_compressible"]["data"] == bd.table_file(tc.entries("none_compressible"),
                                                               *tc.CASES["none_compressible"])[0]
    assert tables["index_compressed"]["types"][-1] == 1 and tables["index_raw"]["types"][-1] == 0


def test_keep_rule():
    from lsbm_amd import snappy, sstable
    for raw, comp in rule_pairs():
        want = comp != U64 and comp < ((raw - raw // 8) & U64)
        assert stm.keep_compressed(raw, comp) == want, (raw, comp)
        assert sstable.keep_compressed(raw, comp) == want, (raw, comp)
        assert sstable.keep_compressed(raw, comp - (1 << 64) if comp >> 63 else comp) == want, (raw, comp)
        if comp != U64:  # (snappy.keep_compressed takes real lengths)
            assert bool(snappy.keep_compressed(raw, comp)) == want, (raw, comp)
    assert not stm.keep_compressed(0, 0) and stm.keep_compressed(16, 13) and not stm.keep_compressed(16, 14)


def test_symbols_exported_and_declared(product_lib):
    import re
    from lsbm_amd import _lib
    text = open(os.path.join(os.path.dirname(HERE), "include", "lsbm_table_pack.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(lsbm_\w+)\s*\(", text)))
    assert names == sorted(_lib.TABLE_PACK_SIGNATURES) and len(names) == 3
    for n in names:
        assert hasattr(product_lib, n), n
    assert product_lib.lsbm_block_pack_scratch_bytes(0) >= 8


def test_entry_points_check_arguments(product_lib):
    """A bad argument is LSBM_ERR_INVALID, with or without a device; a good
    call gets past the checks (to the device, or to LSBM_ERR_NO_DEVICE); host
    tensors are refused, nothing is packed on the CPU.  (This module imports
    torch at its top: torch brings a HIP runtime of its own, and a process
    that loads the product library first and torch second, as an unmarked test
    ahead of the GPU tests would, found no device at the library's init.)"""
    from lsbm_amd import _lib, sstable
    L = _lib.lib()
    keep = [np.zeros(64, dtype=np.uint64) for _ in range(10)]
    p = [x.ctypes.data for x in keep]
    need = L.lsbm_block_pack_scratch_bytes(1)

    def plan(**kw):
        return L.lsbm_block_pack_plan_dev(kw.get("raw_len", p[0]), kw.get("comp_len", p[1]), kw.get("n", 1), 0, 5,
                                          kw.get("types", p[2]), kw.get("handles", p[3]), kw.get("end", p[4]),
                                          kw.get("scratch", p[5]), kw.get("scratch_bytes", need), None)

    def pack(**kw):
        return L.lsbm_block_pack_dev(kw.get("raw", p[0]), 64, kw.get("raw_handles", p[1]), kw.get("comp", p[6]), 64,
                                     kw.get("comp_offsets", p[7]), kw.get("types", p[2]), kw.get("handles", p[3]),
                                     kw.get("n", 1), 5, kw.get("out", p[8]), 64, kw.get("status", p[9]),
                                     kw.get("scratch", p[5]), kw.get("scratch_bytes", need), None)

    inv = _lib.LSBM_ERR_INVALID
    for bad in ("raw_len", "types", "handles", "end", "scratch"):
        assert plan(**{bad: None}) == inv, bad
    assert plan(scratch_bytes=need - 1) == inv and plan(scratch=p[5] + 1) == inv
    assert plan(n=(1 << 31) + 1) == inv
    assert plan(types=p[0]) == inv and plan(handles=p[1]) == inv and plan(end=p[0]) == inv  # outputs alias inputs
    for bad in ("raw", "comp", "out", "types", "handles", "status", "scratch"):
        assert pack(**{bad: None}) == inv, bad
    assert pack(scratch_bytes=need - 1) == inv
    assert pack(out=p[0]) == inv and pack(out=p[6]) == inv and pack(status=p[3]) == inv and pack(scratch=p[2]) == inv
    assert pack(status=p[8]) == inv  # outputs alias each other
    if not torch.cuda.is_available():  # (host pointers: only where no kernel can run on them)
        assert plan() == _lib.LSBM_ERR_NO_DEVICE and pack() == _lib.LSBM_ERR_NO_DEVICE
        assert plan(comp_len=None) == _lib.LSBM_ERR_NO_DEVICE
    t = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError):
        sstable.pack_plan(t)
    with pytest.raises(ValueError):
        sstable.read_blocks(torch.zeros(8, dtype=torch.uint8), t)


# ---------------------------------------------------------------- GPU helpers


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: frombuffer views are read-only)


def _image(torch, data):
    return _dev(torch, np.frombuffer(bytes(data) + b"\0", np.uint8))[:len(data)]


def _signed(values):
    return np.array([v - (1 << 64) if v >> 63 else v for v in values], dtype=np.int64)


class Entries:
    """[(key, value)] as the device tensors lsbm_block_decode_dev would write;
    the values sit in an image of their own."""

    def __init__(self, torch, entries):
        koff = np.zeros(len(entries) + 1, dtype=np.int64)
        koff[1:] = np.cumsum([len(k) for k, _ in entries])
        img, values = bytearray(b"\x5a"), []
        for _, v in entries:
            values.append([len(img), len(v)])
            img += v
        self.keys = _image(torch, b"".join(k for k, _ in entries))
        self.koff = _dev(torch, koff)
        self.values = _dev(torch, np.array(values, dtype=np.int64).reshape(-1, 2))
        self.image = _image(torch, img)


def gpu_write(torch, entries, params, compression):
    from lsbm_amd import sstable
    cmp, block_size, restart_interval, bits_per_key = params
    E = Entries(torch, entries)
    image, handles, index_handle = sstable.write_table(E.keys, E.koff, E.values, E.image, cmp, block_size,
                                                       restart_interval, bits_per_key, compression)
    return image.cpu().numpy().tobytes(), handles.cpu().numpy().reshape(-1, 2).tolist(), list(index_handle)


# ---------------------------------------------------------------- GPU: plan


def check_plan(torch, raw, comp, first_offset, gap):
    from lsbm_amd import sstable
    types, handles, end = sstable.pack_plan(_dev(torch, _signed(raw)), None if comp is None else _dev(torch, _signed(comp)),
                                            first_offset, gap)
    wt, wh, wend = stm.pack_plan(raw, comp, first_offset, gap)
    assert types.cpu().tolist() == wt
    assert handles.cpu().numpy().astype(np.uint64).tolist() == [x for h in wh for x in h]
    assert int(end.cpu().numpy().astype(np.uint64)[0]) == wend


@pytest.mark.gpu
def test_gpu_plan_sizes(torch_cuda):
    """n around a tile (256) and one more than a single pass of the second
    level covers (256 tiles of 256); gap 0 and 5; a first offset; no comp_len."""
    rng = np.random.default_rng(0x9A)
    for n in (0, 1, 255, 256, 257, 256 * 256 + 1):
        raw = rng.integers(0, 70000, n).tolist()
        comp = [int(r * f) for r, f in zip(raw, rng.choice([0.3, 0.874, 0.876, 1.1], n))]
        for i in range(0, n, 7):
            comp[i] = U64
        check_plan(torch_cuda, raw, comp, 0, 5)
        check_plan(torch_cuda, raw, comp, 123456789, 0)
        check_plan(torch_cuda, raw, None, 77, 5)


@pytest.mark.gpu
def test_gpu_plan_rule_edges(torch_cuda):
    pairs = rule_pairs()
    check_plan(torch_cuda, [r for r, _ in pairs], [c for _, c in pairs], 3, 5)
    check_plan(torch_cuda, [r for r, _ in pairs], [c for _, c in pairs], 0, 0)


# ---------------------------------------------------------------- GPU: pack

PACK_SMALL = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
PACK_LARGE = (255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 200 * 1024 + 37)


class PackBatch:
    """Blocks of the given (length, source phase, destination phase), sources
    alternating between the two images, destinations in a guarded output."""

    def __init__(self, torch, shapes, gap=5, seed=5):
        rng = np.random.default_rng(seed)
        src = [bytearray(rng.integers(0, 256, 3, dtype=np.uint8).tobytes()) for _ in range(2)]
        self.types, self.raw_handles, self.comp_offsets, self.handles, self.want = [], [], [], [], []
        pos = 64
        for i, (length, sp, dp) in enumerate(shapes):
            t = i % 2
            while len(src[t]) % 16 != sp:
                src[t].append(rng.integers(0, 256))
            so = len(src[t])
            src[t] += rng.integers(0, 256, length, dtype=np.uint8).tobytes()
            while pos % 16 != dp:
                pos += 1
            self.types.append(t)
            self.raw_handles += [so if t == 0 else 0, length]
            self.comp_offsets.append(so if t == 1 else 0)
            self.handles += [pos - 64, length]
            self.want.append((pos, bytes(src[t][so:so + length])))
            pos += length + gap + 64  # 64 guard bytes after every gap
        self.end = pos - 64  # the out_size that just admits the last block and its gap
        self.gap = gap
        self.raw, self.comp = _image(torch, src[0]), _image(torch, src[1])
        self.buffer = torch.full((pos,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0 and self.comp.data_ptr() % 16 == 0 and self.buffer.data_ptr() % 16 == 0
        self.d = [_dev(torch, np.array(x, dtype=dt)) for x, dt in
                  ((self.types, np.uint8), (self.raw_handles, np.int64), (self.comp_offsets, np.int64),
                   (self.handles, np.int64))]

    def run(self, out_size=None, raw=None, comp=None):
        from lsbm_amd import sstable
        types, raw_handles, comp_offsets, handles = self.d
        out = self.buffer[64:64 + (self.end - 64 if out_size is None else out_size)]
        st = sstable.pack(self.raw if raw is None else raw, raw_handles, self.comp if comp is None else comp,
                          comp_offsets, types, handles, out, self.gap)
        return st.cpu().tolist(), self.buffer.cpu().numpy()

    def differs(self, got, skip=()):
        """The blocks (index, length, type) at or after which the buffer is not as expected."""
        bad = np.nonzero(got != self.expected(skip))[0]
        starts = [pos for pos, _ in self.want]
        at = sorted(set(int(np.searchsorted(starts, b, side="right")) - 1 for b in bad[:50]))
        return [(i, len(self.want[i][1]), self.types[i]) if i >= 0 else (i, 0, 0) for i in at]

    def expected(self, skip=()):
        want = np.full(self.buffer.numel(), GUARD, dtype=np.uint8)
        for i, (pos, data) in enumerate(self.want):
            if i not in skip:
                want[pos:pos + len(data)] = np.frombuffer(data, np.uint8)
        return want


@pytest.mark.gpu
def test_gpu_pack_every_phase(torch_cuda):
    """All 16 x 16 source and destination phases for the lengths up to 65, the
    larger lengths at a few phases, sources from both images in one batch; the
    guard bytes before, between and after the blocks stay untouched."""
    shapes = [(n, sp, dp) for n in PACK_SMALL for sp in range(16) for dp in range(16)]
    shapes += [(n, sp, dp) for n in PACK_LARGE for sp, dp in ((0, 0), (0, 7), (5, 0), (3, 3), (13, 2), (1, 15))]
    for gap in (5, 0):
        B = PackBatch(torch_cuda, shapes, gap)
        st, got = B.run()
        assert st == [0] * len(shapes)
        assert B.differs(got) == []


@pytest.mark.gpu
def test_gpu_pack_statuses(torch_cuda):
    torch = torch_cuda
    from lsbm_amd import sstable
    shapes = [(n, (3 * i) % 16, (5 * i + 1) % 16) for i, n in enumerate((100, 4096, 33, 8193, 700, 64))]
    # an out_size one byte short: NO_ROOM for exactly the last block, nothing stored for it
    B = PackBatch(torch, shapes)
    st, got = B.run(out_size=B.end - 64 - 1)
    assert st == [0] * 5 + [sstable.PACK_NO_ROOM]
    assert np.array_equal(got, B.expected(skip=(5,)))
    # a source range one byte past its image: BAD_INPUT for that block only (the
    # last block of each image ends at the image's end)
    B = PackBatch(torch, shapes)
    st, got = B.run(raw=B.raw[:B.raw.numel() - 1])
    assert st == [0] * 4 + [sstable.PACK_BAD_INPUT, 0]
    assert np.array_equal(got, B.expected(skip=(4,)))
    B = PackBatch(torch, shapes)
    st, got = B.run(comp=B.comp[:B.comp.numel() - 1])
    assert st == [0] * 5 + [sstable.PACK_BAD_INPUT]
    assert np.array_equal(got, B.expected(skip=(5,)))
    # type byte 2
    B = PackBatch(torch, shapes)
    B.d[0][2] = 2
    st, got = B.run()
    assert st == [0, 0, sstable.PACK_BAD_INPUT, 0, 0, 0]
    assert np.array_equal(got, B.expected(skip=(2,)))
    # n = 0
    B = PackBatch(torch, [])
    st, got = B.run()
    assert st == [] and np.array_equal(got, B.expected())


# ---------------------------------------------------------------- GPU: write_table


@pytest.mark.gpu
def test_gpu_write_table_equals_fixture(torch_cuda, fx):
    cases, _ = fx
    for name, params in tc.CASES.items():
        data, handles, index_handle = gpu_write(torch_cuda, tc.entries(name), params, 1)
        r = cases[name]
        assert data == r["data"], name
        assert handles == r["data_handles"] and index_handle == r["index_handle"], name


@pytest.mark.gpu
def test_gpu_write_table_without_compression_equals_table_build(torch_cuda):
    from lsbm_amd import block_build
    for name in ("mixed_1024_16", "bloom_internal", "one_entry", "empty", "index_compressed"):
        cmp, block_size, restart_interval, bits_per_key = tc.CASES[name]
        entries = tc.entries(name)
        E = Entries(torch_cuda, entries)
        image, handles, index_handle = block_build.table_build(E.keys, E.koff, E.values.reshape(-1), E.image, cmp,
                                                               block_size, restart_interval, bits_per_key)
        got = gpu_write(torch_cuda, entries, tc.CASES[name], 0)
        assert got[0] == image.cpu().numpy().tobytes(), name
        assert got[1] == handles.cpu().numpy().reshape(-1, 2).tolist() and got[2] == list(index_handle), name
        assert got[0] == bd.table_file(entries, cmp, block_size, restart_interval, bits_per_key)[0], name


@pytest.mark.gpu
def test_gpu_write_table_block_counts(torch_cuda, codec):
    """1, 63, 64, 65 and 129 data blocks (a wave, a wave and one, more than a
    tile's half) of alternating kinds against the model."""
    kinds = "rxxrrrxr" * 17
    for nb in (1, 63, 64, 65, 129):
        entries = tc._blocks_of_kinds(kinds[:nb], 128, 4, 40 + nb)
        want = stm.table_file(entries, bm.BYTEWISE, 128, 4, 10, codec[0])
        assert len(want[1]) == nb and (nb == 1 or len(set(want[3][:nb])) == 2)
        data, handles, index_handle = gpu_write(torch_cuda, entries, (bm.BYTEWISE, 128, 4, 10), 1)
        assert data == want[0], nb
        assert handles == [list(h) for h in want[1]] and index_handle == list(want[2]), nb


# ---------------------------------------------------------------- GPU: read_blocks


def all_handles(table):
    """Every block of a fixture file in file order: data, [filter], metaindex, index."""
    hs = list(table["data_handles"])
    if table["filter_handle"] is not None:
        hs.append(table["filter_handle"])
    return hs + [table["meta_handle"], table["index_handle"]]


def gpu_read(torch, data, handles, **kw):
    from lsbm_amd import sstable
    contents, oh, st = sstable.read_blocks(_image(torch, data), _dev(torch, np.array(handles, dtype=np.int64).reshape(-1)),
                                           **kw)
    c, oh = contents.cpu().numpy().tobytes(), oh.cpu().numpy().reshape(-1, 2).tolist()
    return [c[o:o + s] for o, s in oh], st.cpu().tolist(), contents.numel()


def reseal(data, handle, body=None, typ=None):
    """The file with the block's contents / type byte replaced and its trailer sealed again."""
    off, size = handle
    body = bytes(data[off:off + size]) if body is None else body
    assert len(body) == size
    typ = data[off + size] if typ is None else typ
    return data[:off] + body + bd.trailer(body, typ) + data[off + size + 5:]


@pytest.mark.gpu
def test_gpu_read_blocks(torch_cuda, fx, tables, codec, snappy_oracle):
    torch = torch_cuda
    from lsbm_amd import sstable as ss
    cases, _ = fx
    for name in ("mixed_1024_16", "bloom_internal", "index_compressed", "one_entry", "empty"):
        r, t = cases[name], tables[name]
        hs = all_handles(t)
        assert len(hs) == len(r["types"])
        want = [stm.read_block(r["data"], h, codec[1]) for h in hs]
        assert [w[0] for w in want] == [0] * len(hs) and [w[2] for w in want] == r["types"]
        for verify in (True, False):
            got, st, total = gpu_read(torch, r["data"], hs, verify=verify)
            assert st == [0] * len(hs), name
            assert got == [w[1] for w in want], name
            assert total == sum(len(w[1]) for w in want), name
        assert got[:len(t["blocks"])] == t["blocks"]
    # failures, each between two blocks that stay OK
    r, t = cases["mixed_1024_16"], tables["mixed_1024_16"]
    hs = [tuple(h) for h in r["data_handles"]]
    assert r["types"][:4] == [1, 0, 1, 0]
    good = t["blocks"]

    def check(data, handles, bad, status, **kw):
        got, st, _ = gpu_read(torch, data, handles, **kw)
        assert st == [status if i == bad else 0 for i in range(len(handles))], (st, status)
        assert got == [b"" if i == bad else good[i] for i in range(len(handles))]

    off, size = hs[2]
    flipped = bytearray(r["data"])
    flipped[off + size // 2] ^= 0x10
    check(bytes(flipped), hs, 2, ss.READ_BAD_CHECKSUM, verify=True)
    # the preamble varint changed (one more byte than the stream produces), sealed again
    body = bytearray(r["data"][off:off + size])
    ok, ulen = snappy_oracle.uncompressed_length(bytes(body))
    assert ok and 128 <= ulen < 16384 and body[0] & 0x7F != 0x7F
    body[0] += 1
    ok, _ = snappy_oracle.uncompress(bytes(body))
    assert not ok  # (the expectation is the oracle's, not assumed)
    check(reseal(r["data"], hs[2], bytes(body)), hs, 2, ss.READ_BAD_COMPRESSED)
    # a raw block relabelled as compressed: the oracle decides
    ok, _ = snappy_oracle.uncompress(r["data"][hs[1][0]:hs[1][0] + hs[1][1]])
    if not ok:
        check(reseal(r["data"], hs[1], typ=1), hs, 1, ss.READ_BAD_COMPRESSED)
    check(reseal(r["data"], hs[2], typ=2), hs, 2, ss.READ_BAD_TYPE)
    check(reseal(r["data"], hs[1], typ=2), hs, 1, ss.READ_BAD_TYPE)
    # a handle that reaches past the image (its trailer's last byte is missing)
    short = list(hs)
    short[1] = (len(r["data"]) - 100, 96)
    check(r["data"], short, 1, ss.READ_TRUNCATED)
    short[1] = (-1, 10)
    check(r["data"], short, 1, ss.READ_TRUNCATED)
    # a preamble that claims more than max_bytes: a hostile one, and an honest one under a small limit
    body = bytearray(r["data"][off:off + size])
    assert body[1] < 128  # a two-byte preamble
    hostile = bytes([0xFF, 0xFF, 0xFF, 0xFF, 0x0F]) + bytes(body[5:])
    check(reseal(r["data"], hs[2], hostile), hs, 2, ss.READ_TOO_LARGE)
    check(r["data"], hs[:4], 2, ss.READ_TOO_LARGE, max_bytes=len(good[0]) + len(good[2]) - 1)


# ---------------------------------------------------------------- GPU: table_get


def model_get(t, key, cmp):
    """Table::InternalGet over read_table's blocks: (state, value bytes or None)."""
    r = bm.seek(t["index"], key, cmp, value_is_handle=True)
    if r["state"] != bm.VALID:
        return r["state"], None
    blk = t["blocks"][t["data_handles"].index(r["handle"])]
    s = bm.seek(blk, key, cmp)
    if s["state"] != bm.VALID:
        return s["state"], None
    return bm.VALID, blk[s["value_offset"]:s["value_offset"] + s["value_length"]]


def gpu_get(torch, data, index_handle, keys, cmp, filt=None, **kw):
    from lsbm_amd import sstable
    Q = Entries(torch, [(k, b"") for k in keys])
    res = sstable.table_get(_image(torch, data), index_handle, Q.keys, Q.koff, filter=None if filt is None else
                            _image(torch, filt), cmp=cmp, **kw)
    img, val = res.value_image.cpu().numpy(), res.value.cpu().numpy()
    state = res.state.cpu().tolist()
    values = [img[int(a):int(a) + int(n)].tobytes() if s == 0 else None for (a, n), s in zip(val, state)]
    return state, values, res.value_image.numel()


def absent_keys(entries, cmp):
    out = []
    for k, _ in entries[::3]:
        user = k[:-8] if cmp == bm.INTERNAL_KEY else k
        tag = k[-8:] if cmp == bm.INTERNAL_KEY else b""
        out += [user + b"!" + tag, user[:-1] + tag, bytes([user[0] ^ 0x55]) + user[1:] + tag]
    return out + [b"\xff" * 9 + (b"\0" * 8 if cmp == bm.INTERNAL_KEY else b"")]


@pytest.mark.gpu
def test_gpu_table_get(torch_cuda, fx, tables):
    from lsbm_amd import block
    cases, _ = fx
    for name in ("mixed_256_1", "mixed_4096_16", "index_compressed", "bloom_internal"):
        r, t = cases[name], tables[name]
        cmp = tc.CASES[name][0]
        present = [k for k, _ in t["entries"]]
        absent = absent_keys(t["entries"], cmp)
        want = [model_get(t, k, cmp) for k in present + absent]
        assert [w for w in want[:len(present)]] == [(0, v) for _, v in t["entries"]]
        state, values, _ = gpu_get(torch_cuda, r["data"], r["index_handle"], present + absent, cmp, verify=True)
        assert state == [w[0] for w in want], name
        assert values == [w[1] for w in want], name
        assert block.GET_NEEDS_UNCOMPRESS not in state
        if t["filter"] is not None:
            state, values, _ = gpu_get(torch_cuda, r["data"], r["index_handle"], present + absent, cmp, t["filter"],
                                       verify=True)
            assert state[:len(present)] == [0] * len(present) and values[:len(present)] == [v for _, v in t["entries"]]
            for s, v, w in zip(state[len(present):], values[len(present):], want[len(present):]):
                assert s == block.GET_FILTERED or (s, v) == w
            assert block.GET_FILTERED in state


@pytest.mark.gpu
def test_gpu_table_get_corrupt_block_and_unique_blocks(torch_cuda, fx, tables, snappy_oracle):
    from lsbm_amd import block, sstable
    r, t = fx[0]["mixed_1024_16"], tables["mixed_1024_16"]
    cmp = tc.CASES["mixed_1024_16"][0]
    keys = [k for k, _ in t["entries"]]
    in_block = [i for i, blk in enumerate(t["blocks"]) for _ in stm.block_entries(blk)]
    assert r["types"][2] == 1
    off, size = r["data_handles"][2]
    flipped = bytearray(r["data"])
    flipped[off + size - 1] ^= 1
    state, values, _ = gpu_get(torch_cuda, bytes(flipped), r["index_handle"], keys, cmp, verify=True)
    assert state == [block.GET_BAD_CHECKSUM if b == 2 else 0 for b in in_block]
    assert values == [None if b == 2 else v for b, (_, v) in zip(in_block, t["entries"])]
    body = bytearray(r["data"][off:off + size])
    body[0] += 1
    assert not snappy_oracle.uncompress(bytes(body))[0]
    state, values, _ = gpu_get(torch_cuda, reseal(r["data"], (off, size), bytes(body)), r["index_handle"], keys, cmp)
    assert state == [sstable.GET_BAD_COMPRESSED if b == 2 else 0 for b in in_block]
    assert sstable.GET_BAD_COMPRESSED not in (block.GET_NEEDS_UNCOMPRESS, block.GET_FILTERED, block.GET_BAD_CHECKSUM,
                                              block.GET_BAD_TYPE)
    # 1,000 queries into 3 blocks uncompress 3 blocks
    some = [k for k, b in zip(keys, in_block) if b in (0, 2, 3)]
    queries = [some[i % len(some)] for i in range(1000)]
    state, values, total = gpu_get(torch_cuda, r["data"], r["index_handle"], queries, cmp)
    assert state == [0] * 1000 and values == [dict(t["entries"])[k] for k in queries]
    assert total == sum(len(t["blocks"][b]) for b in (0, 2, 3))


# ---------------------------------------------------------------- GPU: compact


@pytest.mark.gpu
def test_gpu_compact(torch_cuda, fx, codec):
    torch = torch_cuda
    from lsbm_amd import merge, sstable
    _, comp = fx
    c = dict(tc.COMPACTION)
    cmp, max_file_size = c.pop("cmp"), c.pop("max_file_size")
    images = [_image(torch, r["data"]) for r in comp["inputs"]]
    handles = [np.array(r["data_handles"], dtype=np.int64).reshape(-1) for r in comp["inputs"]]
    want = [r["data"] for r in comp["outputs"]]
    out = sstable.compact(images, handles, max_file_size, cmp=cmp, compression=1, **c)
    assert [o.image.cpu().numpy().tobytes() for o in out] == want
    out = sstable.compact(images, None, max_file_size, index_handles=[r["index_handle"] for r in comp["inputs"]],
                          cmp=cmp, compression=1, **c)
    assert [o.image.cpu().numpy().tobytes() for o in out] == want
    # compression=0: merge.compact's output over the uncompressed form of the inputs
    runs = tc.compaction_runs()
    plain = [bd.table_file(run, cmp, c["block_size"], c["restart_interval"], c["bits_per_key"]) for run in runs]
    ref = merge.compact([_image(torch, p[0]) for p in plain],
                        [np.array(p[1], dtype=np.int64).reshape(-1) for p in plain], max_file_size, cmp=cmp, **c)
    raw = sstable.compact(images, handles, max_file_size, cmp=cmp, compression=0, **c)
    assert [o.image.cpu().numpy().tobytes() for o in raw] == [o.image.cpu().numpy().tobytes() for o in ref]
    assert len(raw) != len(out)  # (the cut saw packed sizes)
    # table_get reads the outputs back
    kept, _ = mm.merge_entries(runs, cmp, c["drop"], c["smallest_snapshot"], c["bottom_level"])
    found = []
    for o, f in zip(out, want):
        ents = stm.read_table(f, codec[1])["entries"]
        state, values, _ = gpu_get(torch, f, o.index_handle, [k for k, _ in ents], cmp, verify=True)
        assert state == [0] * len(ents) and values == [v for _, v in ents]
        found += ents
    assert found == kept
