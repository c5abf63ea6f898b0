"""The inputs of tests/golden/snappy_tables.json: seeded entries per case, shared
by the generator (make_snappy_table_fixture.py) and tests/test_sstable.py.  The
expected files are in the fixture; nothing here compresses anything.
"""
from golden import buildmodel as bd
from golden import mergemodel as mm
from golden.blockmodel import BYTEWISE, INTERNAL_KEY
from golden.splitmix import stream_bytes

# name -> (cmp, block_size, restart_interval, bits_per_key)
CASES = {}
for _bs in (256, 1024, 4096):
    for _ri in (1, 16):
        CASES[f"mixed_{_bs}_{_ri}"] = (BYTEWISE, _bs, _ri, None)
CASES.update({
    "all_compressible": (BYTEWISE, 1024, 16, None),
    "none_compressible": (BYTEWISE, 256, 16, None),
    "index_compressed": (BYTEWISE, 32, 16, None),
    "index_raw": (BYTEWISE, 256, 16, None),
    "bloom_internal": (INTERNAL_KEY, 512, 16, 10),
    "one_entry": (INTERNAL_KEY, 4096, 16, 10),
    "empty": (INTERNAL_KEY, 4096, 16, None),
})

COMPACTION = dict(cmp=INTERNAL_KEY, max_file_size=800, drop=True, smallest_snapshot=40, bottom_level=True,
                  block_size=256, restart_interval=4, bits_per_key=10)


def _random(seed, n):
    """n random bytes; consecutive seeds give disjoint pieces of one stream."""
    return stream_bytes(0x5AB1E, 4096 * seed, n).tobytes()


def _closed(entries, block_size, restart_interval):
    """The last Add flushed: the next entry would open a block."""
    first, _ = bd.plan([(k, len(v)) for k, v in entries] + [(b"\xff", 0)], block_size, restart_interval)
    return first[-2] == len(entries)


def _blocks_of_kinds(kinds, block_size, restart_interval, seed):
    """Entries that fill one data block per kind: 'r' values of one repeated
    byte, 'x' values of random bytes."""
    entries, vlen = [], max(8, block_size // 5)
    for b, kind in enumerate(kinds):
        while True:
            i = len(entries)
            value = bytes([97 + i % 26]) * vlen if kind == "r" else _random(seed + i, vlen)
            entries.append((b"%05d" % i, value))
            if _closed(entries, block_size, restart_interval):
                break
    return entries


def entries(name):
    cmp, block_size, restart_interval, _ = CASES[name]
    if name.startswith("mixed_"):
        return _blocks_of_kinds("rxrxrx" if block_size < 4096 else "rxrx", block_size, restart_interval, 1000 + block_size)
    if name == "all_compressible":
        return _blocks_of_kinds("rrrrrr", block_size, restart_interval, 0)
    if name == "none_compressible":
        return _blocks_of_kinds("xxxx", block_size, restart_interval, 77)
    if name == "index_compressed":  # one entry a block, long similar keys
        return [(b"tenant-0001/table-orders/row-%08d" % (7 * i), b"v%03d" % (i % 1000)) for i in range(300)]
    if name == "index_raw":  # three blocks whose separators share nothing
        out = []
        for i in range(9):
            out.append((bytes([40 + 20 * i]) + _random(500 + i, 11), _random(600 + i, 90)))
        return out
    if name == "bloom_internal":  # half of every value repeats: kept compressed, and the offsets move a lot
        return [(mm.internal_key(b"user%05d" % i, 1000 - i), bytes([65 + i % 26]) * 60 + _random(900 + i, 40))
                for i in range(110)]
    if name == "one_entry":
        return [(mm.internal_key(b"only", 5), b"value")]
    if name == "empty":
        return []
    raise KeyError(name)


def compaction_runs():
    """Three sorted runs with overlapping user keys, a deletion below the
    snapshot, versions on both sides of it."""
    def value(i, r):
        return bytes([48 + (i + r) % 10]) * 50 + _random(3000 + 10 * i + r, 14)

    run0 = [(mm.internal_key(b"k%04d" % i, 90 + i % 5), value(i, 0)) for i in range(0, 60, 2)]
    run1 = [(mm.internal_key(b"k%04d" % i, 30 + i % 5), value(i, 1)) for i in range(0, 60, 3)]
    run2 = [(mm.internal_key(b"k%04d" % i, 10 + i % 5), value(i, 2)) for i in range(0, 60)]
    run1[4] = (mm.internal_key(b"k%04d" % 12, 35, mm.TYPE_DELETION), b"")
    return [run0, run1, run2]
