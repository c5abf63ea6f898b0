"""The scenarios of the memtable-switch fixture (tests/golden/memcut_fixture.*):
for each a name and the log's records as WriteBatch reps.  The fixture maker
feeds them to the reference and the tests rebuild the same bytes, so only the
reference's results are stored.  Entry sizes are chosen with the model's arena
so that each scenario meets the allocator where its name says; what the
reference then reports is recorded, not assumed.
"""
import random
import struct

from . import memcutmodel as mm
from .writemodel import put_varint32

# write_buffer_size values every scenario is cut with, in both modes.  16
# standard blocks are 65,536 + 8 * 16 = 65,664 bytes of usage.
WRITE_BUFFER_SIZES = (4104, 8192, 65536, 65600, 65664, 4 << 20)
HEIGHT12_DRAW = 1338279  # the draw that ends the first height-12 insert from the fixed seed
HEIGHT12_INSERT = 1003046


def key_of(i, n):
    """n key bytes for the i-th entry of a scenario."""
    return (b"%08d" % i * (n // 8 + 1))[:n]


def value_of(i, n):
    return bytes([97 + i % 26]) * n


def rep_of(seq, ops, count=None):
    """A WriteBatch rep: ops are (type, key length, value length)."""
    out = bytearray(struct.pack("<QI", seq, len(ops) if count is None else count))
    for j, (t, kl, vl) in enumerate(ops):
        out.append(t)
        out += put_varint32(kl) + key_of(seq + j, kl)
        if t:
            out += put_varint32(vl) + value_of(seq + j, vl)
    return bytes(out)


class Design:
    """Ops for one memtable, with the model's arena alongside to aim sizes."""

    def __init__(self):
        self.arena, self.rnd, self.ops = mm.Arena(), mm.SEED, []
        self.arena.allocate_aligned(8 + 8 * mm.MAX_HEIGHT)

    def add(self, kl, vl, t=1):
        self.ops.append((t, kl, vl))
        self.arena.allocate(mm.entry_size(kl + 8, vl if t else 0))
        h, self.rnd = mm.random_height(self.rnd)
        self.arena.allocate_aligned(8 + 8 * h)
        return self

    def node(self):
        return 8 + 8 * mm.random_height(self.rnd)[0]

    def add_size(self, size, kl=8):
        """A Put whose encoded length is exactly `size`."""
        for lv in (1, 2, 3):
            vl = size - (1 + kl + 8) - lv
            if vl >= 0 and len(put_varint32(vl)) == lv:
                return self.add(kl, vl)
        raise ValueError(size)

    def leave(self, remaining):
        """A Put that fits and leaves `remaining` bytes (a multiple of 8) in the block."""
        assert self.arena.remaining - remaining - self.node() >= 32, (self.arena.remaining, remaining)
        return self.add_size(self.arena.remaining - remaining - self.node())


def _records(ops, counts, seq=1):
    """The ops split into records of the given entry counts (the last count repeats)."""
    out, at, i = [], 0, 0
    while at < len(ops):
        c = counts[min(i, len(counts) - 1)]
        out.append(rep_of(seq + at, ops[at:at + c]))
        at, i = at + max(c, 1), i + 1
    return out


def scenarios():
    """[(name, [rep, ...])]"""
    rng = random.Random(0x3E3C07)
    out = []
    out.append(("empty_batch", [rep_of(1, [])]))
    for n in (0, 1, 255, 256, 257):
        ops = [(1, 16, 100)] * n
        out.append((f"one_record_{n}", [rep_of(1, ops)]))
    # the arena's corners, one entry a record so that every step is recorded
    d = Design()
    d.leave(3600)
    d.add_size(3000)  # above a quarter block, fits
    d.leave(200)
    d.add_size(200 - d.node())  # cost == remaining exactly
    assert d.arena.remaining == 0
    d.add(16, 100)  # a new block
    d.leave(2048)
    d.add_size(1025)  # fits
    d.leave(40)
    d.add_size(40)  # the key fits, its node does not
    d.leave(1016)
    d.add_size(1024)  # does not fit, not above a quarter block: a new block
    d.leave(1016)
    d.add_size(1025)  # does not fit, above: a block of its own
    d.leave(40)
    for size in (2000, 1025, 5000, 1100):  # oversized in a row; within three of them a node does not fit
        d.add_size(size)
    d.add(16, 100).add(16, 100)
    out.append(("arena_corners", _records(d.ops, [1])))
    # varint lengths of key and value
    ops = [(1, kl, 10) for kl in (0, 1, 119, 120, 121, 300)] + \
          [(1, 8, vl) for vl in (0, 127, 128, 16383, 16384, 17000)] + [(0, 119, 0), (0, 120, 0)]
    out.append(("varint_edges", _records(ops, [1])))
    out.append(("deletions", _records([(rng.randrange(2), rng.randrange(0, 41), rng.randrange(0, 200))
                                       for _ in range(600)], [3, 1, 7])))
    # enough standard blocks to pass n_blocks = 2, 3, 5, 9, 17, 33; at 65,600 the vector's capacity decides
    out.append(("blocks_33", _records([(1, 16, 100)] * 1100, [1])))
    out.append(("five_memtables", _records([(1, 23, 100)] * 2600, [5, 1, 40])))
    out.append(("mixed_sizes", _records([(int(rng.randrange(8) > 0), rng.randrange(0, 41),
                                          rng.choice((0, 10, 100, 100, 100, 900, 1100, 5000)))
                                         for _ in range(700)], [2, 9, 1, 30])))
    # records RecoverLogFile drops, before, between and after; and records in error that keep entries, the
    # first of them after the first cut at 64 KiB
    small = [b"", b"short", bytes(11)]
    good = _records([(1, 16, 100)] * 1200, [10])
    bad_put = rep_of(5000, [(1, 16, 100), (1, 16, 100)], count=3) + b"\x01\x04key!\x7f"  # value runs past the end
    wrong_count = rep_of(6000, [(1, 16, 100)] * 4, count=9)
    unknown_tag = rep_of(7000, [(0, 5, 0)]) + b"\x07"
    out.append(("too_small", small[:2] + good[:7] + small + good[7:20] + [small[1]]))
    out.append(("records_in_error", good[:60] + [bad_put] + good[60:80] + [wrong_count, small[0], unknown_tag] + good[80:]))
    # a cut on the last record at 65,536 (blocks_33 cut short where the 16th block arrives)
    ops, d = [], Design()
    while d.arena.usage() <= 65536:
        d.add(16, 100)
    out.append(("cut_on_last", _records(d.ops, [1])))
    # batches DBImpl::BuildBatchGroup cannot merge (each above 512 KiB, so two pass the 1 MiB cap): as writers each
    # is its own group, and WRITE switches before every one at 64 KiB and before every eighth or so at 4 MiB
    out.append(("big_batches", _records([(1, 16, 16500 + 100 * (i % 5)) for i in range(20 * 32)], [32])))
    return out


def entries_of(ops_per_record):
    """(entries [(ikl, vl, type)], entry_base) from per-record [(klen, vlen, type)]."""
    entries, base = [], [0]
    for ops in ops_per_record:
        entries += [(kl + 8, vl, t) for kl, vl, t in ops]
        base.append(len(entries))
    return entries, base
