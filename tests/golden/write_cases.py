"""What tests/golden/make_write_fixture.py, tests/test_write.py and
tests/test_write_gpu.py share: the write and log cases as specs, the byte
pattern their keys, values and payloads are made of, and the fixture read back.

An op spec is (type, klen, kseed, vlen, vseed); a writer spec (sync, [op spec]);
a write case (name, last_sequence, [writer spec]).  A log case is (name,
[(length, seed)]).  pattern(seed, n) has period 251, so the fixture deflates
to little and a copy that is off by a multiple of 16 still differs.
"""
import json
import os
import random
import zlib

G = os.path.dirname(os.path.abspath(__file__))
B, H = 32768, 7
P = B - H
LENGTHS = [0, 1, 127, 128, 16383, 16384, 2097151, 2097152]  # each varint width, and its last value


def pattern(seed, n):
    p = bytes((seed + i) % 251 for i in range(251))
    return (p * (n // 251 + 1))[:n]


def ops_of(op_specs):
    """[(type, key, value)] of [(type, klen, kseed, vlen, vseed)]."""
    return [(t, pattern(ks, kl), pattern(vs, vl) if t else b"") for t, kl, ks, vl, vs in op_specs]


def writers_of(writer_specs):
    """[(ops, sync)]."""
    return [(ops_of(ops), bool(sync)) for sync, ops in writer_specs]


def sized(byte_size, seed=0, sync=0):
    """A writer whose batch is one Put of a 1-byte key with ByteSize exactly
    byte_size (16, 17, ... ; not 143..144 and the like where the value's varint
    grows: asserted)."""
    for vlen_bytes in (1, 2, 3, 4):
        vl = byte_size - 12 - 3 - vlen_bytes
        if vl >= 0 and len(_varint(vl)) == vlen_bytes:
            return (sync, [(1, 1, seed, vl, seed + 1)])
    raise AssertionError(byte_size)


def _varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def write_specs():
    rng = random.Random(0x77A17E)
    cases = []
    # every varint width of a key and of a value, Deletes beside Puts, an empty batch, one op
    ws = [(0, [])]
    for i, ln in enumerate(LENGTHS):
        ws.append((0, [(1, ln, i, 3, 100 + i), (0, ln, 7 * i + 1, 0, 0), (1, 5, 3 * i, ln, 50 + i)]))
    ws += [(0, [(1, 3, 9, 4, 10)]), (0, []), (0, [(0, 2, 1, 0, 0)])]
    cases.append(("encoding", 0x0123456789AB, ws))
    # 65 and 257 ops: a wave and a workgroup of lanes, and one more; short ops at every source and destination phase
    small = lambda: (rng.choice((0, 1, 1)), rng.randrange(0, 41), rng.randrange(251), rng.randrange(0, 200),  # noqa: E731
                     rng.randrange(251))
    cases.append(("ops_65_257", 0, [(0, [small() for _ in range(65)]), (0, [small() for _ in range(257)]),
                                    (0, [small() for _ in range(1)])]))
    cases.append(("one_writer", 41, [(1, [small() for _ in range(3)])]))
    # the group rule
    cases.append(("leader_131072_exact", 5, [sized(131072, 1), sized(131072, 2), sized(16, 3), sized(20, 4)]))
    cases.append(("leader_131072_one_above", 5, [sized(131072, 1), sized(131073, 2), sized(16, 3)]))
    cases.append(("leader_131073_exact", 5, [sized(131073, 1), sized((1 << 20) - 131073, 2), sized(16, 3), sized(16, 4)]))
    cases.append(("leader_131073_one_above", 5, [sized(131073, 1), sized((1 << 20) - 131072, 2), sized(16, 3)]))
    cases.append(("leader_above_1mib", 5, [sized((1 << 20) + 1, 1), sized(16, 2), sized(16, 3), sized(40, 4)]))
    # bodies that fit max_size = 1000 + 131072 where the ByteSize sums (12 more per batch) do not
    cases.append(("header_counting", 9, [sized(1000, 0)] + [sized(1311, i + 1) for i in range(101)]))
    # sync: a non-sync leader stops before a sync writer, a sync leader takes both kinds, all sync
    tiny = lambda s: (s, [small() for _ in range(rng.randrange(0, 3))])  # noqa: E731
    cases.append(("sync_mixed", 1000, [tiny(s) for s in (0, 0, 1, 0, 1, 1, 0, 0, 0, 1)]))
    cases.append(("sync_all", 1000, [tiny(1) for _ in range(6)]))
    cases.append(("sync_leader_takes_both", 1000, [tiny(s) for s in (1, 0, 1, 0, 0)]))
    # 1,025 writers in groups of a few: the chain's staged links turn over
    cases.append(("writers_1025", 1 << 40, [tiny(rng.choice((0, 0, 1))) for _ in range(1025)]))
    return cases


def _leaving(lens, r):
    """lens + one record that ends r bytes before its block does."""
    off = _end(lens)
    room = B - off % B - H - r
    if room < 0:
        lens = lens + [40]
        off = _end(lens)
        room = B - off % B - H - r
    return lens + [room]


def _end(lens, off=0):
    from golden import writemodel as wm
    return wm.add_records([bytes(n) for n in lens], off)[3]


def log_specs():
    rng = random.Random(0x106)
    named = [0, 1, 6, 7, 8, P - 8, P - 7, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 5 * P + 3]
    mixed = []
    for n in named:
        mixed += [n, rng.randrange(1, 60)]
    cases = [("lengths", mixed)]
    ends = []
    for r in range(8):  # each pad width, and (r == 7) the zero-length FIRST
        ends = _leaving(ends, r) + [rng.randrange(1, 30)]
    for r in range(8):  # ... followed by a zero-length record, and by a long one
        ends = _leaving(ends, r) + [0 if r % 2 else P + 5]
    cases.append(("ends", ends))
    # records that end exactly on a block end as record 0 and record 63 of a run of 64, and in consecutive records
    ev = _leaving([], 0)
    ev += [rng.randrange(1, 50) for _ in range(62)]
    ev = _leaving(ev, 0)
    ev = _leaving(ev, 0) + [P, P, 3]
    ev = _leaving(ev, 3)
    ev = _leaving(ev, 7) + [0, 0, 5]
    cases.append(("events", ev))
    cases.append(("ten_P", [P] * 10))
    cases.append(("short_130", [rng.randrange(0, 41) for _ in range(130)]))
    tail = [5, P + 1, 0, 40]
    # a record boundary at file offset P, B - 6, B - 1, B, B + 7 and mid-block: log_offset for what follows
    for name, head in (("offset_P", [P - 7]), ("offset_B-6", [B - 13]), ("offset_B-1", [B - 8]), ("offset_B", [P]),
                       ("offset_B+7", [P, 0]), ("offset_mid", [1000])):
        cases.append((name, head + tail))
    return [(name, [(n, (i * 37) % 251) for i, n in enumerate(lens)]) for name, lens in cases]


def load():
    """(writes, logs).  A write case: name, last_sequence, writers (specs),
    group_first, reps [bytes], log (bytes).  A log case: name, payloads (specs),
    log (bytes)."""
    fx = json.load(open(os.path.join(G, "write_fixture.json")))
    blob = zlib.decompress(open(os.path.join(G, "write_fixture.bin"), "rb").read())
    assert len(blob) == fx["inflated_bytes"]
    cut = lambda span: bytes(blob[span[0]:span[0] + span[1]])  # noqa: E731
    writes = [dict(c, reps=[cut(r) for r in c["reps"]], log=cut(c["log"])) for c in fx["writes"]]
    logs = [dict(c, log=cut(c["log"])) for c in fx["logs"]]
    return writes, logs
