"""What tests/test_memtable.py and tests/test_memtable_gpu.py share: the
fixture of make_memtable_fixture.py read back, and seeded WriteBatch payloads.
"""
import json
import os
import struct
import zlib

G = os.path.dirname(os.path.abspath(__file__))


def _records(blob, span, n):
    """n (key, value) records stored as u32 length + bytes each."""
    p, out = span[0], []
    for _ in range(n):
        kv = []
        for _ in range(2):
            ln = struct.unpack_from("<I", blob, p)[0]
            kv.append(bytes(blob[p + 4:p + 4 + ln]))
            p += 4 + ln
        out.append(tuple(kv))
    assert p == sum(span)
    return out


def load():
    """(cases, malformed): a case is a dict with name, block_size,
    restart_interval, bits_per_key, log (bytes), record_lens, iteration
    [(internal key, value)] and table (bytes or None); a malformed case has
    name, payloads [bytes], statuses [str] and iteration."""
    fx = json.load(open(os.path.join(G, "memtable_fixture.json")))
    blob = zlib.decompress(open(os.path.join(G, "memtable_tables.bin"), "rb").read())
    assert len(blob) == fx["inflated_bytes"]
    cut = lambda span: bytes(blob[span[0]:span[0] + span[1]])  # noqa: E731
    cases = [dict(c, log=cut(c["log"]), iteration=_records(blob, c["iteration"], c["n_entries"]),
                  table=cut(c["table"]) if c["table"] else None) for c in fx["cases"]]
    bad = [dict(m, payloads=[bytes.fromhex(x) for x in m["payloads"]],
                iteration=_records(blob, m["iteration"], m["n_entries"])) for m in fx["malformed"]]
    return cases, bad


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def batch(seq, ops, count=None):
    """A WriteBatch::rep_: ops are (type, user key, value)."""
    b = struct.pack("<QI", seq, len(ops) if count is None else count)
    for t, k, v in ops:
        b += bytes([t]) + varint(len(k)) + k + (varint(len(v)) + v if t else b"")
    return b


def random_payload(rng):
    """A batch of a few entries that is, about half the time, damaged: cut
    short, a byte overwritten (tags, varints and counts among them), or a
    long varint put in."""
    n = rng.randrange(0, 9)
    ops = [(rng.choice((0, 1, 1)), bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 3, 8, 20, 130)))),
            bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 5, 127, 128, 300))))) for _ in range(n)]
    b = bytearray(batch(rng.randrange(1 << 56), ops))
    how = rng.randrange(8)
    if how == 0:
        b = b[:rng.randrange(len(b) + 1)]
    elif how == 1 and len(b) > 12:
        b[rng.randrange(12, len(b))] = rng.choice((0, 1, 2, 0x80, 0xFF, rng.randrange(256)))
    elif how == 2:
        b[8] = (b[8] + rng.choice((1, 255))) & 255
    elif how == 3:
        at = rng.randrange(12, len(b) + 1)
        b[at:at] = bytes([rng.choice((0, 1))]) + bytes(rng.choice((0x80, 0x81, 0xFF)) for _ in range(rng.randrange(1, 5))) \
            + bytes([rng.choice((0x00, 0x01, 0x10, 0x70, 0x80))])
    return bytes(b)
