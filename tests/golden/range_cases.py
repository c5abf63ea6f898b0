"""What tests/test_range_query.py and tests/test_range_query_gpu.py share: the
fixture of make_range_fixture.py opened for the model, and seeded random trees
of sorted-table lists over file metadata alone (the plan reads no file).
"""
import json
import os
import random
import struct
import zlib

from golden import buffered_cases as bc
from golden import buffermodel as bfm
from golden import rangemodel as rgm

HERE = os.path.dirname(os.path.abspath(__file__))
BITS = 10  # the bloom of every fixture file


def load_fixture():
    """(index, body) of range_fixture.json / range_tables.bin; body["files"] as bytes."""
    with open(os.path.join(HERE, "range_fixture.json")) as f:
        index = json.load(f)
    with open(os.path.join(HERE, "range_tables.bin"), "rb") as f:
        text = zlib.decompress(f.read())
    assert len(text) == index["bin"]["inflated"] and zlib.crc32(text) == index["bin"]["crc32"]
    body = json.loads(text)
    body["files"] = [bytes.fromhex(h) for h in body["files"]]
    return index, body


case_files = bc.case_files


def case_version(case, files):
    """(ModelVersion, {number: rangemodel.table_blocks result}) of a fixture case, through save_to."""
    items, live, keys, offs = bc.case_added(case, files)
    added = {}
    for i, ((_, kind, level, number, size), alive) in enumerate(zip(items, live)):
        meta = bfm.FileMeta(number, size, keys[offs[2 * i]:offs[2 * i + 1]], keys[offs[2 * i + 1]:offs[2 * i + 2]])
        added.setdefault((level, kind), []).append((meta, alive))
    v = bfm.save_to(added, case["compaction_buffer_length"])
    return v, {n: rgm.table_blocks(rgm.open_range_table(data)) for n, data in files.items()}


def case_queries(case):
    return [(bytes.fromhex(a), bytes.fromhex(b), s) for a, b, s in case["queries"]]


def run_params(run):
    return rgm.RangeParams(run["use_length"], run["buffered_merge"],
                           [bytes.fromhex(c) for c in run["read_cursor_keys"]], bytes.fromhex(run["read_upto_key"]))


# ---------------------------------------------------------------- random trees


def user(i):
    return b"key%05d" % i  # 8 bytes


def ikey(u, seq):
    return u + struct.pack("<Q", (seq << 8) | 1)


def random_table(rng, numbers, sorted_=True):
    """A sorted table of 0..4 files over key000..key059: disjoint ranges in key
    order that may share a boundary user key; or, for Level 0, any ranges in any
    order."""
    files = []
    n = rng.choice((0, 1, 1, 2, 3, 4))
    if sorted_:
        cuts = sorted(rng.randrange(0, 60) for _ in range(2 * n))
        spans = [(cuts[2 * i], cuts[2 * i + 1]) for i in range(n)]
    else:
        spans = [tuple(sorted((rng.randrange(0, 60), rng.randrange(0, 60)))) for _ in range(n)]
    for i, (lo, hi) in enumerate(spans):
        numbers[0] += 1
        # (sequences that fall along the table: two files that share a boundary user key stay in order)
        files.append(bfm.FileMeta(numbers[0], 1000 + numbers[0], ikey(user(lo), 200 - 10 * i),
                                  ikey(user(hi), 195 - 10 * i)))
    return files


def random_tree(rng, max_tables=4):
    """({(level, type): [[FileMeta]]}, RangeParams): lists of 1..max_tables + 1
    sorted tables; heads of the buffer lists that are not empty among them
    (which SaveTo cannot produce)."""
    numbers = [100]
    lists = {}
    for level in range(4):
        for kind in range(4):
            if level == 0:
                lists[(0, kind)] = [random_table(rng, numbers, sorted_=False)] if kind < 2 else [[]]
            elif kind < 2:
                lists[(level, kind)] = [random_table(rng, numbers)]
            else:
                head = random_table(rng, numbers) if rng.random() < 0.25 else []
                lists[(level, kind)] = [head] + [random_table(rng, numbers)
                                                 for _ in range(rng.randrange(0, max_tables + 1))]
    use = [rng.choice((0, 0, 1, 2, 3, max_tables, max_tables + 2)) for _ in range(4)]
    cursors = [rng.choice((b"", user(rng.randrange(0, 60)), b"key", b"zz")) for _ in range(4)]
    upto = rng.choice((b"", b"zz", b"zz", user(rng.randrange(0, 60)), user(rng.randrange(0, 60)) + b"\x00"))
    return lists, rgm.RangeParams(use, rng.random() < 0.8, cursors, upto)


def random_queries(rng, n):
    """[(start, end)]: start keys of 8 bytes and longer (FindFile then reads a
    user key and a tag out of them), ends of 8 bytes and longer either side of
    the starts."""
    out = []
    for _ in range(n):
        a = rng.randrange(0, 60)
        start = user(a) + rng.choice((b"", b"", b"\x00", b"\x00" * 8, b"\xff" * 8, user(rng.randrange(0, 60))))
        b = rng.choice((a, a, a + rng.randrange(0, 5), a + rng.randrange(0, 30), rng.randrange(0, 60)))
        end = rng.choice((user(b), user(b), user(b) + b"\x00", user(b)[:7] + b"\x00", user(b)[:4] + b"\xff" * 4))
        out.append((start, end))
    return out
