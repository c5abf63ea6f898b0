"""What tests/test_buffered.py and tests/test_buffered_gpu.py share: the
fixture of make_buffered_fixture.py opened for the model, and seeded random
trees of sorted-table lists over a pool of small table files built by the
models' own table writer.
"""
import json
import os
import random
import struct
import zlib

from golden import buffermodel as bfm
from golden import getmodel as gm
from golden import memtablemodel

HERE = os.path.dirname(os.path.abspath(__file__))
BITS = 10  # the bloom of every file here


def load_fixture():
    """(index, body) of buffered_fixture.json / buffered_tables.bin; body["files"] as bytes."""
    with open(os.path.join(HERE, "buffered_fixture.json")) as f:
        index = json.load(f)
    with open(os.path.join(HERE, "buffered_tables.bin"), "rb") as f:
        text = zlib.decompress(f.read())
    assert len(text) == index["bin"]["inflated"] and zlib.crc32(text) == index["bin"]["crc32"]
    body = json.loads(text)
    body["files"] = [bytes.fromhex(h) for h in body["files"]]
    return index, body


def case_files(body, case):
    """{number: file bytes} of a fixture case."""
    return {int(n): body["files"][at] for n, at in case["files"].items()}


def case_added(case, files):
    """Builder::Apply (lsbm/version_set.cc:1660-1683) over the case's records:
    (items, live, keys, key_offsets) in the shape of manifest.recover's edits --
    items rows (record, type, level, number, file_size) in added order."""
    items, keys, deleted = [], [], set()
    for r, rec in enumerate(case["records"]):
        for kind, level, number in rec["deleted"]:
            deleted.add((kind, level, number))
        for kind in range(4):  # (EncodeTo writes the new files type by type)
            for t, level, number, a, b in rec["new"]:
                if t != kind:
                    continue
                deleted.discard((kind, level, number))
                items.append((r, kind, level, number, len(files.get(number, b""))))
                keys += [bytes.fromhex(a), bytes.fromhex(b)]
    live = [(kind, level, number) not in deleted for _, kind, level, number, _ in items]
    offs = [0]
    for key in keys:
        offs.append(offs[-1] + len(key))
    return items, live, b"".join(keys), offs


def case_version(case, files, verify=True):
    """(ModelVersion, {number: opened table}) of a fixture case, through save_to."""
    items, live, keys, offs = case_added(case, files)
    added = {}
    for i, ((_, kind, level, number, size), alive) in enumerate(zip(items, live)):
        meta = bfm.FileMeta(number, size, keys[offs[2 * i]:offs[2 * i + 1]], keys[offs[2 * i + 1]:offs[2 * i + 2]])
        added.setdefault((level, kind), []).append((meta, alive))
    v = bfm.save_to(added, case["compaction_buffer_length"])
    return v, {n: gm.open_table(data, BITS, None, verify) for n, data in files.items()}


def run_params(run):
    return bfm.Params(run["use_length"], run["buffered_merge"], [bytes.fromhex(c) for c in run["read_cursor_keys"]])


def set_visible(v, run):
    """FileMetaData::visible as the run sets it: all true but the named files."""
    hidden = {(level, kind, number) for level, kind, number in run["invisible"]}
    for (level, kind), tables in v.lists().items():
        for table in tables:
            for f in table:
                f.visible = (level, kind, f.number) not in hidden


# ---------------------------------------------------------------- random trees

RANGES = ((0, 20), (20, 40), (40, 60))


def user(i):
    return b"k%02d" % i


def damage_index(data):
    """The index block's restart count set to 0xffffffff (the trailer's CRC left as it is: open without verify)."""
    index_handle = gm.stm.decode_footer(data)[1]
    at = index_handle[0] + index_handle[1] - 4
    return data[:at] + b"\xff\xff\xff\xff" + data[at + 4:]


def pool(seed=1, per_range=10):
    """[(number, range index, file bytes, smallest, largest)]: small tables with
    filters over random subsets of three key ranges; values name the file; some
    entries are deletions; the last file of each range has a damaged index."""
    rng = random.Random(seed)
    out, number = [], 100
    for r, (lo, hi) in enumerate(RANGES):
        for j in range(per_range):
            number += 1
            ents = []
            for i in range(lo, hi):
                if rng.random() < 0.55:
                    seq = rng.randrange(1, 200)
                    kind = 0 if rng.random() < 0.15 else 1
                    ents.append((user(i), seq, kind))
            if not ents:
                ents.append((user(lo), 7, 1))
            ents.sort(key=lambda e: (e[0], -e[1]))
            kv = [(u + struct.pack("<Q", (s << 8) | t), b"f%d:" % number + u if t else b"") for u, s, t in ents]
            data = memtablemodel.table_file(kv, 256, 4, BITS)
            if j == per_range - 1:
                data = damage_index(data)
            out.append((number, r, data, kv[0][0], kv[-1][0]))
    return out


def random_tree(rng, files, max_tables=5, sentinel=True):
    """({(level, type): [[FileMeta]]}, Params, [(user key, sequence)]): lists of
    up to max_tables sorted tables, each at most one pool file per key range;
    with `sentinel`, heads of the buffer lists that are not empty (which SaveTo
    cannot produce), lists of one table, and invisible files."""
    by_range = [[f for f in files if f[1] == r] for r in range(len(RANGES))]

    def table(p=0.7):
        return [bfm.FileMeta(f[0], len(f[2]), f[3], f[4], visible=rng.random() < 0.85)
                for f in (rng.choice(pool_r) for pool_r in by_range) if rng.random() < p]

    lists = {}
    for level in range(4):
        for kind in range(4):
            if level == 0:
                if kind == 0:
                    n = rng.randrange(0, 4)
                    lists[(0, 0)] = [[m for t in (table(0.5) for _ in range(n)) for m in t]]
                elif kind == 1:
                    lists[(0, 1)] = [table(0.5)]
                else:
                    lists[(0, kind)] = [[]]
                continue
            if kind in (0, 1):
                lists[(level, kind)] = [table(0.8)]
                continue
            n = rng.randrange(0, max_tables + 1)
            tables = [table() if rng.random() < 0.85 else [] for _ in range(n)]
            head = table() if sentinel and rng.random() < 0.2 else []
            lists[(level, kind)] = [head] + tables
    use = [0] + [rng.choice((0, 0, 1, 2, 3, max_tables, max_tables + 5)) for _ in range(3)]
    cursors = [rng.choice((b"", user(rng.randrange(0, 60)), user(rng.randrange(0, 60))[:2], b"zz")) for _ in range(4)]
    params = bfm.Params(use, rng.random() < 0.8, cursors)
    return lists, params


def random_queries(rng, n):
    return [(rng.choice((user(rng.randrange(0, 60)), user(rng.randrange(0, 60)), b"k", b"k6", b"")),
             rng.choice((1000, 1000, rng.randrange(0, 220)))) for _ in range(n)]
