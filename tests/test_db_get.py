"""The plain-Python model of the read path (tests/golden/getmodel.py) against
the reference's own results (tests/golden/get_fixture.json, get_tables.bin,
written by tests/golden/make_get_fixture.py from lsbm's MemTable::Get, FindFile,
TableCache::Get / ContainKey / SkipFilterGet and ParseInternalKey): every
MemTable::Get result, every FindFile index with the tests beside it, every saver
call and every final status and value.  CPU only; the GPU Get is compared with
the same fixture and the same model in tests/test_db_get_gpu.py.
"""
import json
import os
import random
import struct
import zlib

import pytest

from golden import getmodel as gm

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(HERE, "golden", "get_fixture.json")) as f:
        fixture = json.load(f)
    with open(os.path.join(HERE, "golden", "get_tables.bin"), "rb") as f:
        blob = zlib.decompress(f.read())
    assert len(blob) == fixture["inflated_bytes"]

    def inflate(rec):  # `<name>_at`: a list kept as JSON text in the stream
        for key in [k for k in rec if k.endswith("_at")]:
            at, size = rec.pop(key)
            rec[key[:-3]] = json.loads(blob[at:at + size])
    inflate(fixture)
    for kind in ("memtables", "find_file", "versions"):
        for rec in fixture[kind]:
            inflate(rec)
    return fixture, blob


def iteration(blob, pair, n):
    """[(internal key, value)] of a recorded memtable iteration."""
    buf, p, out = blob[pair[0]:pair[0] + pair[1]], 0, []
    for _ in range(n):
        kv = []
        for _ in range(2):
            ln = struct.unpack_from("<I", buf, p)[0]
            kv.append(bytes(buf[p + 4:p + 4 + ln]))
            p += 4 + ln
        out.append(tuple(kv))
    assert p == len(buf)
    return out


def memtable_of(batches):
    """The sorted memtable of fixture batches [[sequence, [[type, key hex, value hex]]]]."""
    from golden import memtablemodel as mt
    keys, values = [], []
    for seq, ops in batches:
        for i, (t, k, v) in enumerate(ops):
            keys.append(bytes.fromhex(k) + struct.pack("<Q", ((seq + i) << 8) | t))
            values.append(bytes.fromhex(v))
    return [(keys[i], values[i]) for i in mt.order(keys)]


def codec(snappy_oracle):
    def uncompress(c):
        ok, out = snappy_oracle.uncompress(c)
        return out if ok else None
    return uncompress


def open_version(v, blob, uncompress):
    """(memtables, tables, bounds, runs, visible) of a fixture version for getmodel.version_get."""
    bits = 10 if v["filter_policy"] else None
    tables = [gm.open_table(blob[f["file"][0]:f["file"][0] + f["file"][1]], bits, uncompress) for f in v["files"]]
    bounds = [(bytes.fromhex(f["smallest"]), bytes.fromhex(f["largest"])) for f in v["files"]]
    runs = [(idx, flags) for flags, idx in v["runs"]]
    return [memtable_of(m) for m in v["memtables"]], tables, bounds, runs, [f["visible"] for f in v["files"]]


def test_model_reproduces_memtable_get(fx):
    fixture, blob = fx
    assert [m["n_entries"] for m in fixture["memtables"]][:6] == [0, 1, 2, 255, 256, 257]
    seen = set()
    for m in fixture["memtables"]:
        entries = iteration(blob, m["iteration"], m["n_entries"])
        for khex, seq, got, status, vhex in m["queries"]:
            verdict, value = gm.memtable_get(entries, bytes.fromhex(khex), seq)
            assert (verdict != gm.UNDECIDED) == bool(got), (m["name"], khex, seq)
            want = {"OK": gm.FOUND if got else gm.UNDECIDED, "NotFound: ": gm.DELETED}[status]
            assert verdict == want, (m["name"], khex, seq)
            assert (value or b"") == bytes.fromhex(vhex)
            seen.add(verdict)
    assert seen == {gm.UNDECIDED, gm.FOUND, gm.DELETED}


def test_model_reproduces_find_file(fx):
    fixture, _ = fx
    assert [len(c["files"]) for c in fixture["find_file"]] == [0, 1, 2, 3, 64, 65]
    hidden = level0_differs = 0
    for c in fixture["find_file"]:
        bounds = [(bytes.fromhex(s), bytes.fromhex(g)) for s, g, _ in c["files"]]
        visible = [v for _, _, v in c["files"]]
        for khex, index, covered, covered_visible, overlap in c["queries"]:
            ikey = bytes.fromhex(khex)
            assert gm.find_file([g for _, g in bounds], ikey) == index
            assert (gm.pick(bounds, 0, ikey) >= 0) == bool(covered)
            at = gm.pick(bounds, 0, ikey, visible)
            assert (at >= 0) == bool(covered_visible) and at in (-1, index)
            hidden += covered and not covered_visible
            for i, bit in enumerate(bytes.fromhex(overlap)):
                assert (gm.pick(bounds[i:i + 1], gm.RUN_LEVEL0, ikey) == 0) == bool(bit)
                level0_differs += bool(bit) and index != i
    assert hidden and level0_differs  # an invisible file at the found index; FindFile and the LEVEL0 rule differ


def test_model_reproduces_saver(fx):
    fixture, _ = fx
    states = set()
    for khex, vhex, uhex, state, saved in fixture["saver"]:
        verdict, value = gm.save_value(gm.VALID, bytes.fromhex(khex), bytes.fromhex(vhex), bytes.fromhex(uhex))
        assert verdict == state  # (kNotFound, kFound, kDeleted, kCorrupt are 0..3 in both)
        assert (value or b"") == bytes.fromhex(saved)
        states.add(state)
    assert states == {0, 1, 2, 3}


def test_model_reproduces_versions(fx, snappy_oracle):
    fixture, blob = fx
    uncompress = codec(snappy_oracle)
    for v in fixture["versions"]:
        mems, tables, bounds, runs, visible = open_version(v, blob, uncompress)
        number = [f["number"] for f in v["files"]]
        for (uhex, seq), want in zip(v["queries"], v["results"]):
            user = bytes.fromhex(uhex)
            verdict, value, where = gm.version_get(mems, tables, bounds, runs, user, seq, uncompress,
                                                   bool(v["verify"]), visible)
            what = (v["name"], user, seq)
            assert gm.status_string(verdict, user) == want["status"], what
            assert (value or b"").hex() == want["value"], what
            assert where == want["where"], what
            # every table read the reference made, and what its saver was handed
            ikey = gm.lookup_key(user, seq)
            probes = []
            for r, (files, flags) in enumerate(runs):
                at = gm.pick([bounds[f] for f in files], flags, ikey, [visible[f] for f in files])
                if at < 0:
                    continue
                state, found, val = gm.table_get(tables[files[at]], ikey, uncompress, bool(v["verify"]),
                                                 bool(flags & gm.RUN_PRECHECKED))
                probes.append((r, number[files[at]], state, found, val))
                if gm.save_value(state, found, val, user)[0] != gm.UNDECIDED:
                    break
            if where != -1 and where < len(mems):
                probes = []
            assert [(p["run"], p["number"]) for p in want["probes"]] == [(r, n) for r, n, _, _, _ in probes], what
            for p, (_, _, state, found, val) in zip(want["probes"], probes):
                assert bool(p["saver_called"]) == (state == gm.VALID), what
                if state == gm.VALID:
                    assert (found.hex(), val.hex()) == (p["ikey"], p["value"]), what
                ok = state in (gm.VALID, gm.NOT_VALID, gm.FILTERED)
                assert p["status"] == ("OK" if ok else "Corruption: " + gm.STATE_MESSAGE[state]), what


def test_fixture_versions_show_what_they_exist_for(fx):
    fixture, _ = fx
    by = {v["name"]: v for v in fixture["versions"]}

    def result(v, user, seq):
        return v["results"][v["queries"].index([user.hex(), seq])]

    hot = b"hot-key"
    # the flipped block stops the queries that reach it, though an older file holds the key
    assert result(by["tree"], hot, 2550)["status"] == "NotFound: "  # (the deletion in l0_mid)
    assert result(by["tree_flipped_block"], hot, 2550)["status"] == "Corruption: block checksum mismatch"
    assert result(by["tree_flipped_block"], hot, 9999) == result(by["tree"], hot, 9999)  # decided by the memtable
    assert result(by["tree"], hot, 1250)["value"] == b"hot-ancient".hex()
    assert result(by["tree"], b"both", 9999)["value"] == b"in-mem".hex()
    same = sum(a == b for a, b in zip(by["tree"]["results"], by["tree_flipped_block"]["results"]))
    assert 0 < same < len(by["tree"]["results"])
    plain = {r["status"] for r in by["bad_index_plain"]["results"]}
    assert "Corruption: bad entry in block" in plain
    assert "Corruption: bad entry in block" not in {r["status"] for r in by["bad_index_prechecked"]["results"]}


def test_memtable_lookup_equals_linear_scan():
    """The model's binary search against a scan of the sorted entries, on 300
    seeded random histories with duplicate user keys."""
    from golden import blockmodel as bm
    from golden import memtablemodel as mt
    rng = random.Random(0xD86E7)
    for _ in range(300):
        users = [bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 4))) for _ in range(rng.randint(1, 6))]
        n = rng.randint(0, 40)
        keys = [rng.choice(users) + struct.pack("<Q", (rng.randint(1, 12) << 8) | rng.choice((0, 1, 1)))
                for _ in range(n)]
        entries = [(keys[i], b"v%d" % i) for i in mt.order(keys)]
        for user in users + [b"", b"aab", b"c"]:
            for seq in (0, 3, 6, 12, 20):
                ikey = gm.lookup_key(user, seq)
                first = next((i for i, (k, _) in enumerate(entries) if bm.compare(k, ikey, bm.INTERNAL_KEY) >= 0),
                             len(entries))
                assert gm.memtable_seek(entries, ikey) == first
                want = (gm.UNDECIDED, None)
                if first < n and entries[first][0][:-8] == user:
                    want = (gm.FOUND, entries[first][1]) if entries[first][0][-8] == 1 else (gm.DELETED, None)
                assert gm.memtable_get(entries, user, seq) == want
