"""Readers for the range-scan fixture (tests/golden/scan_fixture.json and
scan_tables.bin, written by make_scan_fixture.py) and the seeded random
histories the model and the GPU scan are compared on."""
import json
import os
import random
import struct
import zlib

from golden import scanmodel as sm

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def fixture():
    """(the JSON, the inflated bytes of scan_tables.bin)."""
    if "fx" not in _cache:
        fx = json.load(open(os.path.join(HERE, "scan_fixture.json")))
        blob = zlib.decompress(open(os.path.join(HERE, "scan_tables.bin"), "rb").read())
        assert len(blob) == fx["inflated_bytes"]
        _cache["fx"] = (fx, blob)
    return _cache["fx"]


def iteration(blob, at):
    """[(key, value)] of an iteration record at {offset, size}."""
    p = at[0]
    (n,) = struct.unpack_from("<I", blob, p)
    p += 4
    out = []
    for _ in range(n):
        pair = []
        for _ in range(2):
            (ln,) = struct.unpack_from("<I", blob, p)
            pair.append(bytes(blob[p + 4:p + 4 + ln]))
            p += 4 + ln
        out.append(tuple(pair))
    assert p == at[0] + at[1]
    return out


def cases():
    """[(name, children [[(key, value)]], merged [(key, value)], queries)], a
    query being (snapshot, lo, hi, limit, reverse, [(user key, value)], status text)."""
    if "cases" not in _cache:
        fx, blob = fixture()
        out = []
        for c in fx["cases"]:
            raw = json.loads(bytes(blob[c["queries_at"][0]:c["queries_at"][0] + c["queries_at"][1]]))
            queries = [(s, None if lo is None else bytes.fromhex(lo), None if hi is None else bytes.fromhex(hi), limit,
                        bool(rev), [(bytes.fromhex(k), bytes.fromhex(v)) for k, v in got], status)
                       for s, lo, hi, limit, rev, got, status in raw]
            out.append((c["name"], [iteration(blob, ch["at"]) for ch in c["children"]],
                        iteration(blob, c["merged"]["at"]), queries))
        _cache["cases"] = out
    return _cache["cases"]


def random_history(seed, max_entries=40, error_keys=True):
    """(sorted [(internal key, value)], the user keys and a few strangers) of a
    seeded history: few user keys, many versions, deletions and error keys."""
    rng = random.Random(seed)
    users = sorted({bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 3))) for _ in range(rng.randint(1, 8))})
    entries = []
    for i in range(rng.randint(0, max_entries)):
        kind = rng.choice([0, 1, 1])
        if error_keys and rng.random() < 0.15:
            kind = rng.choice([2, 255])
        entries.append((sm.ikey(rng.choice(users), rng.randint(1, 30), kind), b"v%d" % i * rng.randint(0, 3)))
    return sm.sort_entries(entries), users + [b"", b"zz", b"b\x00"]


def random_queries(seed, users, count):
    """[(lo, hi, limit)] with absent bounds among them."""
    rng = random.Random(seed ^ 0x5CA9)
    return [(rng.choice(users + [None]), rng.choice(users + [None]), rng.choice([0, 1, 2, 3, 1000]))
            for _ in range(count)]
