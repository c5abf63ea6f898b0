"""Compaction merge (include/lsbm_merge.h, lsbm_amd/merge.py).

CPU: the plain-Python model (tests/golden/mergemodel.py) against the
reference's own MergingIterator results (tests/golden/merge_fixture.json,
merge_tables.bin, written by make_merge_fixture.py); the pairwise drop rule
against the sequential loop of lsbm/db_impl.cc:999-1032 and against the
snapshot-visibility property; the table cut against an entry-by-entry
emulation; the C ABI's symbols and argument checks.
GPU: plan / gather / merge / compact, byte-exact against the fixture or the
model.
"""
import json
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

from golden import blockmodel as bm
from golden import buildmodel as bd
from golden import mergemodel as mm

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
GUARD = 0xEE
MAX_SEQ = mm.MAX_SEQ


def table_entries(f):
    """[(key, value)] of a table file, read back through the block model."""
    f = bytes(f)
    footer = f[-48:]
    assert struct.unpack_from("<Q", footer, 40)[0] == bd.MAGIC
    a = bm.get_varint64(footer, 0, 40)
    b = bm.get_varint64(footer, a[1], 40)
    c = bm.get_varint64(footer, b[1], 40)
    d = bm.get_varint64(footer, c[1], 40)
    index = f[c[0]:c[0] + d[0]]
    st, ients = bm.walk(index)
    assert st == bm.OK
    out = []
    for _, vo, vl, _ in ients:
        o, s = bm.decode_handle(index[vo:vo + vl])
        blk = f[o:o + s]
        st, ents = bm.walk(blk)
        assert st == bm.OK
        out += [(k, blk[eo:eo + el]) for k, eo, el, _ in ents]
    return out


@pytest.fixture(scope="module")
def cases():
    """[(record, [[(key, value)]] runs, [(key, value)] merged by the reference)]."""
    fx = json.load(open(os.path.join(G, "merge_fixture.json")))
    blob = open(os.path.join(G, "merge_tables.bin"), "rb").read()
    out = []
    for r in fx["cases"]:
        runs = [table_entries(blob[o:o + n]) for o, n in r["tables"]]
        p, merged = r["merged"][0], []
        for _ in range(r["n_merged"]):
            kv = []
            for _ in range(2):
                n = struct.unpack_from("<I", blob, p)[0]
                kv.append(blob[p + 4:p + 4 + n])
                p += 4 + n
            merged.append(tuple(kv))
        assert p == sum(r["merged"])
        out.append((r, runs, merged))
    return out


def by_name(cases, name, cmp):
    return [c for c in cases if c[0]["name"] == name and c[0]["cmp"] == cmp][0]


# ---------------------------------------------------------------- CPU: the model
def test_model_reproduces_fixture(cases):
    for r, runs, merged in cases:
        got, source = mm.merge_entries(runs, r["cmp"])
        assert got == merged, (r["name"], r["cmp"])
        # a value names its entry: the reference took the entries the model says
        flat = [e for run in runs for e in run]
        assert [flat[s] for s in source] == merged
        for run in runs:
            assert mm.run_status([k for k, _ in run], r["cmp"]) == mm.OK, r["name"]
            assert [v for _, v in run] == [bytes([v[0], i & 0xff, i >> 8]) for i, (_, v) in enumerate(run)]


def test_fixture_covers_the_cases(cases):
    names = {r["name"] for r, _, _ in cases}
    assert all(sum(r["name"] == n for r, _, _ in cases) == 2 for n in names)  # both comparators
    assert {len(runs) for _, runs, _ in cases} >= {0, 1, 2, 3, 8, 64}
    for cmp in (0, 1):
        lens = [len(run) for run in by_name(cases, "empty_first_middle_last", cmp)[1]]
        assert lens[0] == 0 and lens[-1] == 0 and 0 in lens[1:-1] and any(lens)
        r, runs, merged = by_name(cases, "all_empty", cmp)
        assert runs and not any(runs) and not merged
        r, runs, merged = by_name(cases, "identical_runs", cmp)
        assert len(runs) >= 3 and all([k for k, _ in run] == [k for k, _ in runs[0]] for run in runs)
        n = len(runs)  # ties across every run come out in run order
        assert [v[0] for _, v in merged[:n]] == list(range(n))
        r, runs, merged = by_name(cases, "equal_neighbours", cmp)
        assert any(a[0] == b[0] for run in runs for a, b in zip(run, run[1:]))
        for name, order in (("disjoint_ascending", [0, 1, 2]), ("disjoint_descending", [2, 1, 0])):
            r, runs, merged = by_name(cases, name, cmp)
            seen = [v[0] for _, v in merged]
            assert [x for i, x in enumerate(seen) if i == 0 or seen[i - 1] != x] == order
        r, runs, merged = by_name(cases, "interleave", cmp)
        assert [v[0] for _, v in merged] == [i % 4 for i in range(len(merged))]
        strip = (lambda k: k[:-8]) if cmp else (lambda k: k)
        r, runs, merged = by_name(cases, "prefix_of_next", cmp)
        us = [strip(k) for k, _ in merged]
        assert any(a != b and b.startswith(a) for a, b in zip(us, us[1:]))
        r, runs, merged = by_name(cases, "empty_user_key", cmp)
        assert strip(merged[0][0]) == b""
        r, runs, merged = by_name(cases, "long_keys_one_byte", cmp)
        us = sorted({strip(k) for k, _ in merged})
        assert all(len(u) > 127 for u in us)
        diff = {tuple(i for i in range(len(a)) if a[i] != b[i]) for a in us for b in us if a != b}
        assert (len(us[0]) - 1,) in diff
        for k in (1, 8, 16):
            assert {(8 * k - 1,), (8 * k,), (8 * k + 1,)} <= diff
    r, runs, merged = by_name(cases, "versions_across_runs", 1)
    users = {}
    for ri, run in enumerate(runs):
        for k, _ in run:
            users.setdefault(k[:-8], set()).add(ri)
    assert sum(len(s) >= 3 for s in users.values()) >= 3
    keys = [k for k, _ in merged]
    assert any(a == b for a, b in zip(keys, keys[1:]))  # the same internal key in two runs


def random_history(rng, n_users=6, max_versions=6, seq_hi=40, error_keys=True):
    """Internal keys in merged order: versions of a few user keys, distinct
    sequence numbers per user key, now and then an error key (type 2)."""
    keys = []
    for u in sorted({bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 3))) for _ in range(n_users)}):
        seqs = sorted(rng.sample(range(seq_hi), rng.randint(1, max_versions)), reverse=True)
        for s in seqs:
            typ = 2 if error_keys and rng.random() < 0.08 else rng.choice((0, 1, 1))
            keys.append(mm.internal_key(u, s, typ))
    return keys


def test_pairwise_drop_equals_sequential_drop():
    rng = random.Random(0xD209)
    for trial in range(600):
        keys = random_history(rng)
        for snap in (0, MAX_SEQ, rng.randrange(40), rng.randrange(40)):
            for bottom in (False, True):
                assert mm.drop_pairwise(keys, snap, bottom) == mm.drop_sequential(keys, snap, bottom), \
                    (trial, snap, bottom)
    # an error key resets the rule and is kept
    keys = [mm.internal_key(b"k", 9), mm.internal_key(b"k", 7, 2), mm.internal_key(b"k", 5)]
    assert mm.drop_sequential(keys, 20, False) == [False, False, False]
    assert mm.drop_pairwise(keys, 20, False) == [False, False, False]
    # evaluated as written: with the largest snapshot every parseable entry is hidden
    assert mm.drop_sequential(keys[:1], MAX_SEQ, False) == [True]


def test_snapshot_visibility_property():
    """For every snapshot s >= smallest_snapshot the value visible at s is the
    same before and after merge + drop; at the bottom level a deleted key reads
    as absent either way."""
    rng = random.Random(0x51A9)
    for trial in range(300):
        keys = random_history(rng, error_keys=False)
        entries = [(k, b"v%d" % i) for i, k in enumerate(keys)]
        # spread over runs (each stays sorted), merge back, drop
        runs = [[] for _ in range(rng.randint(1, 5))]
        for e in entries:
            runs[rng.randrange(len(runs))].append(e)
        smallest = rng.randrange(41)
        for bottom in (False, True):
            kept, _ = mm.merge_entries(runs, mm.INTERNAL_KEY, True, smallest, bottom)
            assert [e for e in entries if e in kept] == kept
            for user in {k[:-8] for k in keys}:
                for s in range(smallest, 42):
                    assert mm.visible(kept, user, s) == mm.visible(entries, user, s), (trial, user, s, bottom)


def test_cut_equals_entry_by_entry_emulation():
    rng = random.Random(0xC07)
    for trial in range(120):
        n = rng.randint(0, 120)
        ks = sorted({bytes(rng.choice(b"abcd") for _ in range(rng.randint(1, 20))) for _ in range(n)})
        entries = [(k, rng.randint(0, 60)) for k in ks]
        bs, ri = rng.choice((64, 256, 1024)), rng.choice((1, 3, 16))
        target = rng.choice((1, 5, 100, 300, 1000, 3000, rng.randint(1, 3000)))
        first, sizes = bd.plan(entries, bs, ri)
        table_first, table_block_first = mm.cut_tables(first, sizes, target)
        want_first, want_tables = mm.cut_emulation(entries, bs, ri, target)
        assert table_first == (want_first if entries else [0]), (trial, bs, ri, target)
        # the per-table re-plan tiles to the same blocks
        for t, (bf, bsz) in enumerate(want_tables):
            b0, b1 = table_block_first[t], table_block_first[t + 1]
            assert bf == first[b0:b1 + 1] and bsz == sizes[b0:b1]
            f2, s2 = bd.plan(entries[table_first[t]:table_first[t + 1]], bs, ri)
            assert [table_first[t] + x for x in f2] == bf and s2 == bsz
        from lsbm_amd import merge
        assert merge.cut_tables(first, sizes, target) == (table_first, table_block_first)
    assert mm.cut_tables([0], [], 100) == ([0], [0])


# ---------------------------------------------------------------- CPU: the C ABI
NAMES = ["lsbm_merge_gather_dev", "lsbm_merge_plan_dev", "lsbm_merge_scratch_bytes"]


def test_merge_symbols_exported_and_declared(product_lib):
    from lsbm_amd import _lib
    text = open(os.path.join(REPO, "include", "lsbm_merge.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(lsbm_\w+)\s*\(", text))) == NAMES
    assert sorted(_lib.MERGE_SIGNATURES) == NAMES
    out = subprocess.run(["nm", "-D", "--defined-only", product_lib._name], capture_output=True,
                         text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert not [n for n in NAMES if n not in exported]
    assert any("MergeRuns" in n for n in exported) and any("CutTables" in n for n in exported)
    build_h = open(os.path.join(REPO, "include", "lsbm_block_build.h")).read()
    for name, v in (("OK", 0), ("NO_ROOM", 1), ("BAD_INPUT", 2), ("UNSORTED", 3)):
        assert re.search(r"#define LSBM_MERGE_%s %du\b" % (name, v), build_h)
    import lsbm_amd
    from lsbm_amd import merge
    assert "merge" in lsbm_amd.__all__
    for fn in ("plan", "gather", "merge", "cut_tables", "compact"):
        assert callable(getattr(merge, fn))
    assert (merge.MERGE_OK, merge.MERGE_NO_ROOM, merge.MERGE_BAD_INPUT, merge.MERGE_UNSORTED) == (0, 1, 2, 3)
    assert merge.MAX_RUNS == 64


def _calls(L):
    """The two entry points on fake host pointers (a buffer of its own for
    every role, so that nothing aliases), one argument replaced at a time."""
    keep = [np.zeros(256, dtype=np.uint64) for _ in range(12)] + [np.zeros(64, dtype=np.uint8) for _ in range(2)]
    p = [x.ctypes.data for x in keep]
    kp, op = p[12], p[13]

    def plan(**kw):
        return L.lsbm_merge_plan_dev(kw.get("keys", kp), 8, kw.get("koff", p[0]), 1, kw.get("runs", p[1]),
                                     kw.get("n_runs", 1), kw.get("cmp", 1), kw.get("flags", 0), 0,
                                     kw.get("source", p[2]), kw.get("ooff", p[3]), kw.get("counts", p[4]),
                                     kw.get("status", p[5]), kw.get("scratch", p[6]),
                                     kw.get("scratch_bytes", 2048), None)

    def gather(**kw):
        return L.lsbm_merge_gather_dev(kp, 8, kw.get("koff", p[0]), kw.get("values", p[7]), 1,
                                       kw.get("source", p[2]), kw.get("poff", p[3]), kw.get("counts", p[4]),
                                       kw.get("out_keys", op), 8, kw.get("ooff", p[8]), kw.get("ovals", p[9]), 1,
                                       kw.get("status", p[10]), None)
    return keep, plan, gather


def test_merge_entry_points_check_arguments(product_lib):
    """A bad argument is LSBM_ERR_INVALID, with or without a device; a good
    call gets past the checks (to the device, or to LSBM_ERR_NO_DEVICE)."""
    import torch
    from lsbm_amd import _lib
    L = _lib.lib()
    keep, plan, gather = _calls(L)
    inv = _lib.LSBM_ERR_INVALID
    assert plan(keys=None) == inv
    assert plan(koff=None) == inv
    assert plan(runs=None) == inv
    assert plan(source=None) == inv
    assert plan(ooff=None) == inv
    assert plan(counts=None) == inv
    assert plan(status=None) == inv
    assert plan(scratch=None) == inv
    assert plan(scratch_bytes=8) == inv                                    # short scratch
    assert plan(scratch_bytes=L.lsbm_merge_scratch_bytes(1, 1) - 1) == inv
    assert plan(n_runs=65) == inv                                          # LSBM_MERGE_MAX_RUNS is 64
    assert plan(cmp=2) == inv
    assert plan(cmp=0, flags=1) == inv                                     # DROP under BYTEWISE
    assert plan(cmp=0, flags=3) == inv
    assert plan(flags=4) == inv
    assert gather(koff=None) == inv
    assert gather(values=None) == inv
    assert gather(source=None) == inv
    assert gather(poff=None) == inv
    assert gather(counts=None) == inv
    assert gather(out_keys=None) == inv
    assert gather(ooff=None) == inv
    assert gather(ovals=None) == inv
    assert gather(status=None) == inv
    # outputs that alias inputs
    assert plan(source=keep[0].ctypes.data) == inv
    assert plan(status=keep[1].ctypes.data) == inv
    assert plan(scratch=keep[12].ctypes.data & ~7) == inv
    assert gather(out_keys=keep[12].ctypes.data) == inv
    assert gather(ooff=keep[3].ctypes.data) == inv
    assert gather(ovals=keep[7].ctypes.data) == inv
    assert gather(status=keep[4].ctypes.data) == inv
    if not torch.cuda.is_available():  # (host pointers: only where no kernel can run on them)
        nd = _lib.LSBM_ERR_NO_DEVICE
        assert plan() == nd and gather() == nd
    n = 1000
    assert L.lsbm_merge_scratch_bytes(n, 4) >= 8 * n + 4 * n


def test_merge_entry_points_fail_loudly_without_device(product_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    from lsbm_amd import _lib
    L = _lib.lib()
    keep, plan, gather = _calls(L)
    assert plan() == _lib.LSBM_ERR_NO_DEVICE
    assert gather() == _lib.LSBM_ERR_NO_DEVICE
    from lsbm_amd import merge
    t = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError):
        merge.plan(torch.zeros(8, dtype=torch.uint8), t, t)  # host tensors are refused, never merged on the CPU


# ---------------------------------------------------------------- GPU helpers
def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: frombuffer views are read-only)


class Runs:
    """[[(key, value)]] as the device tensors lsbm_block_decode_dev would write
    for the runs laid back to back; the values sit in an image of their own."""

    def __init__(self, torch, runs):
        self.runs = runs
        flat = [e for run in runs for e in run]
        self.flat = flat
        koff = np.zeros(len(flat) + 1, dtype=np.int64)
        koff[1:] = np.cumsum([len(k) for k, _ in flat])
        kb = np.frombuffer(b"".join(k for k, _ in flat) + b"\0", np.uint8).copy()
        img, values = bytearray(b"\x5a"), []
        for _, v in flat:
            values.append([len(img), len(v)])
            img += v
        rf = np.zeros(len(runs) + 1, dtype=np.int64)
        rf[1:] = np.cumsum([len(r) for r in runs])
        self.koff_host, self.rf_host = koff, rf
        self.values_host = np.array(values, dtype=np.int64).reshape(-1, 2)
        self.image_host = bytes(img)
        self.keys, self.koff = _dev(torch, kb)[:len(kb) - 1], _dev(torch, koff)
        self.values, self.image = _dev(torch, self.values_host), _dev(torch, np.frombuffer(bytes(img), np.uint8))
        self.run_first = _dev(torch, rf)
        self.n = len(flat)


def gpu_merge(R, cmp, **kw):
    """merge.merge read back: ([(key, value)], source, run_status)."""
    from lsbm_amd import merge
    m = merge.merge(R.keys, R.koff, R.values, R.run_first, cmp, **kw)
    keys, koff, vals = m.keys.cpu().numpy(), m.key_offsets.cpu().numpy(), m.values.cpu().numpy()
    got = [(keys[int(koff[j]):int(koff[j + 1])].tobytes(),
            R.image_host[int(vals[j, 0]):int(vals[j, 0]) + int(vals[j, 1])]) for j in range(len(koff) - 1)]
    assert int(koff[0]) == 0 and int(koff[-1]) == keys.size
    return got, m.source.cpu().tolist(), m.run_status.cpu().tolist()


def check_merge(torch, runs, cmp, label="", **kw):
    R = Runs(torch, runs)
    got, source, status = gpu_merge(R, cmp, **kw)
    want, want_source = mm.merge_entries(runs, cmp, kw.get("drop", False), kw.get("smallest_snapshot", 0),
                                         kw.get("bottom_level", False))
    assert status == [0] * len(runs), label
    assert source == want_source, label
    assert got == want, label
    return got


def keyed(users_or_keys, run, cmp, rng=None):
    """A sorted run of (key, value) over user keys; the value names run and position."""
    ks = sorted(users_or_keys)
    if cmp:
        ks = [mm.internal_key(u, (rng.randrange(1, 1 << 30) if rng else 5), 1) for u in ks]
    return [(k, struct.pack("<HI", run, i)) for i, k in enumerate(ks)]


def user_pool(rng, n, lo=2, hi=14):
    ks = set()
    while len(ks) < n:
        ks.add(bytes(rng.choice(b"abc") for _ in range(rng.randint(lo, hi))))
    return sorted(ks)


# ---------------------------------------------------------------- GPU tests
@pytest.mark.gpu
def test_gpu_fixture_merge(torch_cuda, cases):
    """1. every fixture case under its comparator == the reference's MergingIterator."""
    torch = torch_cuda
    for r, runs, merged in cases:
        R = Runs(torch, runs)
        got, source, status = gpu_merge(R, r["cmp"])
        assert status == [0] * len(runs), r["name"]
        assert got == merged, (r["name"], r["cmp"])
        assert [R.flat[s] for s in source] == merged, r["name"]


@pytest.mark.gpu
def test_gpu_run_shapes(torch_cuda):
    """2. run lengths around a lane, a wave (which is also rank's sample
    interval, 64) and a workgroup (the scan tile is one workgroup's 256
    positions), 64 runs of one entry, 4,097 against 1."""
    torch = torch_cuda
    rng = random.Random(0x5A9E)
    pool = user_pool(rng, 700)
    for cmp in (0, 1):
        lens = (0, 1, 63, 64, 65, 255, 256, 257)
        runs = [keyed(rng.sample(pool, n), r, cmp, rng) for r, n in enumerate(lens)]
        check_merge(torch, runs, cmp, ("lens", cmp))
        for n in (255, 256, 257):  # a single run: the output is the input
            check_merge(torch, [keyed(rng.sample(pool, n), 0, cmp, rng)], cmp, ("single", n))
        runs = [keyed([rng.choice(pool[:20])], r, cmp) for r in range(64)]  # many ties: run order decides
        check_merge(torch, runs, cmp, ("64x1", cmp))
        big = [struct.pack(">I", i) for i in range(4097)]
        for one in (b"", struct.pack(">I", 2048), struct.pack(">I", 2048) + b"\0", b"\xff" * 5):
            check_merge(torch, [keyed(big, 0, cmp), keyed([one], 1, cmp)], cmp, ("4097+1", one))
            check_merge(torch, [keyed([one], 0, cmp), keyed(big, 1, cmp)], cmp, ("1+4097", one))
    check_merge(torch, [], 0, "no runs")
    check_merge(torch, [[], []], 1, "empty runs")


@pytest.mark.gpu
def test_gpu_drop_rule(torch_cuda):
    """3. the drop rule, against the model's pairwise form (itself pinned to the
    sequential loop on the CPU)."""
    torch = torch_cuda
    ik = mm.internal_key
    rng = random.Random(0xD20)

    def val(runs):
        return [[(k, struct.pack("<HI", r, i)) for i, k in enumerate(run)] for r, run in enumerate(runs)]

    # versions of one user key that straddle a run boundary and merged positions
    # 63 / 64 and 255 / 256: fillers put the key's newest version at 63 and at 255
    for at in (63, 255):
        fill = [ik(b"a" + struct.pack(">H", i), 9) for i in range(at)]
        runs = val([fill + [ik(b"k", 30), ik(b"k", 10, 0)], [ik(b"k", 20), ik(b"k", 5)], [ik(b"z", 1)]])
        for snap in (0, 4, 5, 10, 15, 20, 25, 30, MAX_SEQ):
            for bottom in (False, True):
                got = check_merge(torch, runs, 1, (at, snap, bottom), drop=True, smallest_snapshot=snap,
                                  bottom_level=bottom)
                if snap == 15 and not bottom:
                    assert [k for k, _ in got[at:]] == [ik(b"k", 30), ik(b"k", 20), ik(b"k", 10, 0), ik(b"z", 1)]
    # five versions, the snapshot between the 2nd and the 3rd: the 3rd is the
    # newest one the snapshot sees and stays, the 4th and 5th go
    five = val([[ik(b"u", 50), ik(b"u", 30), ik(b"u", 10)], [ik(b"u", 40), ik(b"u", 20)]])
    got = check_merge(torch, five, 1, "five", drop=True, smallest_snapshot=35)
    assert [k for k, _ in got] == [ik(b"u", 50), ik(b"u", 40), ik(b"u", 30)]
    # a deletion with and without BOTTOM_LEVEL
    dele = val([[ik(b"d", 9, 0), ik(b"e", 3)], [ik(b"d", 4)]])
    got = check_merge(torch, dele, 1, "del", drop=True, smallest_snapshot=100)
    assert [k for k, _ in got] == [ik(b"d", 9, 0), ik(b"e", 3)]
    got = check_merge(torch, dele, 1, "del bottom", drop=True, smallest_snapshot=100, bottom_level=True)
    assert [k for k, _ in got] == [ik(b"e", 3)]
    got = check_merge(torch, dele, 1, "del newer than the snapshot", drop=True, smallest_snapshot=8,
                      bottom_level=True)
    assert [k for k, _ in got] == [ik(b"d", 9, 0), ik(b"d", 4), ik(b"e", 3)]
    # a type-2 key between two versions of one user key resets the rule and is kept
    err = val([[ik(b"k", 9), ik(b"k", 5)], [ik(b"k", 7, 2)]])
    got = check_merge(torch, err, 1, "type 2", drop=True, smallest_snapshot=100)
    assert [k for k, _ in got] == [ik(b"k", 9), ik(b"k", 7, 2), ik(b"k", 5)]
    # snapshot 0 keeps every version of distinct sequence; kMaxSequenceNumber, as written, hides everything
    hist = [k for k in random_history(rng, 12, 6, 40) if k[-8] <= 1 and mm.tag_of(k) >> 8]
    runs = [[] for _ in range(4)]
    for k in hist:
        runs[rng.randrange(4)].append(k)
    got = check_merge(torch, val(runs), 1, "snapshot 0", drop=True, smallest_snapshot=0, bottom_level=True)
    assert len(got) == len(hist)
    R = Runs(torch, val(runs))
    got, source, status = gpu_merge(R, 1, drop=True, smallest_snapshot=MAX_SEQ)
    assert got == [] and source == [] and status == [0] * 4  # everything dropped: n_out = 0
    # random histories over 1..5 runs
    for trial in range(12):
        keys = random_history(rng, 40, 6, 60)
        runs = [[] for _ in range(rng.randint(1, 5))]
        for k in keys:
            runs[rng.randrange(len(runs))].append(k)
        check_merge(torch, val(runs), 1, ("random", trial), drop=True, smallest_snapshot=rng.randrange(60),
                    bottom_level=bool(trial & 1))
    from lsbm_amd import merge
    with pytest.raises(ValueError):
        merge.merge(R.keys, R.koff, R.values, R.run_first, 0, drop=True, smallest_snapshot=1)


@pytest.mark.gpu
def test_gpu_error_status_and_no_room(torch_cuda):
    """4. an unsorted run and a 7-byte internal key give their status and
    n_out = 0; caps one byte / one entry short give NO_ROOM and an untouched
    guard region."""
    torch = torch_cuda
    from lsbm_amd import merge
    rng = random.Random(0xE44)
    pool = user_pool(rng, 300)
    for cmp in (0, 1):
        runs = [keyed(rng.sample(pool, n), r, cmp, rng) for r, n in enumerate((70, 300, 5))]
        runs[1][200], runs[1][201] = runs[1][201], runs[1][200]
        R = Runs(torch, runs)
        p = merge.plan(R.keys, R.koff, R.run_first, cmp)
        assert p.run_status.cpu().tolist() == [0, merge.MERGE_UNSORTED, 0]
        assert p.counts.cpu().tolist() == [0, 0]
        got, source, status = gpu_merge(R, cmp)
        assert got == [] and status == [0, 3, 0]
    runs = [keyed(rng.sample(pool, n), r, 1, rng) for r, n in enumerate((70, 30))]
    runs[0][69] = (b"7 bytes", b"")
    runs[1][3], runs[1][4] = runs[1][4], runs[1][3]
    R = Runs(torch, runs)
    p = merge.plan(R.keys, R.koff, R.run_first, 1)
    assert p.run_status.cpu().tolist() == [merge.MERGE_BAD_INPUT, merge.MERGE_UNSORTED]
    assert p.counts.cpu().tolist() == [0, 0]
    assert merge.plan(R.keys, R.koff, R.run_first, 0).run_status.cpu().tolist()[1] == merge.MERGE_UNSORTED
    # key offsets that decrease or pass keys_size; run_first that decreases or passes n
    runs = [keyed(rng.sample(pool, n), r, 0) for r, n in enumerate((40, 40))]
    R = Runs(torch, runs)
    koff = R.koff_host.copy()
    koff[79] = koff[78] - 1  # (entry 78 alone: entry 79 is the run's last and still a key)
    p = merge.plan(R.keys, _dev(torch, koff), R.run_first, 0)
    assert p.run_status.cpu().tolist() == [0, 2] and p.counts.cpu().tolist() == [0, 0]
    koff = R.koff_host.copy()
    koff[80] += 1
    p = merge.plan(R.keys, _dev(torch, koff), R.run_first, 0)
    assert p.run_status.cpu().tolist() == [0, 2] and p.counts.cpu().tolist() == [0, 0]
    for rf in ([0, 50, 40], [0, 40, 81], [1, 40, 80], [0, 40, 79]):
        p = merge.plan(R.keys, R.koff, _dev(torch, np.array(rf, dtype=np.int64)), 0)
        assert max(p.run_status.cpu().tolist()) == 2 and p.counts.cpu().tolist() == [0, 0], rf
    # gather: exact caps fit; one byte or one entry short is NO_ROOM with nothing written
    p = merge.plan(R.keys, R.koff, R.run_first, 0)
    n_out, nbytes = p.counts.cpu().tolist()
    assert n_out == 80 and nbytes == R.keys.numel()
    want, _ = mm.merge_entries(runs, 0)
    for short_keys, short_entries in ((0, 0), (1, 0), (0, 1)):
        ok = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
        oo = torch.full((n_out + 1 + 8,), -2, dtype=torch.int64, device="cuda")
        ov = torch.full((n_out + 8, 2), -2, dtype=torch.int64, device="cuda")
        cap = n_out - short_entries
        g = merge.gather(R.keys, R.koff, R.values, p, ok[:nbytes - short_keys], oo[:cap + 1], ov[:cap])
        st = int(g.status.cpu()[0])
        okh, ooh, ovh = ok.cpu().numpy(), oo.cpu().numpy(), ov.cpu().numpy()
        if short_keys or short_entries:
            assert st == merge.MERGE_NO_ROOM
            assert np.all(okh == GUARD) and np.all(ooh == -2) and np.all(ovh == -2)
        else:
            assert st == merge.MERGE_OK
            assert okh[:nbytes].tobytes() == b"".join(k for k, _ in want)
            assert np.all(okh[nbytes:] == GUARD) and np.all(ooh[n_out + 1:] == -2) and np.all(ovh[n_out:] == -2)
            assert list(ooh[:n_out + 1]) == list(np.cumsum([0] + [len(k) for k, _ in want]))
    # a plan that is not of these entries moves nothing of the wave it touches
    bad = merge.PlanResult(p.source.clone(), p.out_key_offsets.clone(), p.counts, p.run_status)
    bad.source[5] = 80
    g = merge.gather(R.keys, R.koff, R.values, bad)
    assert int(g.status.cpu()[0]) == merge.MERGE_BAD_INPUT


@pytest.mark.gpu
def test_gpu_compact_end_to_end(torch_cuda):
    """5. four overlapping input tables -> 3+ output tables, byte-identical to
    buildmodel.table_file over the model's merged, thinned and cut entries;
    table_get(verify=True) finds every kept key."""
    torch = torch_cuda
    from lsbm_amd import block, merge
    rng = random.Random(0xC0AC)
    pool = user_pool(rng, 500, 6, 16)
    runs = []
    for r in range(4):
        ents = []
        for u in sorted(rng.sample(pool, 300)):
            seqs = sorted(rng.sample(range(1, 1000), 2 if rng.random() < 0.1 else 1), reverse=True)
            for s in seqs:
                typ = 0 if rng.random() < 0.1 else 1
                ents.append((mm.internal_key(u, s, typ), bytes(rng.randrange(256) for _ in range(rng.randint(0, 40)))))
        runs.append(ents)
    files = [bd.table_file(run, mm.INTERNAL_KEY, 1024, 16, 10) for run in runs]
    images = [_dev(torch, np.frombuffer(f[0], np.uint8)) for f in files]
    handles = [np.array(f[1], dtype=np.int64).reshape(-1) for f in files]
    for kw in (dict(drop=True, smallest_snapshot=600, bottom_level=True), dict()):
        want = mm.compact(runs, mm.INTERNAL_KEY, 12000, block_size=1024, restart_interval=16, bits_per_key=10,
                          **kw)
        assert len(want) >= 3
        out = merge.compact(images, handles, 12000, block_size=1024, bits_per_key=10, **kw)
        assert [o.image.cpu().numpy().tobytes() for o in out] == want
    # from the index handles alone; and every kept key is found in its output table
    out = merge.compact(images, None, 12000, index_handles=[f[2] for f in files], block_size=1024, bits_per_key=10,
                        drop=True, smallest_snapshot=600, bottom_level=True)
    want = mm.compact(runs, mm.INTERNAL_KEY, 12000, True, 600, True, 1024, 16, 10)
    assert [o.image.cpu().numpy().tobytes() for o in out] == want
    kept, _ = mm.merge_entries(runs, mm.INTERNAL_KEY, True, 600, True)
    found = 0
    for o, f in zip(out, want):
        ents = table_entries(f)
        E = Runs(torch, [ents])
        res = block.table_get(o.image, o.index_handle, E.keys, E.koff, verify=True, cmp=block.INTERNAL_KEY)
        assert not res.state.cpu().numpy().any()
        img, val = o.image.cpu().numpy(), res.value.cpu().numpy()
        first = {}  # (the same internal key from two inputs: Seek stops at the first, the earlier input's)
        for k, v in ents:
            first.setdefault(k, v)
        assert res.key_len.cpu().tolist() == [len(k) for k, _ in ents]
        assert [img[int(a):int(a) + int(n)].tobytes() for a, n in val] == [first[k] for k, _ in ents]
        found += len(ents)
    assert found == len(kept)


def _blob(b):
    b = bytes(b)
    return struct.pack("<Q", len(b)) + b


@pytest.mark.gpu
def test_cpp_compaction_layer(torch_cuda, cases, tmp_path):
    """6. include/lsbm/compaction.h (MergeRuns, CutTables) against the fixture
    and the model, driven by tests/cpp/merge_tool.cc."""
    exe = tmp_path / "merge_tool"
    libdir = os.path.join(REPO, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"),
                    os.path.join(HERE, "cpp", "merge_tool.cc"), "-L", libdir, "-llsbm_crc32c",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    u64 = lambda a: np.array(a, dtype=np.uint64).tobytes()  # noqa: E731

    def run(runs, cmp, drop=0, snap=0, bottom=0, swap=None):
        flat = [e for r in runs for e in r]
        if swap:
            flat[swap[0]], flat[swap[1]] = flat[swap[1]], flat[swap[0]]
        keys = b"".join(k for k, _ in flat)
        koff = np.concatenate([[0], np.cumsum([len(k) for k, _ in flat])]).astype(np.uint64)
        voff = np.concatenate([[0], np.cumsum([len(v) for _, v in flat])]).astype(np.uint64)
        values = np.stack([voff[:-1], np.diff(voff)], axis=1).astype(np.uint64)
        rf = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.uint64)
        cmd = (_blob(u64([cmp, drop, snap, bottom])) + _blob(keys) + _blob(koff.tobytes())
               + _blob(values.tobytes()) + _blob(rf.tobytes()))
        fi, fo = tmp_path / "cmd.bin", tmp_path / "out.bin"
        fi.write_bytes(cmd)
        p = subprocess.run([str(exe), "merge", str(fi), str(fo)], check=True, capture_output=True, text=True,
                           timeout=120)
        out = fo.read_bytes()
        n, nr = struct.unpack_from("<QQ", out, 0)
        w = np.frombuffer(out, dtype=np.uint64, count=2 + nr + n + (n + 1) + 2 * n)
        st, src = list(w[2:2 + nr]), list(w[2 + nr:2 + nr + n])
        ko = w[2 + nr + n:2 + nr + 2 * n + 1]
        vals = w[2 + nr + 2 * n + 1:].reshape(-1, 2)
        kb = out[8 * w.size:]
        image = b"".join(v for _, v in flat)
        got = [(kb[int(ko[j]):int(ko[j + 1])], image[int(vals[j, 0]):int(vals[j, 0] + vals[j, 1])]) for j in range(n)]
        return p.stdout.strip(), got, [int(s) for s in src], [int(s) for s in st]

    for name, cmp in (("eight_runs", 0), ("versions_across_runs", 1), ("sixty_four_runs", 1), ("no_runs", 0)):
        r, runs, merged = by_name(cases, name, cmp)
        status, got, src, st = run(runs, cmp)
        assert status == "status OK" and got == merged and st == [0] * len(runs), name
    r, runs, merged = by_name(cases, "versions_across_runs", 1)
    want, want_src = mm.merge_entries(runs, 1, True, 20, True)
    status, got, src, st = run(runs, 1, 1, 20, 1)
    assert status == "status OK" and got == want and src == want_src and len(want) < len(merged)
    r, runs, merged = by_name(cases, "two_runs", 0)
    status, got, src, st = run(runs, 0, swap=(len(runs[0]) + 2, len(runs[0]) + 3))
    assert status == "status Invalid argument: run is not sorted (run 1)" and got == [] and st == [0, 3]
    # CutTables == the model's cut
    rng = random.Random(0xC7)
    for trial in range(6):
        ks = sorted({bytes(rng.choice(b"abcd") for _ in range(rng.randint(1, 20))) for _ in range(150)})
        first, sizes = bd.plan([(k, rng.randint(0, 60)) for k in ks], 256, 16)
        target = rng.choice((1, 300, 1000, 3000, 10 ** 9))
        fi, fo = tmp_path / "cut.bin", tmp_path / "cut_out.bin"
        fi.write_bytes(_blob(u64([target])) + _blob(u64(first)) + _blob(u64(sizes)))
        p = subprocess.run([str(exe), "cut", str(fi), str(fo)], check=True, capture_output=True, text=True,
                           timeout=120)
        assert p.stdout.strip() == "status OK"
        w = [int(x) for x in np.frombuffer(fo.read_bytes(), dtype=np.uint64)]
        nt = w[0]
        assert (w[1:nt + 2], w[nt + 2:]) == mm.cut_tables(first, sizes, target), (trial, target)
