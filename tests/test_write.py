"""Batched DB::Write, CPU side (include/lsbm_write.h, lsbm_amd/write.py).

The plain-Python model (tests/golden/writemodel.py, a transcript of
WriteBatch::Put / Delete, BuildBatchGroup, Append / SetSequence and
log::Writer::AddRecord) against the reference's own results
(tests/golden/write_fixture.json + .bin, written by make_write_fixture.py, whose
driver runs DBImpl::BuildBatchGroup itself on writers queued on an unopened
DBImpl): every group's leader and rep, the sequence numbers, the log files with
their CRCs through the oracle; the model's AddRecord at every record boundary
as log_offset, and against log.layout_records; the C ABI's symbols.  The GPU
side is tests/test_write_gpu.py.
"""
import os
import random
import re
import struct
import subprocess

import pytest

from golden import write_cases as wc
from golden import writemodel as wm

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def fixture():
    return wc.load()


def masked_crc(oracle):
    return lambda data: oracle.mask(oracle.value(data))


def test_model_reproduces_write_fixture(fixture, oracle):
    writes, _ = fixture
    for c in writes:
        writers = wc.writers_of(c["writers"])
        reps, group_first, group_sync, seqs, counts, last = wm.write(writers, c["last_sequence"])
        assert group_first == c["group_first"], c["name"]
        assert reps == c["reps"], c["name"]
        assert last == c["new_last_sequence"] == c["last_sequence"] + sum(len(ops) for ops, _ in writers), c["name"]
        assert seqs[0] == c["last_sequence"] + 1 and all(b == a + n for a, b, n in zip(seqs, seqs[1:], counts))
        assert group_sync == [writers[f][1] for f in group_first[:-1]]
        log, heads, frags, end = wm.add_records(reps, 0, masked_crc(oracle))
        assert log == c["log"] and end == len(log), c["name"]


def test_model_reproduces_log_fixture_from_every_boundary(fixture, oracle):
    _, logs = fixture
    for c in logs:
        payloads = [wc.pattern(seed, n) for n, seed in c["payloads"]]
        log, heads, frags, end = wm.add_records(payloads, 0, masked_crc(oracle))
        assert log == c["log"] and end == len(log), c["name"]
        assert sum(frags) == len(heads)
        # a Writer that starts at any record boundary appends the rest of the file
        at = 0
        for i in range(len(payloads) + 1):
            tail, theads, _, tend = wm.add_records(payloads[i:], at, masked_crc(oracle))
            assert tail == c["log"][at:] and tend == len(c["log"]), (c["name"], i)
            if i < len(payloads):
                at = wm.add_records(payloads[:i + 1], 0)[3]


def test_fixture_covers_the_cases(fixture):
    writes, logs = fixture
    by = {c["name"]: c for c in writes}
    B, P = wc.B, wc.P
    klens = {op[1] for _, ops in by["encoding"]["writers"] for op in ops}
    vlens = {op[3] for _, ops in by["encoding"]["writers"] for op in ops if op[0]}
    assert set(wc.LENGTHS) <= klens and set(wc.LENGTHS) <= vlens
    assert any(not ops for _, ops in by["encoding"]["writers"])
    assert any(op[0] == 0 for _, ops in by["encoding"]["writers"] for op in ops)
    assert [len(ops) for _, ops in by["ops_65_257"]["writers"]] == [65, 257, 1]
    assert by["one_writer"]["group_first"] == [0, 1]
    size = lambda c, w: wm.batch_of(wc.ops_of(by[c]["writers"][w][1])).byte_size()  # noqa: E731
    assert size("leader_131072_exact", 0) == 131072 and by["leader_131072_exact"]["group_first"] == [0, 2, 4]
    assert size("leader_131072_one_above", 1) == 131073 and by["leader_131072_one_above"]["group_first"] == [0, 1, 3]
    assert size("leader_131073_exact", 0) + size("leader_131073_exact", 1) == 1 << 20
    assert by["leader_131073_exact"]["group_first"] == [0, 2, 4]
    assert by["leader_131073_one_above"]["group_first"] == [0, 1, 3]
    assert size("leader_above_1mib", 0) > 1 << 20 and by["leader_above_1mib"]["group_first"] == [0, 1, 4]
    # bodies alone (ByteSize - 12 per follower) would let 100 followers join; the reference takes 99
    hc = by["header_counting"]
    sizes = [size("header_counting", w) for w in range(len(hc["writers"]))]
    assert sizes[0] + sum(s - 12 for s in sizes[1:101]) <= sizes[0] + 131072 < sum(sizes[:101])
    assert hc["group_first"][:2] == [0, 100]
    sm = by["sync_mixed"]
    syncs = [s for s, _ in sm["writers"]]
    assert sm["group_first"][:3] == [0, 2, 10] and syncs[:3] == [0, 0, 1]  # stops before the sync writer; it takes the rest
    assert by["sync_all"]["group_first"] == [0, 6]
    assert by["sync_leader_takes_both"]["group_first"] == [0, 5]
    assert len(by["writers_1025"]["writers"]) == 1025
    lb = {c["name"]: c for c in logs}
    named = {0, 1, 6, 7, 8, P - 8, P - 7, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 5 * P + 3}
    assert named <= {n for n, _ in lb["lengths"]["payloads"]}
    # every trailer width 1..6 and a zero-length FIRST are in the "ends" file
    log, pos, pads, empty_first = lb["ends"]["log"], 0, set(), False
    while pos < len(log):
        left = B - pos % B
        if left < 7:
            assert log[pos:pos + left] == bytes(left)
            pads.add(left)
            pos += left
            continue
        n, t = log[pos + 4] | log[pos + 5] << 8, log[pos + 6]
        empty_first |= t == 2 and n == 0
        pos += 7 + n
    assert pads == {1, 2, 3, 4, 5, 6} and empty_first
    assert [n for n, _ in lb["ten_P"]["payloads"]] == [P] * 10 and len(lb["short_130"]["payloads"]) == 130
    for name, at in (("offset_P", P), ("offset_B-6", B - 6), ("offset_B-1", B - 1), ("offset_B", B),
                     ("offset_B+7", B + 7), ("offset_mid", 1007)):
        lens = [n for n, _ in lb[name]["payloads"]]
        k = 2 if name == "offset_B+7" else 1
        assert wm.add_records([bytes(n) for n in lens[:k]])[3] == at, name


def test_group_rule_model_is_the_running_sum_rule():
    """BuildBatchGroup's loop == "the largest end whose running ByteSize sum
    stays within max_size, capped by the next sync writer": the form the
    kernel uses, on random queues."""
    rng = random.Random(0x6209)
    for trial in range(300):
        n = rng.randrange(1, 40)
        sizes = [rng.choice((12, 16, 500, 40000, 131072, 131073, 300000, 1 << 20, (1 << 20) + 1)) for _ in range(n)]
        syncs = [rng.random() < 0.3 for _ in range(n)]
        sums = [0]
        for s in sizes:
            sums.append(sums[-1] + s)
        first, cuts = 0, [0]
        while first < n:
            mx = sizes[first] + 131072 if sizes[first] <= 131072 else 1 << 20
            e = first + 1
            while e < n and sums[e + 1] - sums[first] <= mx:
                e += 1
            if not syncs[first]:
                nxt = next((w for w in range(first + 1, n) if syncs[w]), n)
                e = min(e, nxt)
            cuts.append(e)
            first = e
        assert cuts == wm.groups(sizes, syncs), trial


def test_model_add_record_is_layout_records():
    from lsbm_amd.log import layout_records
    rng = random.Random(0xADD)
    P = wc.P
    for trial in range(40):
        lens = [rng.choice((0, 1, 6, 7, 8, 30, 1270, P - 8, P - 7, P - 1, P, P + 1, 2 * P, 2 * P + 1, 5 * P + 3))
                for _ in range(rng.randrange(0, 12))]
        payloads = [wc.pattern(i, n) for i, n in enumerate(lens)]
        image, heads = layout_records(payloads)
        log, mheads, frags, end = wm.add_records(payloads)
        assert log == image.tobytes() and mheads == heads.tolist() and end == len(log), trial


def test_reps_feed_the_memtable_model(fixture):
    writes, _ = fixture
    c = [c for c in writes if c["name"] == "ops_65_257"][0]
    got = wm.memtable_iteration(c["reps"])
    ops = [op for o, _ in wc.writers_of(c["writers"]) for op in o]
    assert len(got) == len(ops)
    want = {(k + struct.pack("<Q", (c["last_sequence"] + 1 + i) << 8 | t), v) for i, (t, k, v) in enumerate(ops)}
    assert set(got) == want


def test_header_declares_what_the_library_exports(product_lib):
    text = open(os.path.join(REPO, "include", "lsbm_write.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(lsbm_\w+)\s*\(", text)))
    from lsbm_amd import _lib
    assert names == sorted(_lib.WRITE_SIGNATURES) and len(names) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", product_lib._name], capture_output=True, text=True,
                         check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert not [n for n in names if n not in exported]
    import lsbm_amd
    assert "write" in lsbm_amd.__all__
    from lsbm_amd import write
    assert (write.OK, write.NO_ROOM, write.BAD_INPUT) == (0, 1, 2)
    assert (write.kBlockSize, write.kHeaderSize) == (wm.kBlockSize, wm.kHeaderSize)
