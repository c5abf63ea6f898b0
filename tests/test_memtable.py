"""Memtable flush, CPU side (include/lsbm_memtable.h, lsbm_amd/memtable.py).

The plain-Python model (tests/golden/memtablemodel.py) against the reference's
own results (tests/golden/memtable_fixture.json, memtable_tables.bin, written
by make_memtable_fixture.py): the log's records, the memtable's iteration, the
table bytes, and for every malformed payload the status and the entries that
survive; the model's order against an insertion-by-insertion emulation of the
skiplist rule; the C ABI's symbols.  The GPU side is tests/test_memtable_gpu.py.
"""
import os
import random
import re
import struct
import subprocess

import pytest

from golden import memtable_cases as mc
from golden import memtablemodel as mt

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def fixture():
    return mc.load()


def records_of(log):
    """[(offset, length)] over the records laid back to back, and that buffer."""
    recs, buf = [], b""
    for r in mt.log_records(log):
        recs.append((len(buf), len(r)))
        buf += r
    return buf, recs


def test_model_reproduces_fixture(fixture):
    cases, _ = fixture
    for c in cases:
        buf, recs = records_of(c["log"])
        assert [n for _, n in recs] == c["record_lens"], c["name"]
        got, statuses, _ = mt.entries(buf, recs)
        assert statuses == [mt.OK] * len(recs), c["name"]
        assert got == c["iteration"], c["name"]
        table = mt.table_file(got, c["block_size"], c["restart_interval"], c["bits_per_key"])
        assert table == c["table"], c["name"]


def test_model_reproduces_malformed(fixture):
    _, bad = fixture
    words = dict(mt.MESSAGE)
    words[mt.TOO_SMALL] = "Corruption: log record too small"
    for m in bad:
        buf, recs = b"", []
        for p in m["payloads"]:
            recs.append((len(buf), len(p)))
            buf += p
        got, statuses, _ = mt.entries(buf, recs)
        assert [words[s] for s in statuses] == m["statuses"], m["name"]
        assert got == m["iteration"], m["name"]


def test_fixture_covers_the_cases(fixture):
    cases, bad = fixture
    by = {c["name"]: c for c in cases}
    assert by["no_batches"]["record_lens"] == [] and by["no_batches"]["table"] is None
    assert by["empty_batch"]["record_lens"] == [12] and by["empty_batch"]["table"] is None
    assert len(by["one_entry"]["iteration"]) == 1 and len(by["one_entry"]["record_lens"]) == 1
    assert len(by["batch_1000"]["iteration"]) == 1000 and len(by["batch_1000"]["record_lens"]) == 1
    # the fragmented log: FIRST / MIDDLE / LAST, an empty FIRST after 7 spare bytes, a 3-byte trailer
    log = by["fragments"]["log"]
    types, pos = [], 0
    while pos < len(log):
        left = 32768 - pos % 32768
        if left < 7:
            assert log[pos:pos + left] == bytes(left)
            types.append("trailer%d" % left)
            pos += left
            continue
        n, t = log[pos + 4] | log[pos + 5] << 8, log[pos + 6]
        types.append((t, n) if (t == 2 and n == 0) else t)
        pos += 7 + n
    assert types == [1, 2, 3, 4, 1, (2, 0), 4, 1, "trailer3", 1]
    vlens = {len(v) for _, v in by["fragments"]["iteration"]}
    assert {0, 200, 20000} <= vlens
    assert any(k[-8] == 0 for k, _ in by["deletions"]["iteration"])
    assert any(k[:-8] == b"never-written" and k[-8] == 0 for k, _ in by["deletions"]["iteration"])
    hot = [k for k, _ in by["hot_key_300"]["iteration"] if k[:-8] == b"hot"]
    tags = [struct.unpack("<Q", k[-8:])[0] for k in hot]
    assert len(hot) == 300 and tags == sorted(tags, reverse=True) and len(by["hot_key_300"]["record_lens"]) == 60
    us = [k[:-8] for k, _ in by["prefix_and_empty"]["iteration"]]
    assert us[0] == b"" and any(a != b and b.startswith(a) for a, b in zip(us, us[1:]))
    assert any(v == b"" and k[-8] == 1 for k, v in by["prefix_and_empty"]["iteration"])
    us = sorted({k[:-8] for k, _ in by["long_keys_one_byte"]["iteration"]})
    assert all(len(u) == 137 for u in us)
    diff = {tuple(i for i in range(137) if a[i] != b[i]) for a in us for b in us if a != b}
    assert (136,) in diff
    for k in (1, 8, 16):
        assert {(8 * k - 1,), (8 * k,), (8 * k + 1,)} <= diff
    same = [(k, v) for k, v in by["equal_internal_keys"]["iteration"] if k[:-8] == b"same"]
    assert [v for _, v in same] == [b"third", b"second", b"first", b""]  # equal keys: the later first; then the Delete
    assert same[0][0] == same[1][0] == same[2][0]
    us = [k[:-8] for k, _ in by["descending_arrival"]["iteration"]]
    seqs = [struct.unpack("<Q", k[-8:])[0] >> 8 for k, _ in by["descending_arrival"]["iteration"]]
    assert us == sorted(us) and seqs == sorted(seqs, reverse=True) and len(us) == 40
    assert any(c["bits_per_key"] for c in cases) and any(not c["bits_per_key"] for c in cases)
    names = {m["name"] for m in bad}
    assert {"length_0", "length_11", "length_12_count_0", "put_key_varint_cut", "key_one_past_end",
            "value_one_past_end", "tag_2", "count_one_high", "count_one_low", "varint_fifth_byte_high_bits",
            "varint_five_continuation_bytes", "bad_between_good"} <= names
    seen = {s for m in bad for s in m["statuses"]}
    assert seen == {"OK", "Corruption: log record too small", "Corruption: bad WriteBatch Put",
                    "Corruption: bad WriteBatch Delete", "Corruption: unknown WriteBatch tag",
                    "Corruption: WriteBatch has wrong count"}
    m = [m for m in bad if m["name"] == "varint_fifth_byte_high_bits"][0]
    assert m["statuses"] == ["OK"] and any(k[:-8] == b"key" for k, _ in m["iteration"])
    m = [m for m in bad if m["name"] == "value_one_past_end"][0]
    assert len(m["iteration"]) == 1  # the Put whose value fails is not in the memtable
    m = [m for m in bad if m["name"] == "bad_between_good"][0]
    assert m["statuses"][0] == "OK" and m["statuses"][1] != "OK" and m["statuses"][2] == "OK"
    assert {k[:-8] for k, _ in m["iteration"]} == {b"good", b"gone", b"half", b"tail"}


def test_order_is_the_skiplist_rule():
    """sorted by (user key, -tag, -arrival) == SkipList::Insert one key at a
    time, on 300 random histories with duplicates."""
    rng = random.Random(0x5C1B)
    with_duplicates = 0
    for trial in range(300):
        users = [bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 4))) for _ in range(rng.randint(1, 5))]
        keys = [rng.choice(users) + struct.pack("<Q", rng.randrange(1, 6) << 8 | rng.choice((0, 1, 1)))
                for _ in range(rng.randint(0, 40))]
        assert mt.order(keys) == mt.skiplist_order(keys), trial
        with_duplicates += len(set(keys)) < len(keys)
    assert with_duplicates > 150


def test_max_sequence_model():
    b = mc.batch(100, [(1, b"a", b"b")] * 3)
    assert mt.max_sequence(b, [(0, len(b))]) == 102
    assert mt.max_sequence(b, [(0, 11)]) == 0
    z = mc.batch(0, [])
    assert mt.max_sequence(z, [(0, len(z))]) == (1 << 64) - 1  # Sequence 0 + Count 0 - 1 wraps, as it does there
    neg = mc.batch(50, [], count=0xFFFFFFFF)  # Count is an int: -1
    assert mt.max_sequence(neg, [(0, len(neg))]) == 48


def test_header_declares_what_the_library_exports(product_lib):
    text = open(os.path.join(REPO, "include", "lsbm_memtable.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(lsbm_\w+)\s*\(", text)))
    from lsbm_amd import _lib
    assert names == sorted(_lib.MEMTABLE_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", product_lib._name], capture_output=True, text=True,
                         check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert not [n for n in names if n not in exported]
    import lsbm_amd
    assert "memtable" in lsbm_amd.__all__
    from lsbm_amd import memtable
    assert (memtable.WB_OK, memtable.WB_TOO_SMALL, memtable.WB_BAD_PUT, memtable.WB_BAD_DELETE,
            memtable.WB_UNKNOWN_TAG, memtable.WB_WRONG_COUNT, memtable.WB_BAD_INPUT) == \
        (mt.OK, mt.TOO_SMALL, mt.BAD_PUT, mt.BAD_DELETE, mt.UNKNOWN_TAG, mt.WRONG_COUNT, mt.BAD_INPUT)
    for name, code in re.findall(r"#define (LSBM_WB_\w+) (\d+)u", open(os.path.join(REPO, "include",
                                                                                   "lsbm_memtable.h")).read()):
        assert getattr(memtable, name[5:]) == int(code)
