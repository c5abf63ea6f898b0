"""Memtable flush on the GPU (include/lsbm_memtable.h, lsbm_amd/memtable.py):
scan / decode / sort / entries / flush / recover_log, everything exact against
the reference's fixture (tests/golden/memtable_fixture.json) or the plain-Python
model (tests/golden/memtablemodel.py, pinned to that fixture by
tests/test_memtable.py).
"""
import ctypes
import random
import struct

import numpy as np
import pytest

from golden import memtable_cases as mc
from golden import memtablemodel as mt
from golden import snappytablemodel as stm

pytestmark = pytest.mark.gpu

GUARD = 0xEE
MAX_SEQ = (1 << 56) - 1


@pytest.fixture(scope="module")
def fixture():
    return mc.load()


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(1, dtype=getattr(torch, str(a.dtype)), device="cuda")[:0]
    return torch.from_numpy(a.copy()).to("cuda")


def _image(torch, b):
    return _dev(torch, np.frombuffer(bytes(b) + b"\0", dtype=np.uint8))[:len(b)]


def lay_out(payloads, gap=0):
    """The payloads back to back (gap bytes of 0xAA between them): (bytes, [(offset, length)])."""
    buf, recs = bytearray(), []
    for p in payloads:
        buf += b"\xaa" * gap
        recs.append((len(buf), len(p)))
        buf += p
    return bytes(buf), recs


def check_scan_decode(torch, buf, recs, label=""):
    """scan and decode of the records against the model's walk, with guard
    bytes around every output of decode."""
    from lsbm_amd import memtable
    image = _image(torch, buf)
    records = _dev(torch, np.array(recs, dtype=np.int64).reshape(-1))
    want = [mt.insert_into(buf, off, ln) for off, ln in recs]
    counts, status = memtable.scan(image, records)
    counts, status = counts.cpu().tolist(), status.cpu().tolist()
    assert status == [st for st, _ in want], label
    assert counts == [[len(es), sum(len(k) - 8 for k, _, _ in es)] for _, es in want], label
    entry_base, key_base = memtable.bases(_dev(torch, np.array(counts, dtype=np.int64).reshape(-1, 2)))
    flat = [e for _, es in want for e in es]
    ne, nk = len(flat), sum(len(k) for k, _, _ in flat)
    assert (int(entry_base[-1]), int(key_base[-1])) == (ne, nk), label
    g_keys = torch.full((nk + 128,), GUARD, dtype=torch.uint8, device="cuda")
    g_off = torch.full((ne + 1 + 16,), -2, dtype=torch.int64, device="cuda")
    g_val = torch.full((2 * ne + 32,), -2, dtype=torch.int64, device="cuda")
    d = memtable.decode(image, records, entry_base, key_base, keys=g_keys[64:64 + nk], key_offsets=g_off[8:8 + ne + 1],
                        values=g_val[16:16 + 2 * ne])
    assert d.status.cpu().tolist() == status, label
    kh, oh, vh = g_keys.cpu().numpy(), g_off.cpu().numpy(), g_val.cpu().numpy()
    assert np.all(kh[:64] == GUARD) and np.all(kh[64 + nk:] == GUARD), label
    assert np.all(oh[:8] == -2) and np.all(oh[8 + ne + 1:] == -2), label
    assert np.all(vh[:16] == -2) and np.all(vh[16 + 2 * ne:] == -2), label
    off = oh[8:8 + ne + 1]
    assert int(off[0]) == 0 and int(off[-1]) == nk, label
    got = [(kh[64 + int(off[j]):64 + int(off[j + 1])].tobytes(), int(vh[16 + 2 * j]), int(vh[16 + 2 * j + 1]))
           for j in range(ne)]
    assert got == [(k, vo, len(v)) for k, v, vo in flat], label
    assert memtable.max_sequence_of(d.max_sequence) == mt.max_sequence(buf, recs), label
    return flat


def test_scan_decode_fixture_and_random_payloads(torch_cuda, fixture):
    """Every fixture payload and 2,000 seeded payloads with random damage."""
    cases, bad = fixture
    payloads = [r for c in cases for r in mt.log_records(c["log"])] + [p for m in bad for p in m["payloads"]]
    rng = random.Random(0xBA7C4)
    payloads += [mc.random_payload(rng) for _ in range(2000)]
    buf, recs = lay_out(payloads, gap=3)
    check_scan_decode(torch_cuda, buf, recs)
    statuses = {mt.walk(buf, o, n)[0] for o, n in recs}
    assert statuses == {mt.OK, mt.TOO_SMALL, mt.BAD_PUT, mt.BAD_DELETE, mt.UNKNOWN_TAG, mt.WRONG_COUNT}
    # each malformed case alone is what the reference's memtable held
    for m in bad:
        buf, recs = lay_out(m["payloads"])
        flat = check_scan_decode(torch_cuda, buf, recs, m["name"])
        assert sorted(k for k, _, _ in flat) == sorted(k for k, _ in m["iteration"]), m["name"]


def test_scan_decode_record_counts_and_log_image(torch_cuda):
    from lsbm_amd import log
    torch = torch_cuda
    rng = random.Random(0x10C)
    good = [mc.batch(rng.randrange(1 << 40), [(rng.choice((0, 1)), bytes([65 + i % 26]) * rng.randrange(0, 12), b"v" * i)
                                              for i in range(rng.randrange(0, 4))]) for _ in range(257)]
    for n in (0, 1, 255, 256, 257):
        buf, recs = lay_out(good[:n])
        check_scan_decode(torch, buf or b"\0", recs, n)
    # records that point into a log image, at the payloads past the 7-byte headers
    image, heads = log.layout_records(good[:40])
    recs = [(int(h) + 7, len(p)) for h, p in zip(heads, good[:40])]
    check_scan_decode(torch, image.tobytes(), recs, "log image")
    # a pair one byte past the image; its neighbours are still walked
    buf, recs = lay_out(good[1:4])
    recs[1] = (recs[2][0], recs[2][1] + 1)
    check_scan_decode(torch, buf, recs, "past the image")
    assert [mt.walk(buf, o, n)[0] for o, n in recs] == [mt.OK, mt.BAD_INPUT, mt.OK]
    recs[1] = (len(buf) + 1, 0)
    check_scan_decode(torch, buf, recs, "offset past the image")
    recs[1] = (len(buf), 0)  # (an empty pair at the end is inside: too small)
    check_scan_decode(torch, buf, recs, "empty at the end")


# ---------------------------------------------------------------- sort

def ikey(user, seq, typ=1):
    return user + struct.pack("<Q", seq << 8 | typ)


class Keys:
    def __init__(self, torch, keys):
        kb = b"".join(keys)
        koff = np.zeros(len(keys) + 1, dtype=np.int64)
        koff[1:] = np.cumsum([len(k) for k in keys])
        self.keys = _image(torch, kb)
        self.koff = _dev(torch, koff)
        self.host = keys


def check_sort(torch, keys, label=""):
    from lsbm_amd import memtable
    K = Keys(torch, keys)
    p = memtable.sort(K.keys, K.koff)
    n = len(keys)
    source = p.source.cpu().tolist()
    want = mt.order(keys)
    assert p.run_status.cpu().tolist() == [0], label
    assert sorted(source) == list(range(n)), label  # a permutation
    assert source == want, label
    assert p.counts.cpu().tolist() == [n, sum(len(k) for k in keys)], label
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(keys[i]) for i in want])
    assert np.array_equal(p.out_key_offsets.cpu().numpy(), off), label
    return K, p


def key_sets(rng, n):
    """{name: n internal keys in arrival order}."""
    def user(lo=0, hi=12, alphabet=b"ab"):
        return bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))

    mixed = [ikey(user(), rng.randrange(1, 50), rng.choice((0, 1))) for _ in range(n)]
    in_order = [mixed[i] for i in mt.order(mixed)]
    out = {"mixed": mixed, "sorted": in_order, "reversed": in_order[::-1],
           "one_user": [ikey(b"user", s) for s in rng.sample(range(1, 4 * n + 2), n)],
           "all_equal": [ikey(b"equal", 7)] * n,
           "lengths_8_to_300": [ikey(bytes(rng.choice(b"xy") for _ in range(rng.choice((0, 1, 7, 8, 9, 100, 292)))),
                                     rng.randrange(1, 9)) for _ in range(n)]}
    for shared in (8, 16, 137):
        head = bytes(rng.randrange(256) for _ in range(shared))
        out["equal_through_%d" % shared] = [ikey(head + user(0, 3), rng.randrange(1, 9)) for _ in range(n)]
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768])
def test_sort_shapes(torch_cuda, n):
    rng = random.Random(0x50A7 + n)
    for name, keys in key_sets(rng, n).items():
        K, p = check_sort(torch_cuda, keys, (name, n))
        if name == "all_equal":
            assert p.source.cpu().tolist() == list(range(n))[::-1]  # arrival reversed


def test_sort_4097_and_boundaries(torch_cuda):
    rng = random.Random(0x4097)
    sets = key_sets(rng, 4097)
    for name in ("mixed", "reversed", "all_equal", "equal_through_137"):
        check_sort(torch_cuda, sets[name], (name, 4097))
    # a key and the key it is a prefix of, side by side across a tile boundary
    # (entries 255 | 256) and across a run boundary of the first pass (511 | 512)
    for at in (255, 511):
        for shorter_first in (True, False):
            keys = [ikey(bytes(rng.choice(b"pq") for _ in range(rng.randint(0, 20))), rng.randrange(1, 9))
                    for _ in range(1030)]
            pair = [ikey(b"pqpqpqpqpq", 5), ikey(b"pqpqpqpqpq\x00", 5)]
            keys[at], keys[at + 1] = pair if shorter_first else pair[::-1]
            check_sort(torch_cuda, keys, ("prefix pair", at, shorter_first))


def test_sort_65537(torch_cuda):
    """Nine merge passes."""
    rng = random.Random(0x10001)
    users = [bytes(rng.choice(b"abcdefgh") for _ in range(rng.choice((3, 8, 9, 17)))) for _ in range(20000)]
    keys = [ikey(rng.choice(users), rng.randrange(1, 4), rng.choice((0, 1))) for _ in range(65537)]
    check_sort(torch_cuda, keys, 65537)


def test_sort_errors(torch_cuda):
    from lsbm_amd import _lib, memtable
    from lsbm_amd.engine import _ptr, _stream_ptr
    torch = torch_cuda
    rng = random.Random(0xE44)
    keys = [ikey(bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 6))), i + 1) for i in range(700)]
    K = Keys(torch, keys)
    # a 7-byte key
    koff = K.koff.clone()
    koff[300:] -= int(koff[300] - koff[299]) - 7
    p = memtable.sort(K.keys, koff.contiguous())
    assert p.run_status.cpu().tolist() == [2] and p.counts.cpu().tolist() == [0, 0]
    # an offset that decreases, one past keys_size
    for at, v in ((5, 0), (699, K.keys.numel() + 1)):
        koff = K.koff.clone()
        koff[at] = v
        p = memtable.sort(K.keys, koff)
        assert p.run_status.cpu().tolist() == [2] and p.counts.cpu().tolist() == [0, 0], at
    # scratch one byte short
    L = _lib.lib()
    n = len(keys)
    need = L.lsbm_memtable_sort_scratch_bytes(n)
    scratch = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    source = torch.zeros(n, dtype=torch.int64, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(nbytes, src=source):
        return L.lsbm_memtable_sort_dev(_ptr(K.keys), K.keys.numel(), _ptr(K.koff), n, _ptr(src), _ptr(out_off),
                                        _ptr(counts), _ptr(status), _ptr(scratch), nbytes, _stream_ptr(None))
    assert call(need - 1) == _lib.LSBM_ERR_INVALID
    assert call(need, K.koff) == _lib.LSBM_ERR_INVALID  # an output that aliases an input
    assert call(need) == _lib.LSBM_OK
    assert source.cpu().tolist() == mt.order(keys)
    assert need == 24 * n + 8 * ((n + 255) // 256) + 8 + (8 if n % 2 else 0)
    assert L.lsbm_memtable_sort_dev(None, 0, _ptr(K.koff), (1 << 31) + 1, _ptr(source), _ptr(out_off), _ptr(counts),
                                    _ptr(status), _ptr(scratch), ctypes.c_uint64(1 << 62), _stream_ptr(None)) \
        == _lib.LSBM_ERR_INVALID


# ---------------------------------------------------------------- end to end

def read_entries(e, image_host):
    keys, off, vals = e.keys.cpu().numpy(), e.key_offsets.cpu().numpy(), e.values.cpu().numpy().reshape(-1, 2)
    return [(keys[int(off[j]):int(off[j + 1])].tobytes(),
             image_host[int(vals[j, 0]):int(vals[j, 0]) + int(vals[j, 1])]) for j in range(len(off) - 1)]


def test_entries_flush_recover_fixture(torch_cuda, fixture):
    """entries, flush and recover_log over every fixture log == the reference's
    iteration and table file, byte for byte."""
    from lsbm_amd import memtable
    cases, bad = fixture
    for c in cases:
        image, records = memtable.log_records(c["log"])
        host = image.cpu().numpy().tobytes()
        lens = records.cpu().numpy().reshape(-1, 2)[:, 1].tolist()
        assert lens == c["record_lens"], c["name"]
        assert [host[o:o + n] for o, n in records.cpu().numpy().reshape(-1, 2).tolist()] == mt.log_records(c["log"])
        e = memtable.entries(image, records, paranoid=True)
        assert read_entries(e, host) == c["iteration"], c["name"]
        assert e.status.cpu().tolist() == [0] * len(lens)
        recs = records.cpu().numpy().reshape(-1, 2).tolist()
        assert e.max_sequence == mt.max_sequence(host, recs), c["name"]
        f = memtable.recover_log(c["log"], block_size=c["block_size"], restart_interval=c["restart_interval"],
                                 bits_per_key=c["bits_per_key"])
        if c["table"] is None:
            assert f.image is None and f.smallest is None and f.largest is None, c["name"]
        else:
            assert f.image.cpu().numpy().tobytes() == c["table"], c["name"]
            assert (f.smallest, f.largest) == (c["iteration"][0][0], c["iteration"][-1][0]), c["name"]
        assert f.max_sequence == e.max_sequence
    for m in bad:
        buf, recs = lay_out(m["payloads"])
        image = _image(torch_cuda, buf or b"\0")[:len(buf)]
        records = _dev(torch_cuda, np.array(recs, dtype=np.int64).reshape(-1))
        e = memtable.entries(image, records)
        assert read_entries(e, buf) == m["iteration"], m["name"]
        words = dict(mt.MESSAGE)
        words[mt.TOO_SMALL] = "Corruption: log record too small"
        assert [words[s] for s in e.status.cpu().tolist()] == m["statuses"], m["name"]
        first_bad = [s for s in m["statuses"] if s != "OK"]
        if first_bad:
            with pytest.raises(ValueError, match=first_bad[0].split(": ", 1)[1].replace("(", r"\(")):
                memtable.entries(image, records, paranoid=True)


def test_log_records_faults(torch_cuda, fixture):
    from lsbm_amd import memtable
    cases, _ = fixture
    log = bytearray([c for c in cases if c["name"] == "one_batch"][0]["log"])
    for damage in ("crc", "type", "length", "cut"):
        b = bytearray(log)
        if damage == "crc":
            b[20] ^= 1
        elif damage == "type":
            b[6] = 9
        elif damage == "length":
            b[5] = 0x7F
        else:
            b = b[:-1]
        with pytest.raises(ValueError, match="lsbm::log::BatchReader"):
            memtable.log_records(bytes(b))


def test_flush_snappy_get_and_compact(torch_cuda, fixture, snappy_oracle):
    """flush with snappy == the model; the flushed table read back by
    sstable.table_get; two flushed tables through sstable.compact == the model."""
    from lsbm_amd import block, memtable, sstable
    from lsbm_amd.table import kSnappyCompression
    torch = torch_cuda
    cases, _ = fixture
    by = {c["name"]: c for c in cases}
    comp = lambda raw: snappy_oracle.compress(raw)  # noqa: E731
    for name in ("batch_1000", "hot_key_300", "fragments"):
        c = by[name]
        f = memtable.recover_log(c["log"], compression=kSnappyCompression, block_size=c["block_size"],
                                 restart_interval=c["restart_interval"], bits_per_key=c["bits_per_key"])
        want = mt.table_file(c["iteration"], c["block_size"], c["restart_interval"], c["bits_per_key"], comp)
        assert f.image.cpu().numpy().tobytes() == want, name
    # Get over the flushed deletions table: present, deleted and absent user keys
    c = by["deletions"]
    f = memtable.recover_log(c["log"], block_size=c["block_size"], restart_interval=c["restart_interval"],
                             bits_per_key=10)
    ents = c["iteration"]
    users = sorted({k[:-8] for k, _ in ents})
    queries = users + [u + b"\x00" for u in users[:3]] + [b"", b"\xff\xff", b"never"]
    lookups = [ikey(u, MAX_SEQ, 1) for u in queries]
    Q = Keys(torch, lookups)
    g = sstable.table_get(f.image, f.index_handle, Q.keys, Q.koff)
    state, key_len, value = g.state.cpu().tolist(), g.key_len.cpu().tolist(), g.value.cpu().tolist()
    vimg = g.value_image.cpu().numpy().tobytes()
    seen = set()
    for q, look in enumerate(lookups):
        hit = next(((k, v) for k, v in ents if mt.compare(k, look) >= 0), None)
        if hit is None:
            assert state[q] == block.SEEK_NOT_VALID, queries[q]
            seen.add("absent")
            continue
        assert state[q] == block.SEEK_VALID and key_len[q] == len(hit[0]), queries[q]
        assert vimg[value[q][0]:value[q][0] + value[q][1]] == hit[1], queries[q]
        seen.add("absent" if hit[0][:-8] != queries[q] else ("deleted" if hit[0][-8] == 0 else "present"))
    assert seen == {"present", "deleted", "absent"}
    # the tables of two logs, the newer first, compacted
    a, b = by["deletions"], by["one_batch"]
    fa = memtable.recover_log(a["log"], block_size=256, restart_interval=4)
    fb = memtable.recover_log(b["log"], block_size=256, restart_interval=4)
    out = sstable.compact([fb.image, fa.image], index_handles=[fb.index_handle, fa.index_handle],
                          max_file_size=500, block_size=256, restart_interval=4, bits_per_key=10)
    want = stm.compact([b["iteration"], a["iteration"]], 1, 500, block_size=256, restart_interval=4,
                       bits_per_key=10)
    assert len(out) == len(want) > 1
    assert [t.image.cpu().numpy().tobytes() for t in out] == want


def _blob(b):
    b = bytes(b)
    return struct.pack("<Q", len(b)) + b


def test_cpp_build_level0(torch_cuda, fixture, tmp_path):
    """include/lsbm/memtable_flush.h (BuildLevel0) through tests/cpp/memtable_tool.cc
    == the fixture; an injected device error returns non-OK and leaves `file`
    as it was."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    exe = tmp_path / "memtable_tool"
    libdir = os.path.join(repo, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(repo, "include"),
                    os.path.join(here, "cpp", "memtable_tool.cc"), "-L", libdir, "-llsbm_crc32c",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)

    def run(records, block_size=4096, restart_interval=16, bits_per_key=None, paranoid=0, inject=0):
        params = np.array([block_size, restart_interval, 0 if bits_per_key is None else bits_per_key + 1, paranoid,
                           inject], dtype=np.uint64).tobytes()
        fi, fo = tmp_path / "cmd.bin", tmp_path / "out.bin"
        fi.write_bytes(_blob(params) + b"".join(_blob(r) for r in records))
        p = subprocess.run([str(exe), str(fi), str(fo)], check=True, capture_output=True, text=True, timeout=120)
        out = fo.read_bytes()
        max_seq, n = struct.unpack_from("<QQ", out, 0)
        st = list(struct.unpack_from("<%dQ" % n, out, 16))
        at, blobs = 16 + 8 * n, []
        for _ in range(3):
            ln = struct.unpack_from("<Q", out, at)[0]
            blobs.append(out[at + 8:at + 8 + ln])
            at += 8 + ln
        return p.stdout.strip(), max_seq, st, blobs

    cases, bad = fixture
    for c in cases:
        records = mt.log_records(c["log"])
        status, max_seq, st, (file, lo, hi) = run(records, c["block_size"], c["restart_interval"], c["bits_per_key"])
        assert status == "status OK" and st == [0] * len(records), c["name"]
        buf, recs = lay_out(records)
        assert max_seq == mt.max_sequence(buf, recs), c["name"]
        if c["table"] is None:
            assert (file, lo, hi) == (b"", b"", b""), c["name"]
        else:
            assert file == c["table"], c["name"]
            assert (lo, hi) == (c["iteration"][0][0], c["iteration"][-1][0]), c["name"]
    # errors are ignored without paranoid_checks, and named with them
    m = [m for m in bad if m["name"] == "bad_between_good"][0]
    status, _, st, (file, lo, hi) = run(m["payloads"], 256, 4)
    assert status == "status OK" and st == [mt.OK, mt.UNKNOWN_TAG, mt.OK]
    assert file == mt.table_file(m["iteration"], 256, 4)
    status, _, st, (file, lo, hi) = run(m["payloads"], 256, 4, paranoid=1)
    assert status == "status Corruption: unknown WriteBatch tag (record 1)" and file == b"untouched"
    # a device error: non-OK, and the outputs are as they were
    c = [c for c in cases if c["name"] == "one_batch"][0]
    status, _, st, (file, lo, hi) = run(mt.log_records(c["log"]), 256, 4, 10, inject=1)
    assert status == "status IO error: injected fault"
    assert (file, lo, hi) == (b"untouched", b"untouched", b"untouched")
