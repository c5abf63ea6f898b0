"""The scenarios of the MANIFEST fixture (tests/golden/manifest_fixture.*).
The fixture maker feeds them to the reference and the tests rebuild the same
bytes, so only the reference's results are stored.

  records()    (name, bytes): one record each for VersionEdit::DecodeFrom.  None
               holds input on which the reference's behaviour is undefined
               (a type or a read-cursor index of 4 or more): those are
               undefined_records(), for the model and the device only.
  edits()      (name, edit): edit descriptions for AddFile / DeleteFile / Set*
               and EncodeTo, in the model's dict form.
  manifests()  (name, [record bytes], damage): whole MANIFEST files for
               BasicVersionSet::Recover, types 0 and 1 only (the buffer lists
               are evicted by a runtime parameter).  damage: None, ("cut", n)
               drops the file's last n bytes, ("flip", at) inverts one byte.
"""
import random
import struct

from . import manifestmodel as mm
from .manifestmodel import put_slice, put_varint as v

CMP = mm.BYTEWISE


def ikey(user, seq=1, t=1):
    return bytes(user) + ((seq << 8) | t).to_bytes(8, "little")


def bench_key(i, seq=1):
    """db_bench's 16-byte user key, as a 24-byte internal key."""
    return ikey(b"%016d" % i, seq)


def new_file(t, level, number, size, smallest, largest):
    return v(7) + v(t) + v(level) + v(number) + v(size) + put_slice(smallest) + put_slice(largest)


def deleted(t, level, number):
    return v(6) + v(t) + v(level) + v(number)


def chain(n, seed=0):
    """n tag groups of mixed kinds and lengths, 2 bytes the shortest."""
    rnd = random.Random(seed * 7919 + n)
    out = bytearray()
    for i in range(n):
        k = rnd.randrange(6)
        if k == 0:
            out += v(2) + v(rnd.randrange(1 << rnd.choice((3, 20, 62))))
        elif k == 1:
            out += deleted(rnd.randrange(2), rnd.randrange(4), rnd.randrange(1 << 40))
        elif k == 2:
            out += v(11) + v(rnd.randrange(4)) + v(rnd.randrange(1 << 30))
        elif k == 3:
            out += v(4) + v(i)
        else:
            lo, hi = sorted((rnd.randrange(1 << 30), rnd.randrange(1 << 30)))
            out += new_file(rnd.randrange(4), rnd.randrange(4), 10 + i, rnd.randrange(1 << 24),
                            ikey(b"k%09d" % lo, i + 1)[:rnd.choice((0, 1, 7, 8, 9, 18))], ikey(b"k%09d" % hi, i + 1))
    return bytes(out)


CHAIN_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4097)


def snapshot_files(n, seed=1):
    """n files over the (level, type) parts, as a snapshot lists them."""
    rnd = random.Random(seed)
    files = []
    for i in range(n):
        level = min(3, i * 4 // max(n, 1))
        files.append((rnd.randrange(2), level, 5 + i, 2 << 20 | i, bench_key(2 * i, 7), bench_key(2 * i + 1, 9)))
    return files


def all_tags():
    return (v(1) + put_slice(CMP) + v(2) + v(12) + v(9) + v(11) + v(3) + v(40) + v(4) + v(123456789)
            + deleted(0, 1, 17) + deleted(1, 3, 18) + new_file(0, 0, 19, 4096, ikey(b"a"), ikey(b"m", 9))
            + new_file(1, 2, 20, 1 << 21, ikey(b"n"), ikey(b"z", 200)) + new_file(2, 1, 21, 77, ikey(b"b"), ikey(b"c"))
            + new_file(3, 3, 22, 78, ikey(b"d"), ikey(b"e")) + v(10) + v(5) + b"".join(v(11) + v(i) + v(100 + i) for i in range(4)))


def records():
    out = [("empty", b""), ("all_tags", all_tags())]
    alone = {"comparator": v(1) + put_slice(CMP), "log_number": v(2) + v(300), "prev_log_number": v(9) + v(299),
             "next_file": v(3) + v(1 << 40), "last_sequence": v(4) + v((1 << 56) - 1), "deleted": deleted(1, 2, 99),
             "new_file": new_file(1, 3, 100, 2097152, bench_key(1), bench_key(2)), "write_cursor": v(10) + v(77),
             "read_cursor": v(11) + v(3) + v(1 << 33)}
    for name, b in alone.items():
        out.append(("alone_" + name, b))
        # each field truncated at each of its bytes
        for cut in range(1, len(b)):
            out.append((f"cut_{name}_{cut}", b[:cut]))
    out += [
        ("repeated_tags", v(2) + v(1) + v(2) + v(2) + v(1) + put_slice(b"first") + v(1) + put_slice(b"second")
         + v(10) + v(8) + v(10) + v(9) + v(11) + v(1) + v(5) + v(11) + v(1) + v(6) + v(3) + v(4) + v(3) + v(5)),
        ("repeated_files", deleted(0, 1, 5) + deleted(0, 1, 5) + deleted(1, 0, 4) + deleted(0, 0, 9)
         + new_file(1, 1, 6, 10, b"a", b"b") + new_file(0, 1, 6, 10, b"a", b"b") + new_file(1, 1, 6, 11, b"c", b"d")),
        ("unknown_tag_5", v(2) + v(1) + v(5) + v(1) + put_slice(b"key")),
        ("unknown_tag_8", v(8) + v(0)),
        ("unknown_tag_0", v(0)),
        ("unknown_tag_12", v(2) + v(7) + v(12)),
        ("unknown_tag_big", v(0xFFFFFFFF)),
        ("invalid_tag_cut", v(2) + v(7) + b"\x80"),
        ("invalid_tag_4_bytes", b"\x80\x80\x80\x80"),
        ("invalid_tag_6_bytes", b"\x82\x80\x80\x80\x80\x00" + v(5)),
        # a 5-byte tag whose bits above 2^32 are lost: tag 2
        ("tag_5_bytes_lost_bits", b"\x82\x80\x80\x80\x70" + v(44)),
        ("tag_7_two_bytes", b"\x87\x00" + new_file(1, 1, 30, 31, b"s", b"l")[1:]),
        ("varint32_6_bytes", v(6) + b"\x81\x80\x80\x80\x80\x00" + v(1) + v(2)),
        ("varint32_5_bytes_type_0", v(6) + b"\x80\x80\x80\x80\x70" + v(1) + v(2)),
        ("varint64_11_bytes", v(2) + b"\x80" * 10 + b"\x01"),
        ("varint64_10_bytes_lost_bits", v(4) + b"\xff" * 9 + b"\x7f"),
        ("level_4_deleted", deleted(0, 4, 1)),
        ("level_4_new", new_file(1, 4, 1, 1, b"a", b"b")),
        ("level_2_31", v(6) + v(0) + v(1 << 31) + v(1)),
        ("level_5_bytes_lost_bits", v(6) + v(1) + b"\x83\x80\x80\x80\x70" + v(8)),
        ("slice_one_short", v(2) + v(3) + v(1) + v(6) + b"abcde"),
        ("key_one_short", new_file(0, 0, 1, 2, b"abc", b"defg")[:-1]),
        ("empty_keys", new_file(0, 0, 1, 2, b"", b"") + new_file(1, 1, 3, 4, b"", b"x")),
        ("short_keys", new_file(0, 0, 1, 2, b"a", b"abcdefg") + new_file(0, 0, 2, 2, b"12345678", b"123456789")),
        ("long_key", new_file(1, 2, 77, 1 << 30, ikey(b"K" * 19992), ikey(b"L", 3)) + v(3) + v(78)),
        # key bytes that are themselves a well-formed run of tag groups
        ("decoy_key", new_file(0, 1, 50, 60, v(2) + v(9) + deleted(1, 1, 1) + new_file(1, 1, 2, 3, b"q", b"r"),
                               all_tags()) + v(2) + v(8)),
        ("numbers_2_63", v(2) + v(1 << 63) + v(9) + v(M64) + v(3) + v(1 << 63) + v(4) + v(M64)
         + deleted(1, 0, 1 << 63) + deleted(1, 0, M64) + new_file(0, 3, M64, 1 << 63, b"a", b"b")
         + new_file(0, 3, 1 << 63, M64, b"c", b"d") + v(10) + v(M64) + v(11) + v(0) + v(1 << 63)),
        ("snapshot_4097", mm.encode(mm.snapshot_edit(snapshot_files(4097), CMP, 9, 0, 4200, 1 << 40, 3, (1, 2, 3, 4)))),
    ]
    for n in CHAIN_LENGTHS:
        if n != 4097:
            out.append((f"chain_{n}", chain(n)))
    out.append(("chain_257_then_cut", chain(257, 3) + new_file(1, 1, 1, 1, b"abc", b"def")[:-2]))
    return [(name, b) for name, b in out if not _undefined(b)]


M64 = (1 << 64) - 1


def _undefined(b):
    code, _ = mm.decode(b)
    return code in (12, 13)


def undefined_records():
    """Input the reference must not be given: the library's verdicts 12 and 13."""
    return [("type_4_deleted", deleted(4, 1, 1)), ("type_4_new", v(2) + v(1) + new_file(4, 1, 1, 1, b"a", b"b")),
            ("type_2_32_lost_bits", v(6) + b"\x84\x80\x80\x80\x70" + v(1) + v(2)),
            ("type_4_level_4", deleted(4, 4, 1)),  # the level fails first: verdict 6
            ("type_4_cut", deleted(7, 1, 300)[:-1]),  # verdict 6
            ("cursor_4", v(11) + v(4) + v(1)), ("cursor_4_cut", v(3) + v(2) + v(11) + v(9)),
            ("cursor_2_63_cut", v(11) + v(1 << 63) + b"\x80")]


def _edit(**kw):
    e = mm.empty_edit()
    e["write_cursor"], e["read_cursors"] = 0, [0, 0, 0, 0]
    e.update(kw)
    return e


def random_edit(rnd, types=4, max_items=6):
    e = _edit()
    if rnd.random() < 0.5:
        e["comparator"] = rnd.choice((CMP, b"", b"x" * 200))
    for name in ("log_number", "prev_log_number", "next_file", "last_sequence"):
        if rnd.random() < 0.5:
            e[name] = rnd.randrange(1 << rnd.choice((1, 7, 14, 35, 63, 64)))
    e["write_cursor"] = rnd.randrange(1 << rnd.choice((1, 30, 64)))
    e["read_cursors"] = [rnd.randrange(1 << rnd.choice((1, 30, 64))) for _ in range(4)]
    for _ in range(rnd.randrange(max_items)):
        e["deleted"].append((rnd.randrange(min(types, 2)), rnd.randrange(4), rnd.randrange(12)))
    for _ in range(rnd.randrange(max_items)):
        a, b = rnd.randrange(40), rnd.randrange(40)
        e["new"].append((rnd.randrange(types), rnd.randrange(4), rnd.randrange(12), rnd.randrange(1 << 32),
                         ikey(b"u" * a, rnd.randrange(1 << 56))[:rnd.choice((0, 1, 7, 8, 9, 48))],
                         ikey(b"w" * b, rnd.randrange(1 << 56))))
    return e


def edits():
    rnd = random.Random(20)
    out = [("nothing", _edit()),
           ("all_fields", _edit(comparator=CMP, log_number=3, prev_log_number=0, next_file=1 << 35, last_sequence=M64,
                                write_cursor=1 << 63, read_cursors=[0, 127, 128, M64])),
           ("files", _edit(deleted=[(1, 3, 9), (0, 2, 1 << 40), (0, 2, 5), (1, 0, 7), (0, 2, 5)],
                           new=[(1, 0, 11, 100, ikey(b"a"), ikey(b"b")), (0, 3, 12, 200, b"", ikey(b"c")),
                                (3, 1, 13, 300, ikey(b"d"), b"e"), (1, 0, 11, 101, ikey(b"f"), ikey(b"g")),
                                (2, 2, 14, M64, ikey(b"K" * 19992), ikey(b"h"))])),
           ("snapshot_300", mm.snapshot_edit(snapshot_files(300, 5), CMP, 4, 0, 400, 99999, 2, (0, 1, 0, 1)))]
    for n in (1, 63, 64, 65, 257):
        fs = snapshot_files(n, n)
        out.append((f"items_{n}", _edit(next_file=n, deleted=[(f[0], f[1], f[2] + 7) for f in fs], new=fs)))
    for i, ln in enumerate((0, 1, 7, 8, 9, 20000)):
        out.append((f"key_{ln}", _edit(new=[(0, 1, i, 5, b"s" * ln, b"l" * ln)])))
    out += [(f"random_{i}", random_edit(rnd)) for i in range(12)]
    return out


def history(rnd, n_edits, types=2):
    """A MANIFEST's edits: adds, deletes and re-adds over a small set of file
    numbers, so that add-delete-add and delete-then-add inside one edit occur."""
    out = []
    for r in range(n_edits):
        e = mm.empty_edit()
        if r == 0 or rnd.random() < 0.3:
            e["comparator"] = CMP
        for name in ("log_number", "prev_log_number", "next_file", "last_sequence"):
            if r == 0 and name != "prev_log_number" or rnd.random() < 0.4:
                e[name] = 10 + rnd.randrange(1000)
        for _ in range(rnd.randrange(5)):
            e["deleted"].append((rnd.randrange(types), rnd.randrange(2), rnd.randrange(6)))
        for _ in range(rnd.randrange(5)):
            n = rnd.randrange(6)
            e["new"].append((rnd.randrange(types), rnd.randrange(2), n, 1000 * r + n, bench_key(n, r + 1),
                             bench_key(n + 1, r + 1)))
        if rnd.random() < 0.3 and e["new"]:  # delete-then-add of one number inside the edit
            f = e["new"][-1]
            e["deleted"].append(f[:3])
        out.append(e)
    return out


def manifests():
    rnd = random.Random(77)
    snap = mm.encode(mm.snapshot_edit(snapshot_files(900, 2), CMP, 7, 0, 1000, 5555, 1, (0, 0, 0, 0)))
    small = [mm.encode(e) for e in history(rnd, 12)]
    out = [("snapshot", [snap], None),  # a record of several blocks: FIRST, MIDDLE, LAST
           ("history", small, None),
           ("history_2", [mm.encode(e) for e in history(rnd, 40)], None),
           ("empty_file", [], None),
           ("empty_record_only", [b""], None),
           ("torn_tail", small, ("cut", 5)),
           ("torn_snapshot", [snap], ("cut", 40000)),
           ("flipped_crc", small, ("flip", 2)),
           ("flipped_payload_late", small + [snap], ("flip", 33000)),
           ("bad_record", small[:3] + [v(2) + b"\x80"] + small[3:], None),
           ("other_comparator", small[:2] + [v(1) + put_slice(b"other.Comparator")] + small[2:], None),
           ("no_next_file", [v(2) + v(1) + v(4) + v(2)], None),
           ("no_log_number", [v(3) + v(1) + v(4) + v(2)], None),
           ("no_last_sequence", [v(3) + v(1) + v(2) + v(2)], None),
           ("no_prev_log_number", [v(3) + v(9) + v(2) + v(4) + v(4) + v(2)], None),
           ("numbers_across_records", [v(3) + v(9), v(2) + v(4) + v(9) + v(3), v(4) + v(2), v(3) + v(50)], None)]
    return out


def damage(image, how):
    image = bytearray(image)
    if how is None:
        return bytes(image)
    if how[0] == "cut":
        return bytes(image[:len(image) - how[1]])
    image[how[1]] ^= 0xFF
    return bytes(image)


# ---------------------------------------------------------------- a whole database directory

DIRECTORY = dict(table_numbers=(5, 6), log_number=3, manifest_number=2, next_file=7, block_size=4096,
                 restart_interval=16)


def directory_logs():
    """Three logs of 60 WriteBatch records each over 300 user keys, puts and
    deletions: the first two become Level-0 tables, the third stays a log.
    Returns ([records], [the last sequence number of each log])."""
    rng = random.Random(4)
    users = [b"key%04d" % i for i in range(300)]
    logs, last, seq = [], [], 1
    for _ in range(3):
        recs = []
        for _ in range(60):
            ops = [(rng.choice((0, 1, 1, 1)), rng.choice(users), b"v%d-" % seq + b"x" * rng.randrange(0, 30))
                   for _ in range(rng.randrange(1, 9))]
            recs.append(struct.pack("<QI", seq, len(ops)) + b"".join(
                bytes([t, len(k)]) + k + (bytes([len(v)]) + v if t else b"") for t, k, v in ops))
            seq += len(ops)
        logs.append(recs)
        last.append(seq - 1)
    return logs, last


def directory_ops(recs):
    """The operations of a log's records in order: (type, key, value)."""
    out = []
    for r in recs:
        p = 12
        while p < len(r):
            t, kl = r[p], r[p + 1]
            key = r[p + 2:p + 2 + kl]
            p += 2 + kl
            value = b""
            if t:
                value = r[p + 1:p + 1 + r[p]]
                p += 1 + r[p]
            out.append((t, key, value))
    return out


def directory_content(logs):
    """What an iterator over the opened database yields: (live entries, the
    FNV-1a digest tests/cpp/db_verify.cc prints)."""
    state = {}
    for recs in logs:
        for t, key, value in directory_ops(recs):
            state[key] = (t, value)
    live = sorted((k, v) for k, (t, v) in state.items() if t == 1)
    h = 1469598103934665603
    for k, v in live:
        for part in (k, v):
            for i in range(8):
                h = ((h ^ ((len(part) >> (8 * i)) & 0xFF)) * 1099511628211) & M64
            for b in part:
                h = ((h ^ b) * 1099511628211) & M64
    return len(live), "%016x" % h


def directory_snapshot(files, last_sequence):
    """The directory's one MANIFEST record: files are (type, level, number, size, smallest, largest)."""
    return mm.encode(mm.snapshot_edit(files, CMP, DIRECTORY["log_number"], 0, DIRECTORY["next_file"], last_sequence, 0,
                                      (0, 0, 0, 0)))
