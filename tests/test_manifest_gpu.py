"""The batched VersionEdit on the GPU (include/lsbm_manifest.h,
lsbm_amd/manifest.py), exact against the plain-Python model
(tests/golden/manifestmodel.py) and through it against the reference's own
DecodeFrom / EncodeTo / Recover (tests/golden/manifest_fixture.*, which
tests/test_manifest.py pins the model to): every record and edit of the
fixture, chains of every length around the kernels' tile edges, records back
to back and out of order, every verdict, caps with guard bytes, the order and
bounds errors, and the chains snapshot -> frame -> read -> decode and recover.
"""
import ctypes
import random

import numpy as np
import pytest

from golden import manifest_cases as cases
from golden import manifestmodel as mm
from test_manifest import is_bytes, live_numbers, load_fixture, manifest_file, model_recover

pytestmark = pytest.mark.gpu

GUARD, FILL = 512, 0xEE
OK, NO_ROOM, BAD_INPUT = 0, 1, 2
M64 = (1 << 64) - 1
TILE = 256  # kMfThreads: the positions of one workgroup; a wave is 64 of them


def s64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def dev(torch, data):
    a = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    return torch.from_numpy(a.copy()).cuda()[:a.size - 1]


def i64(torch, rows, width=None):
    a = np.array(rows, dtype=np.int64)
    if width is not None:
        a = a.reshape(-1, width)
    return torch.from_numpy(a).cuda()


def tobytes(t):
    return t.cpu().numpy().tobytes()


def lay_out(recs, order=None, gap=0):
    """The records' bytes in an image in `order` (a permutation), `gap` filler
    bytes between them: (image bytes, [(offset, length)] in record order)."""
    order = list(range(len(recs))) if order is None else order
    img, at = bytearray(b"\xee" * gap), [None] * len(recs)
    for i in order:
        at[i] = (len(img), len(recs[i]))
        img += recs[i] + b"\xee" * gap
    return bytes(img), at


def host_edits(E, image):
    """decode_edits' result as the model's (verdict, edit) per record."""
    from lsbm_amd import manifest as mf
    verdict, fields = E.verdict.cpu().tolist(), E.fields.cpu().tolist()
    nf, df = E.new_first.cpu().tolist(), E.del_first.cpu().tolist()
    new, dele = E.new_items.cpu().tolist(), E.del_items.cpu().tolist()
    offs, keys = E.key_offsets.cpu().tolist(), tobytes(E.keys)
    assert nf[0] == 0 and df[0] == 0 and nf[-1] == len(new) and df[-1] == len(dele)
    assert offs[0] == 0 and offs[-1] == len(keys) and len(offs) == 2 * len(new) + 1
    out = []
    for r, f in enumerate(fields):
        f = [x & M64 for x in f]
        e = mm.empty_edit()
        has, rhas = f[mf.HAS], f[mf.READ_HAS]
        if has & 1:
            e["comparator"] = image[f[mf.CMP_OFF]:f[mf.CMP_OFF] + f[mf.CMP_LEN]]
        else:
            assert f[mf.CMP_OFF] == f[mf.CMP_LEN] == 0
        for bit, name, w in ((2, "log_number", mf.LOG), (4, "prev_log_number", mf.PREV_LOG), (8, "next_file", mf.NEXT_FILE),
                             (16, "last_sequence", mf.LAST_SEQ), (32, "write_cursor", mf.WRITE_CURSOR)):
            if has & bit:
                e[name] = f[w]
            else:
                assert f[w] == 0
        for i in range(4):
            if rhas >> i & 1:
                e["read_cursors"][i] = f[mf.READ + i]
            else:
                assert f[mf.READ + i] == 0
        assert has < 64 and rhas < 16
        for j in range(nf[r], nf[r + 1]):
            rec, t, level, number, size = new[j]
            assert rec == r
            e["new"].append((t, level, number & M64, size & M64, keys[offs[2 * j]:offs[2 * j + 1]],
                             keys[offs[2 * j + 1]:offs[2 * j + 2]]))
        for j in range(df[r], df[r + 1]):
            rec, t, level, number = dele[j]
            assert rec == r
            e["deleted"].append((t, level, number & M64))
        out.append((verdict[r], e))
    return out


def check_decode(torch, recs, order=None, gap=0):
    from lsbm_amd import manifest as mf
    image, at = lay_out(recs, order, gap)
    E = mf.decode_edits(dev(torch, image), i64(torch, at, 2))
    got = host_edits(E, image)
    for i, rec in enumerate(recs):
        assert got[i] == mm.decode(rec), (i, rec[:40])
    return E


def device_edits(torch, edits, sort=True):
    """The model's edits as encode's flat shapes (new files type by type, as
    the reference holds them; deleted files as given unless sort)."""
    from lsbm_amd import manifest as mf
    fields, names, dele, new, new_first, keys, offs = [], bytearray(), [], [], [0], bytearray(), [0]
    for r, e in enumerate(edits):
        f = [0] * mf.FIELD_WORDS
        if e["comparator"] is not None:
            f[mf.HAS] |= 1
            f[mf.CMP_OFF], f[mf.CMP_LEN] = len(names), len(e["comparator"])
            names += e["comparator"]
        for bit, name, w in ((2, "log_number", mf.LOG), (4, "prev_log_number", mf.PREV_LOG), (8, "next_file", mf.NEXT_FILE),
                             (16, "last_sequence", mf.LAST_SEQ)):
            if e[name] is not None:
                f[mf.HAS] |= bit
                f[w] = s64(e[name])
        f[mf.WRITE_CURSOR] = s64(e["write_cursor"] or 0)
        f[mf.READ:mf.READ + 4] = [s64(v or 0) for v in e["read_cursors"]]
        fields.append(f)
        ds = sorted(set(e["deleted"])) if sort else e["deleted"]
        dele += [[r, t, level, s64(number)] for t, level, number in ds]
        for t, level, number, size, a, b in sorted(e["new"], key=lambda x: x[0]):
            new.append([r, t, level, s64(number), s64(size)])
            keys += a
            offs.append(len(keys))
            keys += b
            offs.append(len(keys))
        new_first.append(len(new))
    return dict(fields=i64(torch, fields, mf.FIELD_WORDS), names=dev(torch, names), del_items=i64(torch, dele, 4),
                new_first=i64(torch, new_first), new_items=i64(torch, new, 5), keys=dev(torch, keys),
                key_offsets=i64(torch, offs))


def encode(torch, edits):
    from lsbm_amd import manifest as mf
    r = mf.encode_edits(**device_edits(torch, edits))
    image, recs = tobytes(r.image), r.records.cpu().tolist()
    at = 0
    for off, ln in recs:  # back to back from 0
        assert off == at
        at += ln
    assert at == len(image)
    return [image[off:off + ln] for off, ln in recs]


# ---------------------------------------------------------------- decode

def test_decode_every_fixture_record_in_one_call(torch_cuda):
    """All records of the fixture and the undefined-input ones (verdicts 1-13),
    laid out in descending and interleaved offset order with no gap, empty
    records between them: each equals the model's (and so the reference's)
    verdict and edit, later records unaffected by earlier ones' errors."""
    _, body = load_fixture()
    named = cases.records() + cases.undefined_records()
    recs = []
    for _, b in named:
        recs += [b, b""]
    rnd = random.Random(5)
    order = list(range(len(recs)))
    E = check_decode(torch_cuda, recs, order[::-1])
    seen = set(E.verdict.cpu().tolist())
    assert seen == set(range(14))
    rnd.shuffle(order)
    check_decode(torch_cuda, recs, order)
    for i, (name, _) in enumerate(cases.records()):
        assert mm.status_string(E.verdict[2 * i].item()) == body["records"][name]["status"], name


def test_decode_chain_lengths(torch_cuda):
    """Chains of every length around a wave's and a workgroup's positions, one
    call each way: alone (the record starts at position 0) and all together."""
    chains = [cases.chain(n, seed=9) for n in cases.CHAIN_LENGTHS]
    for c in chains[:6] + chains[-1:]:
        check_decode(torch_cuda, [c])
    check_decode(torch_cuda, chains, gap=3)


def test_decode_groups_straddling_tile_edges(torch_cuda):
    """A new-file group (and its keys) across every edge of the kernels' tiles:
    position 64 (wave), 256 (workgroup), and the same in a second record whose
    positions start mid-tile."""
    two = mm.put_varint(4) + mm.put_varint(1)
    big = cases.new_file(1, 2, 77, 1 << 33, cases.bench_key(1), cases.bench_key(2))
    assert len(big) > 40
    recs = []
    for edge in (64, TILE, 2 * TILE, 5 * TILE):
        for before in (1, 2, 20, len(big) - 1):
            start = edge - before
            start -= start % 2
            rec = two * (start // 2) + big + two * 3
            recs.append(rec)
            check_decode(torch_cuda, [rec])
    check_decode(torch_cuda, recs)


def test_decode_stops_at_the_record_s_end(torch_cuda):
    """Records back to back with no gap, the first ending in a truncated group
    that the neighbour's first bytes would complete: the parse stops at the
    record's end and the neighbour decodes as if alone."""
    whole = cases.new_file(1, 1, 9, 10, b"abcdefgh", b"ijklmnop") + mm.put_varint(3) + mm.put_varint(7)
    for cut in (1, 3, 5, 9, 15, len(whole) - 4):
        a, b = cases.chain(65, 1) + whole[:cut], whole[cut:]
        image, at = lay_out([a, b])
        assert at[1][0] == len(a)
        E = check_decode(torch_cuda, [a, b])
        v = E.verdict.cpu().tolist()
        assert v[0] != 0 and v == [mm.decode(a)[0], mm.decode(b)[0]]
        check_decode(torch_cuda, [b, a], order=[1, 0])


def test_decode_decoy_keys(torch_cuda):
    """Key bytes that are a well-formed run of tag groups: positions inside
    them parse, but no chain from a record's first byte reaches them."""
    decoy = dict(cases.records())["decoy_key"]
    E = check_decode(torch_cuda, [decoy, decoy + decoy, b"", decoy])
    assert E.new_first.cpu().tolist() == [0, 1, 3, 3, 4] and E.del_first.cpu().tolist() == [0] * 5


def _raw_decode_emit(torch, image, records, plan, new_cap, del_cap, keys_cap):
    """lsbm_edit_decode_emit_dev into buffers with guard bytes behind the caps."""
    from lsbm_amd import lib
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g64, fill64 = GUARD // 8, int.from_bytes(bytes([FILL]) * 8, "little", signed=True)
    new = torch.full((5 * new_cap + g64,), fill64, dtype=torch.int64, device="cuda")
    dele = torch.full((4 * del_cap + g64,), fill64, dtype=torch.int64, device="cuda")
    offs = torch.full((2 * new_cap + 1 + g64,), fill64, dtype=torch.int64, device="cuda")
    keys = torch.full((keys_cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    rc = lib().lsbm_edit_decode_emit_dev(P(image), image.numel(), P(records), records.numel() // 2, plan.span_cap, P(new),
                                         new_cap, P(offs), P(keys), keys_cap, P(dele), del_cap, P(status),
                                         P(plan.scratch), plan.scratch.numel() * 8,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return new, dele, offs, keys, status.item(), fill64


def test_decode_caps_and_guards(torch_cuda):
    """Caps exactly the totals: every guard byte intact.  Caps one item or one
    key byte short: LSBM_MERGE_NO_ROOM and nothing stored."""
    from lsbm_amd import manifest as mf
    torch = torch_cuda
    recs = [cases.chain(257, 4), cases.all_tags(), b"", cases.chain(64, 2)]
    image, at = lay_out(recs)
    d_image, d_rec = dev(torch, image), i64(torch, at, 2)
    span, longest = sum(len(r) for r in recs), max(len(r) for r in recs)
    plan = mf.decode_plan(d_image, d_rec, span, longest)
    n_new, n_del, kb = plan.totals.cpu().tolist()
    want = [mm.decode(r)[1] for r in recs]
    assert n_new == sum(len(e["new"]) for e in want) and n_del == sum(len(e["deleted"]) for e in want)
    assert kb == sum(len(f[4]) + len(f[5]) for e in want for f in e["new"]) and plan.status.item() == OK
    new, dele, offs, keys, st, fill64 = _raw_decode_emit(torch, d_image, d_rec, plan, n_new, n_del, kb)
    assert st == OK
    assert (new[5 * n_new:] == fill64).all() and (dele[4 * n_del:] == fill64).all()
    assert (offs[2 * n_new + 1:] == fill64).all() and (keys[kb:] == FILL).all()
    E = mf.Edits(plan.verdict, plan.fields, plan.new_first, new[:5 * n_new].reshape(-1, 5), offs[:2 * n_new + 1],
                 keys[:kb], plan.del_first, dele[:4 * n_del].reshape(-1, 4))
    assert [e for _, e in host_edits(E, image)] == want
    for caps in ((n_new - 1, n_del, kb), (n_new, n_del - 1, kb), (n_new, n_del, kb - 1)):
        new, dele, offs, keys, st, _ = _raw_decode_emit(torch, d_image, d_rec, plan, *caps)
        assert st == NO_ROOM, caps
        assert (new == fill64).all() and (dele == fill64).all() and (offs == fill64).all() and (keys == FILL).all()
    # the plan's own caps: a span or a longest record one byte short
    for sc, lc in ((span - 1, longest), (span, longest - 1)):
        p = mf.decode_plan(d_image, d_rec, sc, lc)
        assert p.status.item() == NO_ROOM
        assert p.verdict.cpu().tolist() == [0] * 4 and p.totals.cpu().tolist() == [0, 0, 0]
        assert not p.fields.any() and not p.new_first.any() and not p.del_first.any()


def test_decode_bad_record_bounds(torch_cuda):
    from lsbm_amd import manifest as mf
    torch = torch_cuda
    image = cases.all_tags()
    d_image = dev(torch, image)
    for bad in ([0, len(image) + 1], [len(image) + 1, 0], [5, len(image) - 4], [1 << 61, 1]):
        p = mf.decode_plan(d_image, i64(torch, [[0, len(image)], bad, [0, 3]], 2), 3 * len(image), len(image))
        assert p.status.item() == BAD_INPUT, bad
        assert p.verdict.cpu().tolist() == [0] * 3 and p.totals.cpu().tolist() == [0, 0, 0] and not p.fields.any()
    p = mf.decode_plan(d_image, i64(torch, [[0, len(image)], [len(image), 0], [0, 3]], 2), 3 * len(image), len(image))
    assert p.status.item() == OK and p.verdict.cpu().tolist() == [0, 0, mm.decode(image[:3])[0]]


# ---------------------------------------------------------------- encode

def test_encode_every_fixture_edit(torch_cuda):
    """EncodeTo's recorded bytes for every edit description, each alone and all
    in one call."""
    _, body = load_fixture()
    named = cases.edits()
    got = encode(torch_cuda, [e for _, e in named])
    for (name, e), b in zip(named, got):
        assert b == mm.encode(e), name
        assert is_bytes(body["edits"][name], b), name
    for name, e in named[:4]:
        assert encode(torch_cuda, [e]) == [mm.encode(e)], name
    assert encode(torch_cuda, []) == []


def test_encode_random_edits_and_back(torch_cuda):
    """decode(encode(x)) == canonical(x) through the device both ways."""
    from lsbm_amd import manifest as mf
    rnd = random.Random(3)
    edits = [cases.random_edit(rnd, max_items=9) for _ in range(300)]
    d = device_edits(torch_cuda, edits, sort=False)  # (the wrapper sorts and de-duplicates the deleted files)
    r = mf.encode_edits(**d)
    image = tobytes(r.image)
    recs = [image[o:o + n] for o, n in r.records.cpu().tolist()]
    assert recs == [mm.encode(e) for e in edits]
    back = host_edits(mf.decode_edits(r.image, r.records), image)
    assert back == [(0, mm.canonical(e)) for e in edits]


def _plan(torch, d, out_at=0):
    from lsbm_amd import manifest as mf
    return mf.encode_plan(d["fields"], d["names"], d["del_first"], d["del_items"], d["new_first"], d["new_items"], d["keys"],
                          d["key_offsets"], out_at)


def test_encode_rejects_bad_order_and_bounds(torch_cuda):
    """Every violation the header lists: LSBM_MERGE_BAD_INPUT, records and
    totals untouched."""
    from lsbm_amd import manifest as mf
    torch = torch_cuda
    base = [cases._edit(deleted=[(0, 1, 5), (0, 2, 3), (1, 0, 9)],
                        new=[(0, 1, 1, 10, b"a", b"b"), (1, 1, 2, 20, b"cc", b"dd"), (3, 0, 3, 30, b"", b"e")]),
            cases._edit(comparator=b"cmp", deleted=[(1, 3, M64)], new=[(2, 3, 4, 40, b"f", b"g")])]

    def arrays():
        d = device_edits(torch, base)
        d["del_first"], d["del_items"] = mf.sort_deleted(d["del_items"], len(base))
        return d
    assert _plan(torch, arrays()).status.item() == OK

    def poke(*changes):
        d = arrays()
        for name, index, value in changes:
            d[name].view(-1)[index] = value
        return d
    # deleted rows: 0 (0, 1, 5), 1 (0, 2, 3), 2 (1, 0, 9) of edit 0, 3 (1, 3, 2^64 - 1) of edit 1
    # new rows: 0 (0, 1, 1), 1 (1, 1, 2), 2 (3, 0, 3) of edit 0, 3 (2, 3, 4) of edit 1; key offsets [0, 1, 2, 4, 6, 6, 7, 8, 9]
    assert arrays()["key_offsets"].cpu().tolist() == [0, 1, 2, 4, 6, 6, 7, 8, 9]
    assert _plan(torch, poke(("new_items", 5 * 2 + 1, 1))).status.item() == OK  # equal types: non-descending
    bad = {"deleted descending": poke(("del_items", 4 * 1 + 2, 0)),
           "deleted equal": poke(("del_items", 4 * 1 + 2, 1), ("del_items", 4 * 1 + 3, 5)),
           "deleted type 4": poke(("del_items", 4 * 2 + 1, 4)),
           "deleted level 4": poke(("del_items", 4 * 3 + 2, 4)),
           "deleted record": poke(("del_items", 4 * 3, 0)),
           "new types descend": poke(("new_items", 5 * 0 + 1, 2)),
           "new type 4": poke(("new_items", 5 * 3 + 1, 4)),
           "new level 4": poke(("new_items", 5 * 2 + 2, 4)),
           "new record": poke(("new_items", 5 * 3, 0)),
           "del_first start": poke(("del_first", 0, 1)),
           "del_first end": poke(("del_first", 2, 3)),
           "del_first past": poke(("del_first", 1, 5)),
           "new_first end": poke(("new_first", 2, 5)),
           "key offsets decrease": poke(("key_offsets", 3, 1)),
           "key offsets pass": poke(("key_offsets", 8, 1 << 40)),
           "comparator passes": poke(("fields", 13 + mf.CMP_LEN, 4)),
           "comparator offset": poke(("fields", 13 + mf.CMP_OFF, 1))}
    for what, d in bad.items():
        p = _plan(torch, d)
        assert p.status.item() == BAD_INPUT, what
        assert not p.records.any() and p.totals.item() == 0, what


def test_encode_caps_and_guards(torch_cuda):
    """out_cap exactly the plan's bytes inside a larger image at out_at: guard
    bytes intact on both sides.  One byte short: LSBM_MERGE_NO_ROOM, nothing
    stored."""
    from lsbm_amd import manifest as mf
    torch = torch_cuda
    edits = [e for _, e in cases.edits()[:8]]
    d = device_edits(torch, edits)
    d["del_first"], d["del_items"] = mf.sort_deleted(d["del_items"], len(edits))
    out_at = GUARD + 3
    p = _plan(torch, d, out_at)
    total = p.totals.item()
    want = b"".join(mm.encode(e) for e in edits)
    assert total == len(want) and p.status.item() == OK
    args = (d["fields"], d["names"], d["del_first"], d["del_items"], d["new_first"], d["new_items"], d["keys"],
            d["key_offsets"], p)
    out = torch.full((out_at + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert mf.encode_emit(*args, out, out_at, total).item() == OK
    host = tobytes(out)
    assert host == bytes([FILL]) * out_at + want + bytes([FILL]) * GUARD
    assert p.records.cpu().tolist()[0] == [out_at, len(mm.encode(edits[0]))]
    out.fill_(FILL)
    assert mf.encode_emit(*args, out, out_at, total - 1).item() == NO_ROOM
    assert (out == FILL).all()


# ---------------------------------------------------------------- chains

def file_table(torch, files):
    """A device-resident FileTable of the model's (type, level, number, size, smallest, largest)."""
    from lsbm_amd import manifest as mf
    keys, offs = bytearray(), [0]
    for f in files:
        for k in f[4:6]:
            keys += k
            offs.append(len(keys))
    col = lambda i: i64(torch, [s64(f[i]) for f in files])  # noqa: E731
    return mf.FileTable(col(2), col(3), col(1), col(0), dev(torch, keys), i64(torch, offs))


def test_snapshot_frame_read_decode_round_trip(torch_cuda):
    """snapshot -> write.frame_records -> log.read_records -> decode_edits
    gives back the file table; the record is the model's WriteSnapshot."""
    from lsbm_amd import log, manifest as mf, write
    torch = torch_cuda
    rnd = random.Random(8)
    files = cases.snapshot_files(4097, 3)
    rnd.shuffle(files)
    files = [(rnd.randrange(4),) + f[1:] for f in files]
    numbers = dict(log_number=12, prev_log_number=0, next_file=5000, last_sequence=1 << 50, write_cursor=M64,
                   read_cursors=(1, 0, 1 << 63, 3))
    s = mf.snapshot(file_table(torch, files), **numbers)
    want = mm.encode(mm.snapshot_edit(files, **numbers))
    assert tobytes(s.image) == want and s.records.cpu().tolist() == [[0, len(want)]]
    framed = write.frame_records(s.image, s.records)
    r = log.read_records(framed.log)
    assert r.events.numel() == 0 and r.records.shape[0] == 1
    image = tobytes(r.image)
    (code, e), = host_edits(mf.decode_edits(r.image, r.records), image)
    assert code == 0 and e == mm.decode(want)[1]
    assert sorted(e["new"]) == sorted(files)


def test_recover_the_fixture_s_manifests(torch_cuda, oracle):
    """recover over every MANIFEST of the fixture, torn tails and flipped bytes
    included: the reference's recorded status text, numbers and live set, and
    the model's live files per (level, type)."""
    from lsbm_amd import manifest as mf
    torch = torch_cuda
    _, body = load_fixture()
    for name, payloads, how in cases.manifests():
        want = body["manifests"][name]
        image = cases.damage(manifest_file(oracle, payloads), how)
        got = mf.recover(dev(torch, image))
        assert got.status == want["status"], name
        assert got.ok == (want["status"] == "OK")
        if got.ok:
            model = model_recover(oracle, image)
            assert (got.last_sequence, got.log_number, got.prev_log_number, got.manifest_file_number) == tuple(
                want[k] for k in ("last_sequence", "log_number", "prev_log_number", "manifest_file_number")), name
            assert got.next_file_number == want["manifest_file_number"] + 1
            assert got.files == model["files"], name
            assert live_numbers({"files": got.files}) == want["live"], name
    other = mf.recover(dev(torch, manifest_file(oracle, cases.manifests()[1][1])), comparator=b"mine")
    assert other.status == "Invalid argument: leveldb.BytewiseComparator does not match existing comparator : mine"


def test_manifest_image_is_the_reference_writer_s_file(torch_cuda, oracle):
    """manifest_image: the snapshot framed and sealed is byte for byte the file
    the reference's log::Writer wrote for the same record (the fixture's
    `snapshot` MANIFEST), and recover reads it back."""
    from lsbm_amd import manifest as mf
    torch = torch_cuda
    _, body = load_fixture()
    files = cases.snapshot_files(900, 2)
    m = mf.manifest_image(file_table(torch, files), comparator=cases.CMP, log_number=7, prev_log_number=0, next_file=1000,
                          last_sequence=5555, write_cursor=1, read_cursors=(0, 0, 0, 0))
    assert is_bytes(body["manifests"]["snapshot"]["file"], tobytes(m.log))
    got = mf.recover(m.log)
    assert got.status == "OK" and got.write_cursor == 1 and got.read_cursors == (0, 0, 0, 0)
    assert live_numbers({"files": got.files}) == body["manifests"]["snapshot"]["live"]
    assert sorted(f for fs in got.files.values() for f in fs) == sorted(f[2:] for f in files)
