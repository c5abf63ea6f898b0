"""The batched log::Reader on the GPU (include/lsbm_log_read.h,
lsbm_amd/log.py read_records, lsbm_amd/memtable.py recover), exact against the
plain-Python model (tests/golden/logreadmodel.py) and through it against the
reference's own reader: every scenario of tests/golden/log_fixture.json and
tests/golden/logread_fixture.json, each step against the model's arrays, the
round trip through write.write_batches, caps with guard bytes, and a log past
4 GiB.
"""
import numpy as np
import pytest

from golden import logreadmodel as model
from golden import write_cases as wc
from golden.splitmix import printable_bytes
from test_log_read import load, ok_by, wal_image

pytestmark = pytest.mark.gpu

B = model.BLOCK
GUARD, FILL = 4096, 0xEE
NO_ROOM, BAD_INPUT = 1, 2


def dev(torch, data, lead=0):
    """A uint8 device tensor of the bytes, a view `lead` bytes into its
    allocation: the log then starts at any address phase."""
    a = np.frombuffer(bytes(lead) + bytes(data) + b"\0", dtype=np.uint8)
    return torch.from_numpy(a.copy()).cuda()[lead:a.size - 1]


def tobytes(t):
    return t.cpu().numpy().tobytes()


def check_read(torch, oracle, img, initial_offset, want_text=None, lead=0):
    """read_records against the model: records, last_record_offset, events,
    every record's bytes, the rendered text."""
    from lsbm_amd import log
    img = np.asarray(img, dtype=np.uint8)
    w, p, e = model.read(img, ok_by(oracle), initial_offset)
    r = log.read_records(dev(torch, img.tobytes(), lead), initial_offset=initial_offset)
    assert r.records.cpu().numpy().reshape(-1, 2).tolist() == e.records.tolist()
    assert r.last_record_offset.cpu().tolist() == e.last_record_offset.tolist()
    assert r.events.cpu().numpy().reshape(-1, 4).tolist() == e.events.tolist()
    host = tobytes(r.image)
    assert host[:img.size] == img.tobytes() and host[img.size:] == e.side.tobytes()
    text = log.event_text(r, host, oracle.value)
    assert text == model.event_text(e, model.record_bytes(img, p), oracle.value)
    if want_text is not None:
        assert text == want_text
    return r


def test_read_records_on_the_wal_fixture(torch_cuda, oracle):
    """All 46 scenarios of the reference's fixture (458,511 bytes each)."""
    d = load("log_fixture.json")
    base = wal_image(d)
    assert base.size == 458511
    for i, s in enumerate(d["scenarios"] + d["offset_scenarios"]):
        check_read(torch_cuda, oracle, model.apply_edits(base, s["ops"]), s.get("initial_offset", 0), s["events"],
                   lead=i % 16)


def test_read_records_on_the_hand_framed_images(torch_cuda, oracle):
    d = load("logread_fixture.json")
    payload = printable_bytes(d["seed"], d["payload_bytes"])
    for i, s in enumerate(d["scenarios"]):
        img = model.frame_image(s["frame"], s["edits"], payload, oracle.value)
        for r in s["reads"]:
            check_read(torch_cuda, oracle, img, r["initial_offset"], r["events"], lead=(5 * i + 3) % 16)


def run_steps(torch, image, log_at, n, initial_offset, ok_of, side_at, side_cap):
    """walk (count, then list), plan with the given CRC results, emit."""
    from lsbm_amd import log
    nh = int(log.walk(image, log_at, n, initial_offset).n_headers.cpu()[0])
    w = log.walk(image, log_at, n, initial_offset, headers_cap=nh)
    ok = ok_of(w.headers)
    p = log.plan(image, log_at, n, initial_offset, w.block_first, w.block_end, w.headers, ok)
    t = p.totals.cpu().tolist()
    e = log.emit(image, log_at, n, initial_offset, p, side_at, side_cap, t[0], t[1])
    return nh, w, p, t, e


def test_each_step_against_the_model(torch_cuda, oracle):
    """walk, plan and emit one by one, with the model's CRC results going into
    plan: a wrong walk is not repaired by the steps after it."""
    torch = torch_cuda
    d = load("logread_fixture.json")
    payload = printable_bytes(d["seed"], d["payload_bytes"])
    for i, s in enumerate(d["scenarios"]):
        img = model.frame_image(s["frame"], s["edits"], payload, oracle.value)
        for rd in s["reads"][:3]:
            off = rd["initial_offset"]
            w, p, e = model.read(img, ok_by(oracle), off, log_at=7, side_at=7 + img.size + 9)
            ok = ok_by(oracle)(img, w.headers)
            image = dev(torch, b"\x11" * 7 + img.tobytes() + b"\x22" * (9 + p.side_bytes + 5), lead=i % 16)
            ok_of = lambda h: torch.from_numpy(np.asarray(ok, dtype=np.uint8).copy()).cuda()[:h.numel()]  # noqa: E731
            nh, gw, gp, totals, ge = run_steps(torch, image, 7, img.size, off, ok_of, 7 + img.size + 9, p.side_bytes)
            note = (s["name"], off)
            assert nh == w.headers.size, note
            assert gw.block_first.cpu().tolist() == w.block_first.tolist(), note
            assert gw.block_end.cpu().numpy().reshape(-1, 2).tolist() == w.block_end.tolist(), note
            assert gw.headers.cpu().tolist() == w.headers.tolist(), note
            assert [int(x.cpu()[0]) for x in (gw.status, gp.status, ge.status)] == [0, 0, 0], note
            assert totals == [len(p.records), len(p.events), p.side_bytes, p.stop], note
            assert ge.records.cpu().numpy().reshape(-1, 2).tolist() == e.records.tolist(), note
            assert ge.last_record_offset.cpu().tolist() == e.last_record_offset.tolist(), note
            assert ge.events.cpu().numpy().reshape(-1, 4).tolist() == e.events.tolist(), note
            host = tobytes(image)
            at = 7 + img.size + 9
            assert host[at:at + p.side_bytes] == e.side.tobytes(), note
            assert host[:at] == b"\x11" * 7 + img.tobytes() + b"\x22" * 9 and host[at + p.side_bytes:] == b"\x22" * 5


@pytest.fixture(scope="module")
def writes():
    return wc.load()[0]


@pytest.mark.parametrize("name", ["encoding", "ops_65_257", "leader_131072_exact"])
def test_round_trip_through_write_batches(torch_cuda, oracle, writes, name):
    """What write.write_batches frames, read_records returns: the reps byte for
    byte and no event; memtable.recover of the log is memtable.flush of the
    reps.  "encoding" has reps over 32,761 bytes and empty batches."""
    torch = torch_cuda
    from lsbm_amd import log, memtable, write
    from test_write_gpu import dev_ops
    c = [c for c in writes if c["name"] == name][0]
    ops, sync = dev_ops(torch, wc.writers_of(c["writers"]))
    w = write.write_batches(sync=sync, last_sequence=c["last_sequence"], **ops)
    assert tobytes(w.log) == c["log"]
    r = log.read_records(w.log)
    assert r.events.numel() == 0
    host = tobytes(r.image)
    assert [host[o:o + n] for o, n in r.records.cpu().numpy().reshape(-1, 2).tolist()] == c["reps"]
    assert name != "encoding" or max(len(x) for x in c["reps"]) > B - 7 and any(not ops for _, ops in c["writers"])
    got = memtable.recover(w.log, bits_per_key=10)
    want = memtable.flush(w.reps, w.records, bits_per_key=10)
    assert got.status is None and got.events.numel() == 0
    assert (got.flush.image is None) == (want.image is None)
    if want.image is not None:
        assert tobytes(got.flush.image) == tobytes(want.image)
        assert (got.flush.smallest, got.flush.largest) == (want.smallest, want.largest)
    assert got.flush.max_sequence == want.max_sequence and got.flush.status.tolist() == want.status.tolist()


def test_records_that_end_near_a_block_end(torch_cuda, oracle, writes):
    """write.frame_records over payloads that end 0..7 bytes before a block's
    end (the zero trailers, the zero-length FIRST), read back."""
    torch = torch_cuda
    from lsbm_amd import write
    spec = [p for n, p in wc.log_specs() if n == "ends"][0]
    payloads = [wc.pattern(seed, n) for n, seed in spec]
    image = dev(torch, b"".join(payloads))
    offs = np.concatenate([[0], np.cumsum([len(p) for p in payloads])]).astype(np.int64)
    rec = torch.tensor([x for i, p in enumerate(payloads) for x in (int(offs[i]), len(p))], dtype=torch.int64,
                       device="cuda")
    f = write.frame_records(image, rec)
    r = check_read(torch, oracle, np.frombuffer(tobytes(f.log), np.uint8), 0)
    host = tobytes(r.image)
    assert r.events.numel() == 0
    assert [host[o:o + n] for o, n in r.records.cpu().numpy().reshape(-1, 2).tolist()] == payloads


@pytest.fixture(scope="module")
def small_log(torch_cuda):
    """Twelve write.write_batches calls of one small writer each, appended: a
    log of twelve unfragmented records.  (log bytes, reps)."""
    from lsbm_amd import write
    from test_write_gpu import dev_ops
    log_bytes, reps, seq = b"", [], 100
    for i in range(12):
        ops = [(1, 3 + i, i, 20 + 7 * i, 50 + i), (0, 4, 2 * i, 0, 0), (1, 1, 9 * i, 0, 3)]
        d, sync = dev_ops(torch_cuda, wc.writers_of([(0, ops)]))
        w = write.write_batches(sync=sync, last_sequence=seq, log_offset=len(log_bytes), **d)
        log_bytes += tobytes(w.log)
        reps.append(tobytes(w.reps))
        seq = w.last_sequence
    return log_bytes, reps


def flush_of(torch, reps):
    from lsbm_amd import memtable
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reps])]).astype(np.int64)
    rec = torch.tensor([x for i, r in enumerate(reps) for x in (int(offs[i]), len(r))], dtype=torch.int64, device="cuda")
    return memtable.flush(dev(torch, b"".join(reps)), rec)


def same_table(got, want):
    assert (got.image is None) == (want.image is None)
    if want.image is not None:
        assert tobytes(got.image) == tobytes(want.image)
        assert (got.smallest, got.largest) == (want.smallest, want.largest)
    assert got.max_sequence == want.max_sequence


def test_torn_tail_recovers_the_prefix(torch_cuda, oracle, small_log):
    """A log cut inside an unfragmented record: the records before it, and one
    `truncated record at end of file` or `bad record length` report, as the
    model says; recover inserts the prefix."""
    torch = torch_cuda
    from lsbm_amd import memtable
    c = {"log": small_log[0], "reps": small_log[1]}
    whole = np.frombuffer(c["log"], np.uint8)
    full = model.walk(whole).headers.tolist()
    assert len(full) == 12 and all(whole[h + 6] == 1 for h in full)
    reasons = set()
    for cut in (full[-1] + 3, full[-1] + 7 + 2, full[len(full) // 2] + 1, full[len(full) // 2] + 7, len(whole) - 1):
        img = whole[:cut]
        r = check_read(torch, oracle, img, 0)
        ev = r.events.cpu().numpy().reshape(-1, 4).tolist()
        n = r.records.numel() // 2
        assert len(ev) == 1 and ev[0][0] == n and ev[0][2] in (1, 3) and 0 < n < len(c["reps"])
        reasons.add(ev[0][2])
        host = tobytes(r.image)
        assert [host[o:o + k] for o, k in r.records.cpu().numpy().reshape(-1, 2).tolist()] == c["reps"][:n]
        got = memtable.recover(dev(torch, img.tobytes()))
        same_table(got.flush, flush_of(torch, c["reps"][:n]))
        assert got.status is None and got.events.cpu().numpy().reshape(-1, 4).tolist() == ev
    assert reasons == {1, 3}


def test_recover_paranoid_stops_at_the_first_report(torch_cuda, oracle, small_log):
    """payload_flip_full of the WAL fixture: the first report is where the
    reference's is.  The same flip in a log of WriteBatches with
    paranoid_checks: the table holds exactly the records returned before the
    reporting call."""
    torch = torch_cuda
    from lsbm_amd import log, memtable
    d = load("log_fixture.json")
    s = [s for s in d["scenarios"] if s["name"] == "payload_flip_full"][0]
    r = log.read_records(dev(torch, model.apply_edits(wal_image(d), s["ops"]).tobytes()))
    first = r.events.cpu().numpy().reshape(-1, 4).tolist()[0]
    lines = s["events"].splitlines()
    assert lines.index("D %d Corruption: checksum mismatch" % first[1]) == first[0] and first[2] == 2
    c = {"log": small_log[0], "reps": small_log[1]}
    img = np.frombuffer(c["log"], np.uint8).copy()
    full = model.walk(img).headers.tolist()
    img[full[len(full) // 2] + 7 + 3] ^= 0x10
    _, p, _ = model.read(img, ok_by(oracle), 0)
    k = p.events[0][0]
    assert p.events[0][2] == 2 and 0 < k == len(p.records)  # (the rest of the block goes with the flipped record)
    got = memtable.recover(dev(torch, img.tobytes()), paranoid=True)
    assert got.status == "Corruption: checksum mismatch"
    assert got.events.cpu().numpy().reshape(-1, 4).tolist() == [list(e) for e in p.events]
    same_table(got.flush, flush_of(torch, c["reps"][:k]))
    same_table(memtable.recover(dev(torch, img.tobytes())).flush, flush_of(torch, c["reps"][:k]))
    # a report that comes with a record: FULL, a FIRST that never ends, FULL, FULL.  The second FULL's call
    # reports `partial record without end(1)` and returns the record, which paranoid_checks then does not insert.
    reps = c["reps"][:3]
    frame = [["p", 1, len(reps[0])], ["p", 2, 10], ["p", 1, len(reps[1])], ["p", 1, len(reps[2])]]
    payload = np.frombuffer(reps[0] + bytes(10) + reps[1] + reps[2], np.uint8)
    img = model.frame_image(frame, [], payload, oracle.value)
    got = memtable.recover(dev(torch, img.tobytes()), paranoid=True)
    assert got.status == "Corruption: partial record without end(1)"
    assert got.events.cpu().numpy().reshape(-1, 4).tolist() == [[1, 10, 4, 0]]
    same_table(got.flush, flush_of(torch, reps[:1]))
    loose = memtable.recover(dev(torch, img.tobytes()))
    assert loose.status is None and loose.events.cpu().numpy().reshape(-1, 4).tolist() == [[1, 10, 4, 0]]
    same_table(loose.flush, flush_of(torch, reps))


def guarded(torch, n, dtype):
    """(whole, window): n elements with 4 KiB of 0xEE bytes on either side."""
    per = 1 if dtype == torch.uint8 else 8
    whole = torch.full((2 * GUARD + n * per,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + n * per].view(dtype)


def test_caps_tampering_and_overlap(torch_cuda, oracle):
    """Caps one short: LSBM_MERGE_NO_ROOM, the guards and every other output
    untouched.  A tampered block_first or headers into plan:
    LSBM_MERGE_BAD_INPUT.  A side area that overlaps the log: LSBM_ERR_INVALID."""
    torch = torch_cuda
    from lsbm_amd import log
    from lsbm_amd._lib import LSBM_ERR_INVALID, LsbmError, lib
    from lsbm_amd.engine import _ptr
    d = load("logread_fixture.json")
    s = [s for s in d["scenarios"] if s["name"] == "checksum_in_two_adjacent_blocks"][0]
    s2 = [s for s in d["scenarios"] if s["name"] == "five_blocks_clean"][0]
    payload = printable_bytes(d["seed"], d["payload_bytes"])
    for sc in (s, s2):
        img = model.frame_image(sc["frame"], sc["edits"], payload, oracle.value)
        n = img.size
        w, p, e = model.read(img, ok_by(oracle), 0, side_at=n + GUARD)
        assert len(p.events) >= (2 if sc is s else 0) and (p.side_bytes > 0) == (sc is s2)
        nh, nb, nr, ne = w.headers.size, w.block_end.shape[0], len(p.records), len(p.events)
        side_at = n + GUARD
        whole_img = torch.full((n + 2 * GUARD + p.side_bytes,), FILL, dtype=torch.uint8, device="cuda")
        whole_img[:n] = dev(torch, img.tobytes())
        before = tobytes(whole_img)
        # walk: headers_cap one short
        hw, hv = guarded(torch, max(nh - 1, 1), torch.int64)
        bf_w, bf = guarded(torch, nb + 1, torch.int64)
        be_w, be = guarded(torch, 2 * nb, torch.int64)
        nhd_w, nhd = guarded(torch, 1, torch.int64)
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        scratch = torch.empty(3 * nb + 1, dtype=torch.int64, device="cuda")

        def call_walk(cap):
            return lib().lsbm_log_read_walk_dev(_ptr(whole_img), whole_img.numel(), 0, n, 0, _ptr(bf), _ptr(be), nb,
                                                _ptr(hv), cap, _ptr(nhd), _ptr(st), _ptr(scratch), scratch.numel() * 8,
                                                None)
        assert call_walk(nh - 1) == 0 and int(st.cpu()[0]) == NO_ROOM
        for t in (hw, bf_w, be_w, nhd_w):
            assert bool((t == FILL).all())
        # the real walk, then plan with tampered arrays
        gw = log.walk(whole_img, 0, n, 0, headers_cap=nh)
        assert gw.headers.cpu().tolist() == w.headers.tolist()
        ok = torch.from_numpy(np.asarray(ok_by(oracle)(img, w.headers), dtype=np.uint8).copy()).cuda()
        for what in ("block_first", "headers", "block_end"):
            bad = {k: getattr(gw, k).clone() for k in ("block_first", "block_end", "headers")}
            if what == "block_first":
                bad[what][1] += 1
            elif what == "headers":
                bad[what][nh - 1] += 1
            else:
                bad[what][0, 1] += 1
            gp = log.plan(whole_img, 0, n, 0, bad["block_first"], bad["block_end"], bad["headers"], ok)
            assert int(gp.status.cpu()[0]) == BAD_INPUT, what
            assert gp.totals.cpu().tolist() == [0, 0, 0, 0]
        gp = log.plan(whole_img, 0, n, 0, gw.block_first, gw.block_end, gw.headers, ok)
        assert gp.totals.cpu().tolist() == [nr, ne, p.side_bytes, n]
        # emit: each cap one short, then exact
        for short in ("records", "events", "side", None):
            caps = {"records": nr, "events": ne, "side": p.side_bytes}
            if short:
                if caps[short] == 0:
                    continue
                caps[short] -= 1
            rw, rv = guarded(torch, 2 * nr, torch.int64)
            lw, lv = guarded(torch, nr, torch.int64)
            ew, ev = guarded(torch, 4 * ne, torch.int64)
            rc = lib().lsbm_log_read_emit_dev(_ptr(whole_img), whole_img.numel(), 0, n, 0, nb, nh, side_at, caps["side"],
                                              _ptr(rv), caps["records"], _ptr(lv), _ptr(ev), caps["events"], _ptr(st),
                                              _ptr(gp.scratch), gp.scratch.numel() * 8, None)
            assert rc == 0
            if short:
                assert int(st.cpu()[0]) == NO_ROOM, short
                assert all(bool((t == FILL).all()) for t in (rw, lw, ew)) and tobytes(whole_img) == before, short
            else:
                assert int(st.cpu()[0]) == 0
                assert rv.cpu().numpy().reshape(-1, 2).tolist() == e.records.tolist()
                assert lv.cpu().tolist() == e.last_record_offset.tolist()
                assert ev.cpu().numpy().reshape(-1, 4).tolist() == e.events.tolist()
                for whole, used in ((rw, 16 * nr), (lw, 8 * nr), (ew, 32 * ne)):
                    assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + used:] == FILL).all())
                after = tobytes(whole_img)
                assert after[:side_at] == before[:side_at] and after[side_at + p.side_bytes:] == before[side_at + p.side_bytes:]
                assert after[side_at:side_at + p.side_bytes] == e.side.tobytes()
        # a side area that shares a byte with the log
        with pytest.raises(LsbmError) as err:
            log.emit(whole_img, 0, n, 0, gp, n - 1, 8, nr, ne)
        assert err.value.code == LSBM_ERR_INVALID


def test_log_and_side_area_past_4gib(torch_cuda, oracle):
    """A two-block log with one fragmented record at log_at past 4 GiB, the side
    area past 4 GiB too, and 2^32 below both a decoy log of the same layout
    with another payload: the records are the real log's."""
    torch = torch_cuda
    from lsbm_amd import log
    from high_offsets import LINE
    from test_high_offsets import Arena, Guarded
    frame = [["p", 1, 40], ["p", 2, B - 7 - 47], ["p", 4, 300], ["p", 1, 9]]
    real = model.frame_image(frame, [], printable_bytes(0xA1, 2 * B), oracle.value)
    decoy = model.frame_image(frame, [], printable_bytes(0xB2, 2 * B), oracle.value)
    assert real.size == decoy.size and real.tobytes() != decoy.tobytes()
    log_at, side_at = LINE + 5 * 4096 + 3, LINE + (1 << 20) + 4096 + 5
    arena = Arena(torch)
    try:
        out = Guarded(arena)
        w, p, e = model.read(real, ok_by(oracle), 0, log_at=log_at, side_at=side_at)
        assert len(p.records) == 3 and p.side_bytes == B - 7 - 47 + 300
        out.window(side_at, p.side_bytes)
        out.prefill()
        arena.put(log_at, real.tobytes())
        arena.put(log_at - LINE, decoy.tobytes())
        image = arena.image()
        n = real.size
        ok_of = lambda h: log.verify_records(image[log_at:log_at + n], h)[0]  # noqa: E731
        nh, gw, gp, totals, ge = run_steps(torch, image, log_at, n, 0, ok_of, side_at, p.side_bytes)
        assert [int(x.cpu()[0]) for x in (gw.status, gp.status, ge.status)] == [0, 0, 0]
        assert gw.headers.cpu().tolist() == w.headers.tolist()
        assert ge.records.cpu().numpy().reshape(-1, 2).tolist() == e.records.tolist()
        assert ge.last_record_offset.cpu().tolist() == e.last_record_offset.tolist() and ge.events.numel() == 0
        out.verify([(side_at, e.side.tobytes())], "side area")
        assert arena.get(log_at, n) == real.tobytes() and arena.get(log_at - LINE, n) == decoy.tobytes()
        recs = ge.records.cpu().numpy().reshape(-1, 2).tolist()
        assert [arena.get(o, k) for o, k in recs] == model.record_bytes(real, p)
    finally:
        arena.t = None
        torch.cuda.empty_cache()
