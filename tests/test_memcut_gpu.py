"""The memtable switch on the GPU (include/lsbm_memtable_cut.h,
lsbm_amd/memtable.py heights / cut / recover_all, lsbm_amd/write.py
write_logs), exact against the reference's recorded accounting
(tests/golden/memcut_fixture.*) and the model (tests/golden/memcutmodel.py).
"""
import random

import numpy as np
import pytest

from golden import memcut_cases as cases
from golden import memcutmodel as mm
from test_memcut import FIXTURE, SCENARIOS, joined, random_history

pytestmark = pytest.mark.gpu

CANARY = -0x5A5A5A5A5A5A5A5B
MODES = ((mm.RECOVER, "recover"), (mm.WRITE, "write"))


def i64(torch, a):
    return torch.tensor(list(a), dtype=torch.int64, device="cuda")


def dev_entries(torch, entries, base, status=None, key_extra=0, key_at=0, with_types=False):
    """cut()'s inputs for entries [(ikl, vl, type)]."""
    koff = np.concatenate([[0], np.cumsum([ikl - key_extra for ikl, _, _ in entries], dtype=np.int64)]) + key_at
    values = np.array([[7, vl] for _, vl, _ in entries], dtype=np.int64).reshape(-1)
    types = torch.tensor([t for _, _, t in entries], dtype=torch.uint8, device="cuda") if with_types else None
    st = None if status is None else torch.tensor(list(status), dtype=torch.int32, device="cuda")
    return dict(key_offsets=torch.from_numpy(koff.astype(np.int64)).cuda(), values=torch.from_numpy(values).cuda(),
                entry_base=i64(torch, base), key_extra=key_extra, types=types, rec_status=st)


def run_cut(torch, mt, entries, base, status, mode, wbs, state=None, mem_cap=None, **kw):
    d = dev_entries(torch, entries, base, status, **kw)
    r = mt.cut(mode=mode, write_buffer_size=wbs, state=None if state is None else i64(torch, state), mem_cap=mem_cap,
               **d)
    st = int(r.status.cpu()[0])
    if st != mm.OK:
        return dict(status=st)
    n_mem, cont = r.counts.cpu().tolist()
    return dict(status=st, usage=r.usage.cpu().tolist(), mem_first=r.mem_first[:n_mem + 1].cpu().tolist(),
                mem_usage=r.mem_usage[:n_mem].cpu().tolist(), counts=[n_mem, cont], state=r.state.cpu().tolist())


@pytest.fixture(scope="module")
def mt(torch_cuda):
    from lsbm_amd import memtable
    return memtable


def test_heights_match_the_reference_and_the_model(torch_cuda, mt):
    for name, run in FIXTURE["heights"].items():
        h, rnd = mt.heights(len(run["heights"]), run["rnd"])
        assert h.cpu().tolist() == run["heights"], name
        assert int(rnd.cpu()[0]) == run["rnd_after"], name
    for n in (0, 1, 255, 256, 257, 12000, 40000):  # 40,000 inserts: four workgroups of 16,384 draws
        h, rnd = mt.heights(n)
        want, want_rnd = mm.heights(mm.SEED, n)
        assert h.cpu().tolist() == want, n
        assert int(rnd.cpu()[0]) == want_rnd, n
    for rnd_in in (1, mm.M - 1, 123456789):
        h, rnd = mt.heights(300, rnd_in)
        assert (h.cpu().tolist(), int(rnd.cpu()[0])) == mm.heights(rnd_in, 300)


def test_heights_refuse_a_state_no_generator_has(torch_cuda, mt):
    from lsbm_amd._lib import LsbmError
    for rnd in (0, mm.M, 1 << 40):
        with pytest.raises(LsbmError):
            mt.heights(4, rnd)


@pytest.mark.parametrize("name", SCENARIOS)
def test_cut_equals_the_reference(torch_cuda, mt, name):
    s = FIXTURE["scenarios"][name]
    entries, base = cases.entries_of(s["ops"])
    for w in cases.WRITE_BUFFER_SIZES:
        for mode, key in MODES:
            got = run_cut(torch_cuda, mt, entries, base, s["status"], mode, w)
            rec = s["cuts"][f"{key}_{w}"]
            assert got["status"] == mm.OK
            assert got["usage"] == rec["usage"], (name, key, w)
            assert got["mem_first"] == rec["mem_first"] + [len(s["ops"])], (name, key, w)
            assert got["mem_usage"] == rec["ended"], (name, key, w)
            assert got["state"][0] == rec["open_at_end"]
            assert got == mm.cut(entries, base, s["status"], mode, w), (name, key, w)  # the state too


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_sizes_around_a_step(torch_cuda, mt, n):
    """n entries in one record, n one-entry records and n empty records: the
    walk takes 64 slots a step, a workgroup of the other kernels 256 lanes."""
    rng = random.Random(n)
    entries = [(8 + rng.randrange(41), rng.choice((0, 100, 100, 1100)), 1) for _ in range(n)]
    for base in ([0, n], list(range(n + 1)), [0] * (n + 1), [0]):
        e = entries if base[-1] == n else []
        for mode, _ in MODES:
            for w in (4104, 65536):
                assert run_cut(torch_cuda, mt, e, base, None, mode, w) == mm.cut(e, base, None, mode, w), (base[:3], w)


def test_boundaries_on_the_first_and_the_last_lane(torch_cuda, mt):
    """Random histories cut at 4,104 and 8,192: a new memtable begins on the
    first and on the last lane of a 64-slot step; then a history whose arena
    events do."""
    seen = set()
    for seed in range(4):
        rng = random.Random(900 + seed)
        entries, base, status = random_history(rng, 300)
        for mode, _ in MODES:
            for w in (4104, 8192, 65536):
                want = mm.cut(entries, base, status, mode, w)
                got = run_cut(torch_cuda, mt, entries, base, status, mode, w, with_types=True)
                assert got == want, (seed, mode, w)
                for r in want["mem_first"][:-1]:  # the slot that created the memtable
                    seen.add((base[r] + r) % 64)
    assert {0, 63} <= seen
    # arena events (an entry that takes a new block) on the first and on the last lane: one memtable, one entry a record
    rng = random.Random(77)
    entries = [(8 + rng.randrange(41), rng.choice((100, 100, 900, 1100)), 1) for _ in range(3000)]
    base = list(range(3001))
    arena, rnd, lanes = mm.Arena(), mm.SEED, set()
    arena.allocate_aligned(104)
    for k, (ikl, vl, _) in enumerate(entries):
        before = arena.n_blocks
        arena.allocate(mm.entry_size(ikl, vl))
        h, rnd = mm.random_height(rnd)
        arena.allocate_aligned(8 + 8 * h)
        if arena.n_blocks != before:
            lanes.add(2 * k % 64)  # RECOVER: entry k is slot 2k
    assert {0, 62} <= lanes  # (entries sit on even lanes here; the WRITE layout below puts them on odd ones)
    assert run_cut(torch_cuda, mt, entries, base, None, mm.RECOVER, 4 << 20) == \
        mm.cut(entries, base, None, mm.RECOVER, 4 << 20)
    lanes = {(lane + 1) % 64 for lane in lanes}  # WRITE: entry k is slot 2k + 1
    assert {1, 63} <= lanes
    assert run_cut(torch_cuda, mt, entries, base, None, mm.WRITE, 4 << 20) == \
        mm.cut(entries, base, None, mm.WRITE, 4 << 20)


def test_chunks_of_the_walk(torch_cuda, mt):
    """The walk stages 4,096 slots at a time: 9,000 one-entry records are five
    chunks.  A memtable that enters a chunk takes its heights from where the
    chunk before left it, whether it began in this call (at 64 KiB, every few
    hundred entries), never ends (4 MiB) or came in through the state."""
    rng = random.Random(4096)
    entries = [(8 + rng.randrange(41), rng.choice((0, 100, 100, 100, 1100)), 1) for _ in range(9000)]
    base = list(range(9001))
    state = mm.cut(entries[:700], base[:701], None, mm.WRITE, 4 << 20)["state"]
    for mode, _ in MODES:
        for w in (65536, 4 << 20):
            assert run_cut(torch_cuda, mt, entries, base, None, mode, w) == mm.cut(entries, base, None, mode, w)
        got = run_cut(torch_cuda, mt, entries, base, None, mode, 4 << 20, state=state)
        assert got == mm.cut(entries, base, None, mode, 4 << 20, state) and got["counts"] == [1, 1]
    # 4,096 and 4,097 slots exactly, in records of three entries
    for n_slots in (4096, 4097, 8192):
        nr = n_slots // 4
        e, b = entries[:n_slots - nr], [min(3 * i, n_slots - nr) for i in range(nr)] + [n_slots - nr]
        assert run_cut(torch_cuda, mt, e, b, None, mm.RECOVER, 65536) == mm.cut(e, b, None, mm.RECOVER, 65536)


def test_one_lane_walk_equals_the_wave_walk(torch_cuda, mt, monkeypatch):
    """LSBM_MEMCUT_WALK=lane chooses the walk by one lane (the form the wave's
    arrangement was measured against): every scenario, the chunks and a state."""
    monkeypatch.setenv("LSBM_MEMCUT_WALK", "lane")
    for name in SCENARIOS:
        s = FIXTURE["scenarios"][name]
        entries, base = cases.entries_of(s["ops"])
        for w in (4104, 65536, 65600, 4 << 20):
            for mode, key in MODES:
                got = run_cut(torch_cuda, mt, entries, base, s["status"], mode, w)
                assert got == mm.cut(entries, base, s["status"], mode, w), (name, key, w)
                assert got["usage"] == s["cuts"][f"{key}_{w}"]["usage"]
    rng = random.Random(4096)
    entries = [(8 + rng.randrange(41), rng.choice((0, 100, 100, 100, 1100)), 1) for _ in range(9000)]
    base = list(range(9001))
    state = mm.cut(entries[:700], base[:701], None, mm.WRITE, 4 << 20)["state"]
    for mode, _ in MODES:
        assert run_cut(torch_cuda, mt, entries, base, None, mode, 65536) == mm.cut(entries, base, None, mode, 65536)
        assert run_cut(torch_cuda, mt, entries, base, None, mode, 4 << 20, state=state) == \
            mm.cut(entries, base, None, mode, 4 << 20, state)
    e, b, st = random_history(random.Random(5), 200)
    for mode, _ in MODES:
        assert run_cut(torch_cuda, mt, e, b, st, mode, 8192, with_types=True) == mm.cut(e, b, st, mode, 8192)
        assert run_cut(torch_cuda, mt, e, b, st, mode, 4104, mem_cap=1)["status"] == mm.NO_ROOM


def test_two_calls_through_the_state_equal_one(torch_cuda, mt):
    rng = random.Random(101)
    entries, base, status = random_history(rng, 24)
    n = len(base) - 1
    for w in (4104, 8192):
        for mode, _ in MODES:
            one = run_cut(torch_cuda, mt, entries, base, status, mode, w, with_types=True)
            assert one == mm.cut(entries, base, status, mode, w)
            for at in range(n + 1):
                a = run_cut(torch_cuda, mt, entries[:base[at]], base[:at + 1], status[:at], mode, w, with_types=True)
                b = run_cut(torch_cuda, mt, entries[base[at]:], [x - base[at] for x in base[at:]], status[at:], mode,
                            w, state=a["state"], with_types=True)
                assert joined(a, b, at) == (one["usage"], one["mem_first"][:-1], one["mem_usage"], one["state"]), at


def test_state_with_the_height_12_generator(torch_cuda, mt):
    """A memtable whose generator stands 50 draws before the first height 12."""
    run = FIXTURE["heights"]["height_12"]
    state = [1, 4096 - 104, 1, 4096, run["rnd"], 1000]
    entries = [(24, 100, 1)] * 200
    base = list(range(0, 201, 8))
    for mode, _ in MODES:
        got = run_cut(torch_cuda, mt, entries, base, None, mode, 4 << 20, state=state)
        assert got == mm.cut(entries, base, None, mode, 4 << 20, state)
        assert got["state"][4] == run["rnd_after"] and got["state"][5] == 1200 and got["counts"] == [1, 1]


def test_key_offsets_past_4_gib(torch_cuda, mt):
    s = FIXTURE["scenarios"]["deletions"]
    entries, base = cases.entries_of(s["ops"])
    for extra, types in ((0, False), (8, True)):
        got = run_cut(torch_cuda, mt, entries, base, s["status"], mm.RECOVER, 8192, key_extra=extra,
                      key_at=(1 << 32) + 5, with_types=types)
        assert got == mm.cut(entries, base, s["status"], mm.RECOVER, 8192)


def test_errors_change_no_output(torch_cuda, mt):
    torch = torch_cuda
    from lsbm_amd._lib import LsbmError
    entries, base = [(24, 100, 1)] * 300, list(range(0, 301, 3))
    n, nr = len(entries), len(base) - 1
    n_mem = mm.cut(entries, base, None, mm.RECOVER, 8192)["counts"][0]
    assert n_mem > 3

    def run(want, mode=mm.RECOVER, wbs=8192, mem_cap=n_mem, state=None, **change):
        d = dev_entries(torch, entries, base, [0] * nr, with_types=True)
        for k, f in change.items():
            f(d[k])
        outs = dict(usage=torch.full((nr,), CANARY, dtype=torch.int64, device="cuda"),
                    mem_first=torch.full((mem_cap + 1,), CANARY, dtype=torch.int64, device="cuda"),
                    mem_usage=torch.full((max(mem_cap, 1),), CANARY, dtype=torch.int64, device="cuda")[:mem_cap],
                    counts=torch.full((2,), CANARY, dtype=torch.int64, device="cuda"),
                    state_out=torch.full((6,), CANARY, dtype=torch.int64, device="cuda"))
        r = mt.cut(mode=mode, write_buffer_size=wbs, state=None if state is None else i64(torch, state),
                   mem_cap=mem_cap, **d, **outs)
        assert int(r.status.cpu()[0]) == want
        untouched = all(bool((t == CANARY).all()) for t in outs.values())
        assert untouched == (want != mm.OK)

    def put(i, v):
        def f(t):
            t[i] = v
        return f

    run(mm.OK)
    run(mm.NO_ROOM, mem_cap=n_mem - 1)
    run(mm.NO_ROOM, mode=mm.WRITE, mem_cap=1)
    run(mm.BAD_INPUT, wbs=4103)
    run(mm.BAD_INPUT, key_offsets=put(17, 1 << 40))       # then the offsets decrease
    run(mm.BAD_INPUT, key_offsets=put(n, 1 << 33))        # a key of 2^32 bytes or more
    run(mm.BAD_INPUT, values=put(2 * 299 + 1, 1 << 32))   # a value of 2^32 bytes
    run(mm.BAD_INPUT, values=put(1, -1))
    run(mm.BAD_INPUT, types=put(n - 1, 2))
    run(mm.BAD_INPUT, entry_base=put(0, 1))
    run(mm.BAD_INPUT, entry_base=put(nr, n - 1))
    run(mm.BAD_INPUT, entry_base=put(5, 3))
    for st in ([1, 4104, 1, 4096, mm.SEED, 0], [1, 12, 1, 4096, mm.SEED, 0], [1, 8, 0, 0, mm.SEED, 0],
               [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, mm.M, 0], [2, 0, 1, 4096, mm.SEED, 0]):
        run(mm.BAD_INPUT, state=st)
    # aliasing is refused before anything is enqueued
    d = dev_entries(torch, entries, base)
    with pytest.raises(LsbmError):
        mt.cut(mode=mm.RECOVER, write_buffer_size=8192, usage=d["entry_base"][:nr], **d)
    both = torch.zeros(nr + 6, dtype=torch.int64, device="cuda")
    with pytest.raises(LsbmError):
        mt.cut(mode=mm.RECOVER, write_buffer_size=8192, usage=both[:nr], state_out=both[nr - 1:nr + 5], **d)
    with pytest.raises(LsbmError):
        mt.cut(mode=2, write_buffer_size=8192, **d)


# ---- recover_all and write_logs ----

def log_of(torch, reps):
    """A sealed log image of the records, framed on the device."""
    from lsbm_amd import write
    image = torch.from_numpy(np.frombuffer(b"".join(reps) or b"\0", dtype=np.uint8).copy()).cuda()
    at = np.concatenate([[0], np.cumsum([len(r) for r in reps])])
    records = torch.from_numpy(np.stack([at[:-1], np.diff(at)], 1).astype(np.int64).reshape(-1).copy()).cuda()
    return write.frame_records(image, records).log


def tobytes(t):
    return t.cpu().numpy().tobytes()


def flush_of(torch, mt, log, lo, hi, **kw):
    from lsbm_amd import log as lg
    r = lg.read_records(log)
    return mt.flush(r.image, r.records[lo:hi].reshape(-1).contiguous(), **kw)


@pytest.mark.parametrize("name", ["five_memtables", "too_small", "records_in_error", "cut_on_last"])
def test_recover_all_cuts_where_the_reference_does(torch_cuda, mt, name):
    torch = torch_cuda
    reps = dict(cases.scenarios())[name]
    s = FIXTURE["scenarios"][name]
    log = log_of(torch, reps)
    got = mt.recover_all(log, write_buffer_size=65536, bits_per_key=10)
    rec = s["cuts"]["recover_65536"]
    assert got.mem_first == rec["mem_first"] + [len(reps)] and got.status is None
    bounds = list(zip(got.mem_first[:-1], got.mem_first[1:]))
    tables = [flush_of(torch, mt, log, lo, hi, bits_per_key=10) for lo, hi in bounds]
    tables = [t for t in tables if t.image is not None]
    assert len(got.flushes) == len(tables)
    for f, t in zip(got.flushes, tables):
        assert tobytes(f.image) == tobytes(t.image)
        assert (f.smallest, f.largest, f.max_sequence) == (t.smallest, t.largest, t.max_sequence)
    # the option is clipped to 64 KiB as SanitizeOptions clips it
    assert mt.recover_all(log, write_buffer_size=4104).mem_first == got.mem_first


def test_recover_all_of_a_small_log_equals_recover(torch_cuda, mt):
    torch = torch_cuda
    reps = dict(cases.scenarios())["records_in_error"]
    log = log_of(torch, reps)
    one = mt.recover(log)
    got = mt.recover_all(log, write_buffer_size=1 << 30)
    assert got.mem_first == [0, len(reps)] and len(got.flushes) == 1
    assert tobytes(got.flushes[0].image) == tobytes(one.flush.image)
    assert got.flushes[0].max_sequence == one.flush.max_sequence


def test_recover_all_paranoid_keeps_the_finished_tables_only(torch_cuda, mt):
    torch = torch_cuda
    name = "records_in_error"
    reps = dict(cases.scenarios())[name]
    s = FIXTURE["scenarios"][name]
    bad = [i for i, st in enumerate(s["status"]) if st != 0][0]
    log = log_of(torch, reps)
    loose = mt.recover_all(log, write_buffer_size=65536)
    got = mt.recover_all(log, write_buffer_size=65536, paranoid=True)
    assert got.status == "Corruption: " + mt.STATUS_MESSAGE[s["status"][bad]]
    done = [m for m in range(len(loose.mem_first) - 1) if loose.mem_first[m + 1] <= bad]
    assert 1 <= len(got.flushes) == len(done) < len(loose.flushes)
    for f, t in zip(got.flushes, loose.flushes):
        assert tobytes(f.image) == tobytes(t.image)
    # a corrupt physical record: the reader's report ends the loop the same way
    torn = log.clone()
    torn[40000] ^= 0xFF
    got = mt.recover_all(torn, write_buffer_size=65536, paranoid=True)
    assert got.status.startswith("Corruption: ") and got.events.shape[0] >= 1
    kept = int(got.events[0][0])
    want = [m for m in range(len(loose.mem_first) - 1) if loose.mem_first[m + 1] <= kept]
    assert len(got.flushes) == len(want)


def writers_of(name, sync=False):
    """One writer per record of a scenario: [(ops, sync)] with real keys and values."""
    ops = FIXTURE["scenarios"][name]["ops"]
    out, i = [], 0
    for rec in ops:
        w = []
        for kl, vl, t in rec:
            w.append((t, cases.key_of(i, kl), cases.value_of(i, vl) if t else b""))
            i += 1
        out.append((w, sync))
    return out


def check_segments(torch, got, want_first, log_offset):
    """Every log of a write_logs result: its groups, where it starts, and its
    bytes read back as exactly its records."""
    from lsbm_amd import log as lg
    reps = tobytes(got.reps)
    records = got.records.reshape(-1, 2).cpu().tolist()
    assert [s.first_group for s in got.logs] == want_first[:-1]
    assert [s.n_groups for s in got.logs] == [b - a for a, b in zip(want_first[:-1], want_first[1:])]
    for m, seg in enumerate(got.logs):
        start = log_offset if m == 0 and got.first_log_continues else 0  # every later log is a new file
        assert seg.end_offset == start + seg.log.numel()
        assert seg.records.reshape(-1, 2).cpu().tolist() == records[seg.first_group:seg.first_group + seg.n_groups]
        if start % 32768:
            continue  # (a log that continues mid-block is read back joined to its first part by the caller)
        r = lg.read_records(seg.log)
        assert r.events.shape[0] == 0
        payloads = [tobytes(r.image[o:o + n]) for o, n in r.records.cpu().tolist()]
        assert payloads == [reps[o:o + n] for o, n in records[seg.first_group:seg.first_group + seg.n_groups]]


@pytest.mark.parametrize("wbs,n_logs", [(4 << 20, 3), (65536, 20)])
def test_write_logs_switches_where_the_reference_does(torch_cuda, mt, wbs, n_logs):
    """Twenty batches BuildBatchGroup cannot merge, so every writer is a group
    and a record of the fixture: one call switches logs where the reference's
    MakeRoomForWrite does, and two calls split in the middle continue as one."""
    torch = torch_cuda
    from lsbm_amd import write
    from test_write_gpu import dev_ops
    name = "big_batches"
    writers = writers_of(name)
    rec = FIXTURE["scenarios"][name]["cuts"][f"write_{wbs}"]
    d, sync = dev_ops(torch, writers)
    whole = write.write_batches(sync=sync, last_sequence=7, log_offset=0, **d)
    got = write.write_logs(sync=sync, last_sequence=7, write_buffer_size=wbs, **d)
    assert got.group_first.cpu().tolist() == list(range(len(writers) + 1)) == whole.group_first.cpu().tolist()
    assert got.mem_first == rec["mem_first"] + [len(writers)] and len(got.logs) == n_logs >= 3
    assert got.usage.cpu().tolist() == rec["usage"] and int(got.mem_state.cpu()[0]) == rec["open_at_end"]
    assert got.first_log_continues
    assert tobytes(got.records) == tobytes(whole.records) and tobytes(got.reps) == tobytes(whole.reps)
    assert b"".join(tobytes(s.records) for s in got.logs) == tobytes(whole.records)
    assert got.last_sequence == whole.last_sequence
    assert got.sequences.cpu().tolist() == whole.sequences.cpu().tolist()
    check_segments(torch, got, got.mem_first, 0)
    # the first log's bytes are write_batches' up to the first switch
    assert tobytes(got.logs[0].log) == tobytes(whole.log)[:got.logs[0].log.numel()]
    # two calls, split inside a log (and, at 64 KiB, between two): the second continues as one call would
    for half in (3, 11):
        da, sa = dev_ops(torch, writers[:half])
        db, sb = dev_ops(torch, writers[half:])
        a = write.write_logs(sync=sa, last_sequence=7, write_buffer_size=wbs, **da)
        b = write.write_logs(sync=sb, last_sequence=a.last_sequence, write_buffer_size=wbs, mem_state=a.mem_state,
                             log_offset=a.logs[-1].end_offset, **db)
        switch_at_half = half in rec["mem_first"]
        assert b.first_log_continues == (not switch_at_half)
        check_segments(torch, a, a.mem_first, 0)
        check_segments(torch, b, b.mem_first, a.logs[-1].end_offset)
        logs = [tobytes(s.log) for s in a.logs]
        if b.first_log_continues:
            logs[-1] += tobytes(b.logs[0].log)
        logs += [tobytes(s.log) for s in b.logs[0 if switch_at_half else 1:]]
        assert logs == [tobytes(s.log) for s in got.logs]
        assert b.mem_state.cpu().tolist() == got.mem_state.cpu().tolist() and b.last_sequence == got.last_sequence
        assert a.usage.cpu().tolist() + b.usage.cpu().tolist() == rec["usage"]


def test_write_logs_continues_through_the_state(torch_cuda, mt):
    """One writer a call, the state and the log offset handed on: the calls
    that begin a new log are the fixture's WRITE cuts, and the logs are those
    of one call per log."""
    torch = torch_cuda
    from lsbm_amd import write
    from test_write_gpu import dev_ops
    name = "five_memtables"
    writers = writers_of(name, sync=True)
    state, offset, last, switches, logs, usage = None, 0, 0, [], [], []
    for i, w in enumerate(writers):
        d, sync = dev_ops(torch, [w])
        r = write.write_logs(sync=sync, last_sequence=last, write_buffer_size=65536, mem_state=state,
                             log_offset=offset, **d)
        assert len(r.logs) == 1
        if r.first_log_continues and logs:
            logs[-1] += tobytes(r.logs[0].log)
        else:
            switches.append(i)
            logs.append(tobytes(r.logs[0].log))
        state, offset, last = r.mem_state, r.logs[0].end_offset, r.last_sequence
        usage += r.usage.cpu().tolist()
    rec = FIXTURE["scenarios"][name]["cuts"]["write_65536"]
    assert switches == rec["mem_first"] and len(switches) >= 5
    assert usage == rec["usage"]
    # every log reads back as the records of its calls
    from lsbm_amd import log as lg
    for k, blob in enumerate(logs):
        image = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        r = lg.read_records(image)
        assert r.events.shape[0] == 0 and r.records.shape[0] == (switches + [len(writers)])[k + 1] - switches[k]
