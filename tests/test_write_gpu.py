"""Batched DB::Write on the GPU (include/lsbm_write.h, lsbm_amd/write.py), exact
against the reference's fixture (tests/golden/write_fixture.json, whose group
cuts are DBImpl::BuildBatchGroup's own) and the plain-Python model
(tests/golden/writemodel.py), with guard bytes around every output.
"""
import numpy as np
import pytest

from golden import write_cases as wc
from golden import writemodel as wm

pytestmark = pytest.mark.gpu

B, P = wc.B, wc.P
GUARD = 0xA5


@pytest.fixture(scope="module")
def fixture():
    return wc.load()


def masked_crc(oracle):
    return lambda data: oracle.mask(oracle.value(data))


def dev_ops(torch, writers, key_lead=0, value_lead=0):
    """Device tensors of [(ops, sync)]: keys and values back to back (so their
    sources fall on every phase), after key_lead / value_lead spare bytes."""
    types, keys, koff, vimg, values, bf, sync = [], bytearray(key_lead), [key_lead], bytearray(value_lead), [], [0], []
    for ops, s in writers:
        for t, k, v in ops:
            types.append(t)
            keys += k
            koff.append(len(keys))
            values += [len(vimg), len(v)] if t else [0, 0]
            vimg += v
        bf.append(len(types))
        sync.append(1 if s else 0)
    u8 = lambda b: torch.from_numpy(np.frombuffer(bytes(b) or b"\0", dtype=np.uint8).copy()).cuda()[:len(b)]  # noqa: E731
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device="cuda")  # noqa: E731
    return dict(types=u8(bytes(types)), keys=u8(keys), key_offsets=i64(koff), value_image=u8(vimg),
                values=i64(values), batch_first=i64(bf)), u8(bytes(sync))


def guarded(torch, n, dtype, lead=64):
    """(whole, window): n elements with `lead` guard elements before and 64 after."""
    fill = GUARD if dtype == torch.uint8 else -0x5A5A5A5A
    whole = torch.full((lead + n + 64,), fill, dtype=dtype, device="cuda")
    return whole, whole[lead:lead + n]


def guards_intact(whole, lead, n):
    fill = whole[0].item()
    return bool((whole[:lead] == fill).all()) and bool((whole[lead + n:] == fill).all())


def tobytes(t):
    return t.cpu().numpy().tobytes()


def check_result(torch, r, reps, group_first, group_sync, seqs, counts, last, log_offset, oracle):
    from lsbm_amd import log
    log_bytes, heads, _, end = wm.add_records(reps, log_offset, masked_crc(oracle))
    assert r.group_first.tolist() == group_first
    assert r.group_sync.tolist() == [1 if s else 0 for s in group_sync]
    assert [x & ((1 << 64) - 1) for x in r.sequences.tolist()] == seqs and r.counts.tolist() == counts
    assert r.last_sequence == last and r.end_offset == end
    assert tobytes(r.reps) == b"".join(reps)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in reps])]).astype(np.int64)
    assert r.records.tolist() == [x for i, rep in enumerate(reps) for x in (int(offs[i]), len(rep))]
    assert r.headers.tolist() == heads
    assert tobytes(r.log) == log_bytes
    if heads:
        ok, nbad = log.verify_records(r.log, r.headers)
        assert int(nbad.cpu()[0]) == 0 and bool(ok.all())
    return log_bytes


@pytest.mark.parametrize("name", [n for n, _, _ in wc.write_specs()])
def test_write_batches_equals_the_reference(torch_cuda, fixture, oracle, name):
    """The whole chain against BuildBatchGroup's own cuts, the reference's reps
    and its log file; then the round trips through the log reader and the
    memtable."""
    torch = torch_cuda
    from lsbm_amd import memtable, write
    c = [c for c in fixture[0] if c["name"] == name][0]
    writers = wc.writers_of(c["writers"])
    ops, sync = dev_ops(torch, writers)
    r = write.write_batches(sync=sync, last_sequence=c["last_sequence"], **ops)
    seqs, counts, at = [], [], c["last_sequence"] + 1
    for rep in c["reps"]:
        n = int.from_bytes(rep[8:12], "little")
        seqs.append(at)
        counts.append(n)
        at += n
    log_bytes = check_result(torch, r, c["reps"], c["group_first"], [writers[f][1] for f in c["group_first"][:-1]], seqs,
                             counts, c["new_last_sequence"], 0, oracle)
    assert log_bytes == c["log"]
    if not any(s for s, _ in c["writers"]):  # d_sync NULL is all false
        r0 = write.write_batches(sync=None, last_sequence=c["last_sequence"], **ops)
        assert r0.group_first.tolist() == c["group_first"] and tobytes(r0.log) == c["log"]
    if len(c["log"]) < 1 << 20:
        image, records = memtable.log_records(c["log"])
        pairs = records.reshape(-1, 2).tolist()
        back = tobytes(image)
        assert [back[o:o + n] for o, n in pairs] == c["reps"]
        e = memtable.entries(r.reps, r.records)
        ko, kb, vals, src = e.key_offsets.tolist(), tobytes(e.keys), e.values.reshape(-1, 2).tolist(), tobytes(r.reps)
        got = [(kb[ko[i]:ko[i + 1]], src[vals[i][0]:vals[i][0] + vals[i][1]]) for i in range(len(ko) - 1)]
        assert got == wm.memtable_iteration(c["reps"])


def test_two_calls_append_to_one(torch_cuda, fixture, oracle):
    """A second call that starts at the first's end_offset and last_sequence
    appends what one call over all writers writes, cut at a group boundary (the
    rule then makes the same cuts on both sides)."""
    torch = torch_cuda
    from lsbm_amd import write
    for name in ("header_counting", "sync_mixed", "ops_65_257"):
        c = [c for c in fixture[0] if c["name"] == name][0]
        writers = wc.writers_of(c["writers"])
        cut = c["group_first"][1]
        if cut == len(writers):
            cut = 0
        o1, s1 = dev_ops(torch, writers[:cut])
        o2, s2 = dev_ops(torch, writers[cut:])
        r1 = write.write_batches(sync=s1, last_sequence=c["last_sequence"], **o1)
        r2 = write.write_batches(sync=s2, last_sequence=r1.last_sequence, log_offset=r1.end_offset, **o2)
        assert tobytes(r1.log) + tobytes(r2.log) == c["log"], name
        assert r1.group_first.tolist()[:-1] + [cut + f for f in r2.group_first.tolist()] == c["group_first"]
        assert r2.last_sequence == c["new_last_sequence"] and r2.end_offset == len(c["log"])
        assert (r2.headers + r1.end_offset).tolist() == wm.add_records(c["reps"])[1][r1.headers.numel():]


def test_steps_at_every_phase_with_guards(torch_cuda, oracle):
    """sizes, group, build, frame_plan and frame one by one, outputs between
    guard bytes, the rep image and the log window at all 16 destination
    phases and the keys and values at all 16 source phases; a log that starts
    mid-block."""
    torch = torch_cuda
    from lsbm_amd import write
    spec = [s for s in wc.write_specs() if s[0] == "ops_65_257"][0]
    writers = wc.writers_of(spec[2]) + [([(1, wc.pattern(3, 70000), wc.pattern(9, 40000))], False),
                                        ([(0, b"gone", b"")], True), ([], False)]
    reps, gf, gs, seqs, counts, last = wm.write(writers, 77)
    body = b"".join(reps)
    log_offset = 5 * B + 31000
    log_bytes, heads, frags, end = wm.add_records(reps, log_offset)
    for phase in range(16):
        ops, sync = dev_ops(torch, writers, key_lead=phase, value_lead=(5 * phase) % 16)
        n, nw = ops["types"].numel(), len(writers)
        w_os, op_sum = guarded(torch, n + 1, torch.int64)
        w_bs, batch_sum = guarded(torch, nw + 1, torch.int64)
        s = write.sizes(ops["types"], ops["key_offsets"], ops["keys"].numel(), ops["values"],
                        ops["value_image"].numel(), ops["batch_first"], op_sum, batch_sum)
        sizes = [wm.op_bytes(op) for o, _ in writers for op in o]
        assert s.status.item() == write.OK and op_sum.tolist() == [0] + np.cumsum(sizes).tolist()
        assert np.diff(batch_sum.tolist()).tolist() == [wm.batch_of(o).byte_size() for o, _ in writers]
        assert guards_intact(w_os, 64, n + 1) and guards_intact(w_bs, 64, nw + 1)
        w_gf, group_first = guarded(torch, len(gf), torch.int64)
        w_gs, group_sync = guarded(torch, len(gf) - 1, torch.uint8)
        g = write.group(batch_sum=batch_sum, sync=sync, group_first=group_first, group_sync=group_sync)
        assert g.status.item() == write.OK and g.n_groups.item() == len(gf) - 1
        assert group_first.tolist() == gf and group_sync.tolist() == [int(x) for x in gs]
        assert guards_intact(w_gf, 64, len(gf)) and guards_intact(w_gs, 64, len(gf) - 1)
        ng = len(gf) - 1
        w_reps, d_reps = guarded(torch, len(body), torch.uint8, lead=64 + phase)
        w_rec, records = guarded(torch, 2 * ng, torch.int64)
        w_sc, seq_counts = guarded(torch, 2 * ng, torch.int64)
        b = write.build(ops["types"], ops["keys"], ops["key_offsets"], ops["value_image"], ops["values"],
                        ops["batch_first"], op_sum, group_first, ng, 77, d_reps, records, seq_counts)
        assert b.status.item() == write.OK and tobytes(d_reps) == body and b.last_sequence.item() == last
        assert seq_counts.tolist() == [x for pair in zip(seqs, counts) for x in pair]
        assert guards_intact(w_reps, 64 + phase, len(body)) and guards_intact(w_rec, 64, 2 * ng)
        assert guards_intact(w_sc, 64, 2 * ng)
        w_ff, frag_first = guarded(torch, ng + 1, torch.int64)
        w_rs, rec_start = guarded(torch, ng + 1, torch.int64)
        p = write.frame_plan(records, len(body), log_offset, frag_first, rec_start)
        assert p.status.item() == write.OK and frag_first.tolist() == [0] + np.cumsum(frags).tolist()
        assert rec_start[-1].item() == end and guards_intact(w_ff, 64, ng + 1) and guards_intact(w_rs, 64, ng + 1)
        w_out, out = guarded(torch, len(log_bytes), torch.uint8, lead=64 + (7 * phase) % 16)
        w_h, headers = guarded(torch, len(heads), torch.int64)
        f = write.frame(d_reps, records, log_offset, frag_first, rec_start, out, headers)
        assert f.status.item() == write.OK and tobytes(out) == log_bytes and headers.tolist() == heads
        assert guards_intact(w_out, 64 + (7 * phase) % 16, len(log_bytes)) and guards_intact(w_h, 64, len(heads))


def test_group_rule_on_sizes(torch_cuda):
    """write.group on ByteSize arrays against the model of BuildBatchGroup
    (which the fixture pins): the thresholds, the sync patterns, one writer,
    no writer, and 1,025 writers in groups of four so that the chain's staged
    links turn over."""
    torch = torch_cuda
    from lsbm_amd import write
    rng = np.random.default_rng(0x6209)
    K, M = 131072, 1 << 20
    queues = [([K, K, 16], None), ([K, K + 1], None), ([K, K - 12, 12], None), ([K + 1, M - K - 1, 12], None),
              ([K + 1, M - K, 12], None), ([M + 1, 12, 12], None), ([M, 12], None), ([M - 12, 12, 12], None),
              ([12], None), ([12], [1]), ([], None), ([12] * 5, [0, 0, 1, 0, 0]), ([12] * 5, [1, 0, 1, 0, 0]),
              ([12] * 5, [1] * 5), ([12] * 5, [0] * 5), ([1000] + [1311] * 101, None),
              ([40000] * 1025, None), ([40000] * 1025, (rng.random(1025) < 0.2).astype(int).tolist()),
              ([12] * 30000, None)]
    for t in range(30):
        n = int(rng.integers(1, 3000))
        queues.append((rng.choice([12, 16, 500, 40000, K, K + 1, 300000, M, M + 1], n).tolist(),
                       (rng.random(n) < 0.1).astype(int).tolist() if t % 2 else None))
    for sizes, syncs in queues:
        want = wm.groups(sizes, syncs)
        bb = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        sy = None if syncs is None else torch.tensor(syncs, dtype=torch.uint8, device="cuda")
        g = write.group(bb, sy)
        ng = g.n_groups.item()
        assert g.status.item() == write.OK and g.group_first[:ng + 1].tolist() == want, (sizes[:8], len(sizes))
        assert g.group_sync[:ng].tolist() == [int(syncs[f]) if syncs else 0 for f in want[:-1]]
    assert len(wm.groups([40000] * 1025)) == 258


@pytest.mark.parametrize("name", [n for n, _ in wc.log_specs()])
def test_frame_records_equals_the_reference(torch_cuda, fixture, oracle, name):
    """AddRecord over the fixture's payloads, sealed, from file offset 0 and
    from record boundaries as log_offset (every one for the short cases)."""
    torch = torch_cuda
    from lsbm_amd import write
    c = [c for c in fixture[1] if c["name"] == name][0]
    payloads = [wc.pattern(seed, n) for n, seed in c["payloads"]]
    image = torch.from_numpy(np.frombuffer(b"\x55" * 3 + b"".join(payloads) or b"\0", dtype=np.uint8).copy()).cuda()
    offs = 3 + np.concatenate([[0], np.cumsum([len(p) for p in payloads])]).astype(np.int64)
    rec = [x for i, p in enumerate(payloads) for x in (int(offs[i]), len(p))]
    bounds = [wm.add_records(payloads[:i])[3] for i in range(len(payloads) + 1)]
    picks = range(len(payloads) + 1) if len(payloads) <= 24 else \
        sorted({i for i in (0, 1, 2, 17, 63, 64, 65, len(payloads) - 1, len(payloads)) if i <= len(payloads)})
    for i in picks:
        at = bounds[i]
        records = torch.tensor(rec[2 * i:], dtype=torch.int64, device="cuda")
        r = write.frame_records(image, records, log_offset=at)
        assert tobytes(r.log) == c["log"][at:], (name, i)
        assert r.end_offset == len(c["log"])
        assert r.headers.tolist() == wm.add_records(payloads[i:], at)[1]
        raw = write.frame_records(image, records, log_offset=at, seal=False)
        assert tobytes(raw.log) == wm.add_records(payloads[i:], at)[0]


def test_frame_plan_steps_and_events(torch_cuda):
    """frame_plan alone against the model where its 64-record steps can go wrong:
    a record that ends on a block end, or within 6 bytes of it, or with exactly
    7 left, as record 63 of a step, as record 1, in consecutive records, and
    as record 0 (after which one lane takes the next 64); 2,500 records, so
    that the staged lengths turn over with steps cut short by the stage's end."""
    torch = torch_cuda
    import random
    from lsbm_amd import write
    rng = random.Random(0xF7A3)
    short = lambda k: [rng.randrange(1, 40) for _ in range(k)]  # noqa: E731
    queues = []
    for r in (0, 3, 7):
        q = wc._leaving(short(63), r) + short(70)  # the event is record 63 of the first step
        assert len(q) == 64 + 70
        queues.append(q)
        queues.append(wc._leaving(short(1), r) + [P, P, 0, 5] + short(70))  # record 1, then consecutive
        queues.append(wc._leaving([], r) + short(130))  # record 0
        queues.append(wc._leaving(short(63), r) + [0, 0] + short(5))
    mixed = []
    for _ in range(2500):
        mixed.append(rng.choice((0, 7, P - 7, P, P + 1, 2 * P)) if rng.random() < 0.02 else rng.randrange(0, 300))
    queues.append(mixed)
    queues.append([P] * 70 + short(70) + [P] * 3)
    for lens in queues:
        for at in (0, 1000, B - 3):
            _, heads, frags, end = wm.add_records([bytes(n) for n in lens], at)
            firsts = np.concatenate([[0], np.cumsum(frags)]).tolist()
            records = torch.tensor([x for n in lens for x in (0, n)], dtype=torch.int64, device="cuda")
            p = write.frame_plan(records, max(lens), at)
            assert p.status.item() == write.OK
            assert p.frag_first.tolist() == firsts, (len(lens), at)
            assert p.rec_start.tolist() == [at + heads[f] for f in firsts[:-1]] + [end], (len(lens), at)


def test_frame_window_phase_and_padding(torch_cuda):
    """A log that ended 1..6 bytes before a block end gets that many zero bytes
    first; 0 < log_offset % 32768 < 7 is BAD_INPUT with nothing written."""
    torch = torch_cuda
    from lsbm_amd import write
    payloads = [wc.pattern(1, 20), b"", wc.pattern(2, P + 9)]
    image = torch.from_numpy(np.frombuffer(b"".join(payloads), dtype=np.uint8).copy()).cuda()
    records = torch.tensor([0, 20, 20, 0, 20, P + 9], dtype=torch.int64, device="cuda")
    for at in (0, P, B - 6, B - 1, B, B + 7, 3 * B - 3, 2 * B + 1234, (1 << 33) + B - 7):
        want, heads, frags, end = wm.add_records(payloads, at)
        w_out, out = guarded(torch, len(want), torch.uint8, lead=67)
        w_h, headers = guarded(torch, len(heads), torch.int64)
        p = write.frame_plan(records, image.numel(), at)
        assert p.status.item() == write.OK and p.rec_start[-1].item() == end
        f = write.frame(image, records, at, p.frag_first, p.rec_start, out, headers)
        assert f.status.item() == write.OK and tobytes(out) == want and headers.tolist() == heads, at
        assert guards_intact(w_out, 67, len(want)) and guards_intact(w_h, 64, len(heads))
    for at in (3, B + 1, 7 * B + 6):
        ff = torch.full((4,), 7, dtype=torch.int64, device="cuda")
        rs = torch.full((4,), 7, dtype=torch.int64, device="cuda")
        p = write.frame_plan(records, image.numel(), at, ff, rs)
        assert p.status.item() == write.BAD_INPUT and ff.tolist() == [7] * 4 and rs.tolist() == [7] * 4
        good = write.frame_plan(records, image.numel(), 0)
        w_out, out = guarded(torch, 40000, torch.uint8)
        w_h, headers = guarded(torch, 8, torch.int64)
        f = write.frame(image, records, at, good.frag_first, good.rec_start, out, headers)
        assert f.status.item() == write.BAD_INPUT
        assert bool((w_out == GUARD).all()) and bool((w_h == w_h[0]).all())


def test_bad_input_and_no_room_change_nothing(torch_cuda):
    """Each BAD_INPUT of the header and a cap one too small: the status word,
    and every other output as it was."""
    torch = torch_cuda
    from lsbm_amd import write
    from lsbm_amd._lib import LSBM_ERR_INVALID, LsbmError
    writers = [([(1, b"alpha", b"one"), (0, b"beta", b"")], False), ([], False), ([(1, b"gamma", b"three" * 30)], True),
               ([(1, b"d", b"")], False)]
    ops, sync = dev_ops(torch, writers)
    n, nw = 4, 4
    ksz, vsz = ops["keys"].numel(), ops["value_image"].numel()
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device="cuda")  # noqa: E731

    def run_sizes(**change):
        a = dict(ops, keys_size=ksz, value_image_size=vsz)
        a.update(change)
        op_sum, batch_sum = i64([-9] * (n + 1)), i64([-9] * (nw + 1))
        s = write.sizes(a["types"], a["key_offsets"], a["keys_size"], a["values"], a["value_image_size"],
                        a["batch_first"], op_sum, batch_sum)
        return s.status.item(), op_sum.tolist(), batch_sum.tolist()

    st, op_sum, batch_sum = run_sizes()
    assert st == write.OK and op_sum[0] == 0 and batch_sum[-1] == 12 * nw + op_sum[-1]
    koff, vals, bf = ops["key_offsets"].tolist(), ops["values"].tolist(), ops["batch_first"].tolist()
    types = ops["types"].clone()
    types[1] = 2
    bad = [dict(types=types),
           dict(key_offsets=i64([0, 5, 9, 9 + (1 << 32), 10 + (1 << 32)]), keys_size=1 << 33),  # a key of 2^32 bytes
           dict(values=i64(vals[:5] + [1 << 32] + vals[6:]), value_image_size=1 << 33),  # a value of 2^32 bytes
           dict(key_offsets=i64([0, 5, 4, 14, 15])),  # decreasing
           dict(key_offsets=i64(koff[:-1] + [ksz + 1])),  # past the keys
           dict(values=i64(vals[:4] + [vsz - 1, 150] + vals[6:])),  # past the value image
           dict(values=i64(vals[:4] + [vsz + 1, 0] + vals[6:])),
           dict(batch_first=i64([0, 2, 1, 3, 4])), dict(batch_first=i64([1, 2, 2, 3, 4])),
           dict(batch_first=i64([0, 2, 2, 3, 3])), dict(batch_first=i64([0, 2, 2, 3, 5]))]
    for change in bad:
        st, o, b = run_sizes(**change)
        assert st == write.BAD_INPUT and o == [-9] * (n + 1) and b == [-9] * (nw + 1), list(change)
    # a Delete's value slice is not read
    st, o, _ = run_sizes(values=i64(vals[:2] + [1 << 60, 1 << 40] + vals[4:]))
    assert st == write.OK and o == op_sum

    s = write.sizes(ops["types"], ops["key_offsets"], ksz, ops["values"], vsz, ops["batch_first"])
    want = wm.groups([b - a for a, b in zip(batch_sum, batch_sum[1:])], [w[1] for w in writers])
    ng = len(want) - 1
    assert ng >= 2
    gf, gs = i64([-9] * ng), torch.full((ng - 1,), 9, dtype=torch.uint8, device="cuda")
    g = write.group(batch_sum=s.batch_sum, sync=sync, group_first=gf, group_sync=gs)  # cap = n_groups - 1
    assert g.status.item() == write.NO_ROOM and gf.tolist() == [-9] * ng and gs.tolist() == [9] * (ng - 1)
    assert g.n_groups.item() == 0
    for sums in ([0, 20, 31, 60, 80], [0, 20, 19, 60, 80]):  # a ByteSize under 12; sums that decrease
        g = write.group(batch_sum=i64(sums), group_first=i64([-9] * 5))
        assert g.status.item() == write.BAD_INPUT and g.group_first.tolist() == [-9] * 5

    g = write.group(batch_sum=s.batch_sum, sync=sync)
    total = 12 * ng + op_sum[-1]

    def run_build(cap=total, op_sum_t=s.op_sum, gf_t=g.group_first, n_groups=ng, **change):
        a = dict(ops)
        a.update(change)
        w_reps, reps = guarded(torch, cap, torch.uint8)
        records, sc = i64([-9] * (2 * n_groups)), i64([-9] * (2 * n_groups))
        b = write.build(a["types"], a["keys"], a["key_offsets"], a["value_image"], a["values"], a["batch_first"],
                        op_sum_t, gf_t, n_groups, 100, reps, records, sc)
        untouched = bool((w_reps == GUARD).all()) and records.tolist() == [-9] * (2 * n_groups) and \
            sc.tolist() == [-9] * (2 * n_groups) and b.last_sequence.item() == 0
        return b.status.item(), untouched, reps

    st, untouched, reps = run_build()
    assert st == write.OK and not untouched and tobytes(reps) == b"".join(wm.write(writers, 100)[0])
    st, untouched, _ = run_build(cap=total - 1)
    assert st == write.NO_ROOM and untouched
    tampered = s.op_sum.clone()
    tampered[2] += 1
    for kw in (dict(op_sum_t=tampered), dict(gf_t=i64([0, 2, 2, 4][:ng + 1])), dict(gf_t=i64([1] + want[1:])),
               dict(gf_t=i64(want[:-1] + [nw + 1])), dict(types=types), dict(batch_first=i64([0, 2, 1, 3, 4])),
               dict(key_offsets=i64([0, 5, 4, 14, 15]))):
        st, untouched, _ = run_build(**kw)
        assert st == write.BAD_INPUT and untouched, list(kw)

    b = write.build(n_groups=ng, op_sum=s.op_sum, group_first=g.group_first, last_sequence=100, **ops)
    p = write.frame_plan(b.records, b.reps.numel(), 40)
    n_frag, end = p.frag_first[-1].item(), p.rec_start[-1].item()

    def run_frame(out_cap=end - 40, head_cap=n_frag, ff=p.frag_first, rs=p.rec_start, records=b.records):
        w_out, out = guarded(torch, out_cap, torch.uint8)
        w_h, headers = guarded(torch, head_cap, torch.int64)
        f = write.frame(b.reps, records, 40, ff, rs, out, headers)
        return f.status.item(), bool((w_out == GUARD).all()) and bool((w_h == w_h[0]).all())

    assert run_frame() == (write.OK, False)
    assert run_frame(out_cap=end - 41) == (write.NO_ROOM, True)
    assert run_frame(head_cap=n_frag - 1) == (write.NO_ROOM, True)
    rs = p.rec_start.clone()
    rs[1] += 1
    ff = p.frag_first.clone()
    ff[1] += 1
    outside = b.records.clone()
    outside[1] = b.reps.numel() + 1
    assert run_frame(rs=rs) == (write.BAD_INPUT, True) and run_frame(ff=ff) == (write.BAD_INPUT, True)
    assert run_frame(records=outside) == (write.BAD_INPUT, True)
    pl = write.frame_plan(outside, b.reps.numel(), 40, i64([-9] * (ng + 1)), i64([-9] * (ng + 1)))
    assert pl.status.item() == write.BAD_INPUT and pl.frag_first.tolist() == [-9] * (ng + 1)
    # an output that overlaps an input is refused by the host
    with pytest.raises(LsbmError) as e:
        write.frame(b.reps, b.records, 40, p.frag_first, p.rec_start, b.reps, i64([0] * n_frag))
    assert e.value.code == LSBM_ERR_INVALID
    with pytest.raises(LsbmError):
        write.sizes(ops["types"], ops["key_offsets"], ksz, ops["values"], vsz, ops["batch_first"], ops["key_offsets"])
