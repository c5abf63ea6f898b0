"""Batched range scans on the GPU (include/lsbm_iter.h, lsbm_amd/scan.py,
db.Version.view): every kernel and the whole chain, exact against the
reference's fixture (tests/golden/scan_fixture.json, scan_tables.bin) and the
plain-Python model (tests/golden/scanmodel.py, pinned to that fixture by
tests/test_scan.py).
"""
import ctypes
import random
import struct

import numpy as np
import pytest

from golden import blockmodel as bm
from golden import memtablemodel as mt
from golden import scan_cases
from golden import scanmodel as sm
from golden import snappytablemodel as stm
from test_db_get import codec, fx, memtable_of  # noqa: F401 (fx is a fixture)

pytestmark = pytest.mark.gpu

GUARD = 0xEE
ERR_INVALID = -1
OK, NO_ROOM, BAD_INPUT, UNSORTED = 0, 1, 2, 3
KMAX = sm.kMaxSequenceNumber


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(1, dtype=getattr(torch, str(a.dtype)), device="cuda")[:0]
    return torch.from_numpy(a.copy()).to("cuda")


def pack(keys):
    """(uint8 array, int64 offsets) of a list of byte strings."""
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    return np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)[:int(off[-1])], off


def dev_keys(torch, keys):
    b, off = pack(keys)
    return _dev(torch, b), _dev(torch, off)


def dev_entries(torch, entries):
    """(keys, key_offsets, values int64[n, 2], image) of sorted [(internal key, value)]."""
    keys, koff = dev_keys(torch, [k for k, _ in entries])
    image, voff = pack([v for _, v in entries])
    values = np.stack([voff[:-1], voff[1:] - voff[:-1]], 1) if entries else np.zeros((0, 2), dtype=np.int64)
    return keys, koff, _dev(torch, values.astype(np.int64)), _dev(torch, image)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(torch, n, dtype, fill, pad=16):
    """(whole tensor, the n-element view between two guard zones)."""
    whole = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
    return whole, whole[pad:pad + n]


def guards_intact(whole, n, fill, pad=16):
    h = whole.cpu().numpy()
    return bool(np.all(h[:pad] == fill) and np.all(h[pad + n:] == fill))


def bounds(torch, keys):
    """(buffer, offsets, presence) of a list of user keys with None for an absent bound."""
    b, off = dev_keys(torch, [k or b"" for k in keys])
    return b, off, _dev(torch, np.array([k is not None for k in keys], dtype=np.uint8))


def run_scan(torch, view, queries, reverse):
    """[([(user key, value)], status)] of queries [(lo, hi, limit)] through SnapshotView.scan."""
    lo, lo_off, lo_p = bounds(torch, [q[0] for q in queries])
    hi, hi_off, hi_p = bounds(torch, [q[1] for q in queries])
    limits = _dev(torch, np.array([q[2] for q in queries], dtype=np.int64))
    r = view.scan(lo, lo_off, hi, hi_off, limit=limits, reverse=reverse, lo_present=lo_p, hi_present=hi_p)
    first = r.entry_first.cpu().tolist()
    koff, voff = r.key_offsets.cpu().tolist(), r.value_offsets.cpu().tolist()
    kb, vb = r.keys.cpu().numpy().tobytes(), r.values.cpu().numpy().tobytes()
    assert len(koff) == first[-1] + 1 and len(voff) == first[-1] + 1
    assert koff[-1] == len(kb) and voff[-1] == len(vb)
    status = r.status.cpu().tolist()
    return [([(kb[koff[i]:koff[i + 1]], vb[voff[i]:voff[i + 1]]) for i in range(first[q], first[q + 1])], status[q])
            for q in range(len(queries))]


def model_scan(entries, s, queries, reverse):
    return [sm.scan_port(entries, s, lo, hi, limit, reverse)[:2] for lo, hi, limit in queries]


# ---------------------------------------------------------------- plan


def history_of(n, seed, error_keys=True):
    """n sorted entries: few versions to many per user key, deletions, error keys."""
    rng = random.Random(seed)
    entries, u = [], 0
    while len(entries) < n:
        user = b"u%05d" % u
        u += 1
        for _ in range(min(rng.choice([1, 1, 2, 3, 5, 9]), n - len(entries))):
            kind = rng.choice([0, 1, 1, 1])
            if error_keys and rng.random() < 0.1:
                kind = rng.choice([2, 255])
            entries.append((sm.ikey(user, rng.randint(1, 30), kind), b"v%d" % len(entries)))
    return sm.sort_entries(entries)


def tile_edge_history():
    """3 tiles + 1 of 256 positions, laid out position by position:
      0..99     a000..a099, a value each at seq 1
      100..252  one user key `m`, seq 1000 down: nothing a low snapshot sees
      253       m at seq 3
      254       an error key of m (type 2 at seq 2)
      255       n000, a deletion at seq 2: a deletion head at a tile's last position
      256       n000, a value at seq 1: hidden by 255 across the tile edge; an error key follows
      257       n000, type 255 at seq 0
      258..767  one user key `p` with 510 versions, seq 2000 down to 1491 except the last (seq 1): its
                only visible entry at a low snapshot is in the third tile, two tile edges later
      768       q, a value at seq 1
    and error keys at 511 and 512 (p's versions there carry type 2 / 255)."""
    e = [(sm.ikey(b"a%03d" % i, 1), b"a%d" % i) for i in range(100)]
    e += [(sm.ikey(b"m", 1000 - i), b"m-new") for i in range(153)]
    e += [(sm.ikey(b"m", 3), b"m3"), (sm.ikey(b"m", 2, 2), b"m-bad")]
    e += [(sm.ikey(b"n000", 2, 0), b""), (sm.ikey(b"n000", 1), b"n-old"), (sm.ikey(b"n000", 0, 255), b"n-bad")]
    for i in range(510):
        kind = 2 if len(e) == 511 else (255 if len(e) == 512 else 1)
        e.append((sm.ikey(b"p", 2000 - i if i < 509 else 1, kind), b"p%d" % i))
    e.append((sm.ikey(b"q", 1), b"q"))
    assert len(e) == 769 and e == sm.sort_entries(e)
    return e


def check_view(torch, entries, s):
    """scan.view of the entries against the model's view: every array, the counts and the gathered live entries."""
    from lsbm_amd import scan
    keys, koff, values, image = dev_entries(torch, entries)
    v = scan.view(keys, koff, values, image, s)
    want = sm.View(entries, s)
    n, ny = len(entries), want.n_yield
    p = v.plan
    assert p.status.cpu().tolist() == [OK]
    live_keys = [entries[j][0] for j in want.live]
    assert p.counts.cpu().tolist() == [ny, sum(len(k) for k in live_keys), want.corrupt_rank[n]], (n, s)
    assert v.n_yield == ny
    assert p.source[:ny].cpu().tolist() == want.live, (n, s)
    assert p.yield_rank.cpu().tolist() == want.yield_rank, (n, s)
    assert p.corrupt_rank.cpu().tolist() == want.corrupt_rank, (n, s)
    assert p.first[:ny].cpu().tolist() == want.first, (n, s)
    assert p.back[:ny].cpu().tolist() == want.back, (n, s)
    off = v.live_key_offsets.cpu().tolist()
    assert off == [sum(len(k) for k in live_keys[:j]) for j in range(ny + 1)]
    assert v.live_keys.cpu().numpy().tobytes() == b"".join(live_keys)
    vals = v.live_values.cpu().tolist()
    buf = image.cpu().numpy().tobytes()
    assert [buf[o:o + ln] for o, ln in vals] == [entries[j][1] for j in want.live]
    assert v.value_prefix.cpu().tolist() == [sum(len(entries[j][1]) for j in want.live[:i]) for i in range(ny + 1)]
    return v, want


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 769])
def test_plan_equals_model(torch_cuda, n):
    entries = history_of(n, 0x5CA0 + n)
    for s in (0, 7, 15, 30, KMAX):  # snapshot 0: everything hidden
        _, want = check_view(torch_cuda, entries, s)
        assert want.n_yield == 0 if s == 0 else want.n_yield > 0 or n < 255


def test_plan_tile_edges(torch_cuda):
    entries = tile_edge_history()
    for s in (0, 1, 2, 3, 1490, 1747, 2000, KMAX):
        _, want = check_view(torch_cuda, entries, s)
    want = sm.View(entries, 1)
    # at snapshot 1: p's only visible entry is its last version, two tile edges after its seg_start; n000's
    # deletion is not visible yet, at 2 it heads the key from the last position of tile 0
    assert 767 in want.live and want.first[want.live.index(767)] == 258
    assert 256 in want.live and 256 not in sm.View(entries, 2).live
    # a user key's versions crossing positions 255 / 256 with the head before the edge, and the second tile's
    # first visible entry of a key that starts there
    crossing = sm.sort_entries([(sm.ikey(b"k%03d" % (i // 3), 9 - i % 3), b"x%d" % i) for i in range(300)])
    assert crossing[255][0][:-8] == crossing[256][0][:-8] != crossing[254][0][:-8]
    check_view(torch_cuda, crossing, 8)
    check_view(torch_cuda, crossing[1:], 8)  # the key now starts at 254, its head hidden at 8 sits at 254
    check_view(torch_cuda, crossing[2:], 7)


def test_plan_bad_input_unsorted_and_aliasing(torch_cuda):
    from lsbm_amd import _lib
    torch = torch_cuda
    lib = _lib.lib()
    good = [sm.ikey(b"a", 5), sm.ikey(b"b", 4), sm.ikey(b"b", 3), sm.ikey(b"c", 9)]
    b, off = pack(good)
    cases = [(good, None, OK),
             (good, [0, 9, 8, 27, 36], BAD_INPUT),           # offsets that decrease
             (good, [0, 9, 18, 27, 37], BAD_INPUT),          # the last one passes the buffer
             ([good[0], b"7 bytes", good[3]], None, BAD_INPUT),
             ([good[1], good[0]], None, UNSORTED),           # user keys out of order
             ([good[2], good[1]], None, UNSORTED),           # the tag ascending
             ([good[1], good[1]], None, OK)]                 # equal neighbours are legal
    for keys_list, offsets, want in cases:
        kb, koff = pack(keys_list)
        keys = _dev(torch, kb)
        offs = _dev(torch, np.array(offsets, dtype=np.int64) if offsets else koff)
        n = len(keys_list)
        outs = {name: guarded(torch, size, torch.int64, -7) for name, size in
                (("source", n), ("out_off", n + 1), ("counts", 3), ("yr", n + 1), ("cr", n + 1), ("first", n),
                 ("back", n))}
        gs, status = guarded(torch, 1, torch.int32, -7)
        nbytes = lib.lsbm_dbiter_scratch_bytes(n)
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
        rc = lib.lsbm_dbiter_plan_dev(ptr(keys), keys.numel(), ptr(offs), n, 6, *(ptr(outs[k][1]) for k in
                                      ("source", "out_off", "counts", "yr", "cr", "first", "back")), ptr(status),
                                      ptr(scratch), scratch.numel() * 8, stream_ptr(torch))
        assert rc == 0 and status.cpu().tolist() == [want], (keys_list, offsets)
        assert guards_intact(gs, 1, -7)
        for name, (whole, view) in outs.items():
            assert guards_intact(whole, view.numel(), -7), name
            if want != OK:  # canaries: nothing but the status word is written
                assert bool((view == -7).all()), (name, want)
        if want == OK:
            assert outs["counts"][1].cpu().tolist()[0] == sm.View([(k, b"") for k in keys_list], 6).n_yield
    # aliasing: an output over the keys, and two outputs over each other
    keys, offs = _dev(torch, b), _dev(torch, off)
    n = 4
    o = [torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(7)]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(64, dtype=torch.int64, device="cuda")

    def call(source, yr):
        return lib.lsbm_dbiter_plan_dev(ptr(keys), keys.numel(), ptr(offs), n, 6, ptr(source), ptr(o[1]), ptr(o[2]),
                                        ptr(yr), ptr(o[4]), ptr(o[5]), ptr(o[6]), ptr(status), ptr(scratch), 512,
                                        stream_ptr(torch))
    assert call(o[0], o[3]) == 0
    assert call(offs, o[3]) == ERR_INVALID
    assert call(o[0], o[0]) == ERR_INVALID
    assert lib.lsbm_dbiter_plan_dev(ptr(keys), keys.numel(), ptr(offs), n, 6, ptr(o[0]), ptr(o[1]), ptr(o[2]),
                                    ptr(o[3]), ptr(o[4]), ptr(o[5]), ptr(o[6]), ptr(status), ptr(scratch), 8,
                                    stream_ptr(torch)) == ERR_INVALID  # scratch too small


# ---------------------------------------------------------------- range and emit


@pytest.mark.parametrize("case", range(3))
def test_scan_reproduces_every_fixture_query(torch_cuda, case):
    from lsbm_amd import scan
    torch = torch_cuda
    name, _, merged, queries = scan_cases.cases()[case]
    keys, koff, values, image = dev_entries(torch, merged)
    groups = {}
    for q in queries:
        groups.setdefault((q[0], q[4]), []).append(q)
    for (s, rev), qs in groups.items():
        view = scan.view(keys, koff, values, image, s)
        got = run_scan(torch, view, [(lo, hi, limit) for _, lo, hi, limit, _, _, _ in qs], rev)
        for (out, st), (_, lo, hi, limit, _, want, status) in zip(got, qs):
            assert out == want, (name, s, lo, hi, limit, rev)
            assert scan.status_string(st) == status, (name, s, lo, hi, limit, rev)


def sized_history():
    """Keys of 8 bytes (the empty user key) and 137 + 8 bytes, values of 0 / 1 / 15 / 16 / 17 / 4,097 bytes."""
    sizes = [0, 1, 15, 16, 17, 4097]
    entries = [(sm.ikey(b"", 5), b"E" * 17), (sm.ikey(b"K" * 137, 6), b"L" * 4097)]
    for i in range(200):
        user = b"g%03d" % i + b"x" * (i % 11)
        entries.append((sm.ikey(user, 9, 0 if i % 17 == 3 else 1), bytes([65 + i % 26]) * sizes[i % 6]))
        if i % 5 == 0:
            entries.append((sm.ikey(user, 4, 1), b"old"))
        if i % 23 == 0:
            entries.append((sm.ikey(user, 7, 2), b"bad"))
    return sm.sort_entries(entries)


@pytest.mark.parametrize("q", [0, 1, 255, 256, 257])
def test_scan_query_counts_sizes_and_directions(torch_cuda, q):
    from lsbm_amd import scan
    torch = torch_cuda
    entries = sized_history()
    users = sorted({k[:-8] for k, _ in entries})
    rng = random.Random(0xE317 + q)
    pool = [(None, None, 1000), (b"", None, 63), (b"", None, 64), (b"", None, 65), (None, b"K" * 137 + b"\x00", 65),
            (users[3], users[70], 64), (b"K" * 137, None, 1), (b"", b"g", 1), (users[9], users[9], 5),
            (users[50], users[20], 5), (b"zzz", None, 3), (None, b"", 3), (users[100], None, 0)]
    pool += [(rng.choice(users + [None]), rng.choice(users + [None]), rng.choice([0, 1, 2, 63, 64, 65, 1000]))
             for _ in range(40)]
    queries = [pool[i % len(pool)] for i in range(q)]
    keys, koff, values, image = dev_entries(torch, entries)
    for s in (5, 9):
        view = scan.view(keys, koff, values, image, s)
        for rev in (False, True):
            got = run_scan(torch, view, queries, rev)
            assert got == model_scan(entries, s, queries, rev), (q, s, rev)
    if q == 257:
        counts = {len(out) for out, _ in got}
        assert {0, 1, 63, 64, 65} <= counts


def test_seek_and_ends(torch_cuda):
    from lsbm_amd import scan
    torch = torch_cuda
    entries = sized_history()
    keys, koff, values, image = dev_entries(torch, entries)
    view = scan.view(keys, koff, values, image, 9)
    users = [b"", b"g", b"g0035", b"K" * 137, b"zzzz"]
    uk, uoff = dev_keys(torch, users)
    r = view.seek(uk, uoff)
    kb, off, first = r.keys.cpu().numpy().tobytes(), r.key_offsets.cpu().tolist(), r.entry_first.cpu().tolist()
    got = [[kb[off[i]:off[i + 1]] for i in range(first[q], first[q + 1])] for q in range(len(users))]
    assert got == [[k for k, _ in sm.scan_port(entries, 9, u, None, 1)[0]] for u in users]
    all_fwd = sm.scan_port(entries, 9)[0]
    for r, want in ((view.seek_to_first(), all_fwd[0]), (view.seek_to_last(), all_fwd[-1])):
        assert (r.keys.cpu().numpy().tobytes(), r.values.cpu().numpy().tobytes()) == want
    assert scan.status_string(0) == "OK"
    assert scan.status_string(1) == "Corruption: corrupted internal key in DBIter"


def raw_emit(torch, view, r, sums, reverse, caps, fill=GUARD):
    """lsbm_dbiter_emit_dev into guarded buffers of `caps` = (entries, key bytes, value bytes)."""
    from lsbm_amd import _lib
    gk, ok = guarded(torch, caps[1], torch.uint8, fill, 64)
    gv, ov = guarded(torch, caps[2], torch.uint8, fill, 64)
    gko, oko = guarded(torch, caps[0] + 1, torch.int64, -7)
    gvo, ovo = guarded(torch, caps[0] + 1, torch.int64, -7)
    gs, st = guarded(torch, 1, torch.int32, -7)
    rc = _lib.lib().lsbm_dbiter_emit_dev(
        ptr(r.j_begin), ptr(sums[0]), ptr(sums[1]), ptr(sums[2]), r.count.numel(), int(reverse), ptr(view.live_keys),
        view.live_keys.numel(), ptr(view.live_key_offsets), ptr(view.live_values), view.n_yield,
        ptr(view.value_prefix), ptr(view.value_image), view.value_image.numel(), ptr(ok), caps[1], ptr(oko), ptr(ov),
        caps[2], ptr(ovo), caps[0], ptr(st), stream_ptr(torch))
    intact = (guards_intact(gk, caps[1], fill, 64) and guards_intact(gv, caps[2], fill, 64)
              and guards_intact(gko, caps[0] + 1, -7) and guards_intact(gvo, caps[0] + 1, -7)
              and guards_intact(gs, 1, -7))
    return rc, st.cpu().tolist()[0], (ok, oko, ov, ovo), intact


def test_emit_guards_no_room_and_bad_input(torch_cuda):
    from lsbm_amd import _lib, scan
    torch = torch_cuda
    entries = sized_history()
    keys, koff, values, image = dev_entries(torch, entries)
    view = scan.view(keys, koff, values, image, 9)
    users = sorted({k[:-8] for k, _ in entries})
    queries = [(None, None, 1000), (users[5], users[90], 70), (b"", None, 1), (users[150], None, 3)]
    lo, lo_off, lo_p = bounds(torch, [q[0] for q in queries])
    hi, hi_off, hi_p = bounds(torch, [q[1] for q in queries])
    limits = _dev(torch, np.array([q[2] for q in queries], dtype=np.int64))
    for rev in (False, True):
        r = view.range(lo, lo_off, hi, hi_off, limit=limits, reverse=rev, lo_present=lo_p, hi_present=hi_p)
        assert r.call_status.cpu().tolist() == [OK]
        sums = torch.zeros((3, len(queries) + 1), dtype=torch.int64, device="cuda")
        for i, t in enumerate((r.count, r.key_bytes, r.value_bytes)):
            torch.cumsum(t, 0, out=sums[i, 1:])
        totals = sums[:, -1].cpu().tolist()
        want = model_scan(entries, 9, queries, rev)
        assert totals == [sum(len(o) for o, _ in want), sum(len(k) for o, _ in want for k, _ in o),
                          sum(len(v) for o, _ in want for _, v in o)]
        rc, st, outs, intact = raw_emit(torch, view, r, sums, rev, totals)
        assert (rc, st, intact) == (0, OK, True)
        assert outs[0].cpu().numpy().tobytes() == b"".join(k for o, _ in want for k, _ in o)
        assert outs[2].cpu().numpy().tobytes() == b"".join(v for o, _ in want for _, v in o)
        # caps one entry and one byte short: NO_ROOM and no store
        for short in ((totals[0] - 1, totals[1], totals[2]), (totals[0], totals[1] - 1, totals[2]),
                      (totals[0], totals[1], totals[2] - 1)):
            rc, st, outs, intact = raw_emit(torch, view, r, sums, rev, short)
            assert (rc, st, intact) == (0, NO_ROOM, True)
            assert bool((outs[0] == GUARD).all()) and bool((outs[2] == GUARD).all())
            assert bool((outs[1] == -7).all()) and bool((outs[3] == -7).all())
        # a prefix array that decreases: BAD_INPUT and no store
        broken = sums.clone()
        broken[0, 2] = broken[0, 1] - 1
        rc, st, outs, intact = raw_emit(torch, view, r, broken, rev, totals)
        assert (rc, st, intact) == (0, BAD_INPUT, True)
        assert bool((outs[0] == GUARD).all()) and bool((outs[1] == -7).all())
    # aliasing: the key output over the live keys
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    o = torch.zeros(totals[0] + 1, dtype=torch.int64, device="cuda")
    o2 = torch.zeros(totals[0] + 1, dtype=torch.int64, device="cuda")
    ov = torch.zeros(max(totals[2], 1), dtype=torch.uint8, device="cuda")
    rc = _lib.lib().lsbm_dbiter_emit_dev(
        ptr(r.j_begin), ptr(sums[0]), ptr(sums[1]), ptr(sums[2]), len(queries), 0, ptr(view.live_keys),
        view.live_keys.numel(), ptr(view.live_key_offsets), ptr(view.live_values), view.n_yield,
        ptr(view.value_prefix), ptr(view.value_image), view.value_image.numel(), ptr(view.live_keys),
        view.live_keys.numel(), ptr(o), ptr(ov), ov.numel(), ptr(o2), totals[0], ptr(st), stream_ptr(torch))
    assert rc == ERR_INVALID


def test_range_bad_input_canaries_and_aliasing(torch_cuda):
    from lsbm_amd import _lib, scan
    torch = torch_cuda
    lib = _lib.lib()
    entries = history_of(300, 77)
    keys, koff, values, image = dev_entries(torch, entries)
    view = scan.view(keys, koff, values, image, 15)
    p = view.plan
    lo, lo_off = dev_keys(torch, [b"u00003", b"u00010", b"u00020"])
    hi, hi_off = dev_keys(torch, [b"u00005", b"u00030", b"u00021"])
    nq = 3

    def call(entry_off, lo_offsets, hi_offsets, j_begin=None, count=None):
        outs = {name: guarded(torch, nq, torch.int64, -7) for name in ("j", "c", "kb", "vb")}
        gss, ss = guarded(torch, nq, torch.int32, -7)
        st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        rc = lib.lsbm_dbiter_range_dev(
            ptr(keys), keys.numel(), ptr(entry_off), len(entries), 15, ptr(p.source), ptr(p.out_key_offsets),
            ptr(p.counts), ptr(p.yield_rank), ptr(p.corrupt_rank), ptr(p.first), ptr(p.back), ptr(view.value_prefix),
            ptr(lo), lo.numel(), ptr(lo_offsets), None, ptr(hi), hi.numel(), ptr(hi_offsets), None, nq, 5, None, 0,
            ptr(j_begin if j_begin is not None else outs["j"][1]), ptr(count if count is not None else outs["c"][1]),
            ptr(ss), ptr(outs["kb"][1]), ptr(outs["vb"][1]), ptr(st), stream_ptr(torch))
        written = any(not bool((v == -7).all()) for _, v in outs.values()) or not bool((ss == -7).all())
        intact = all(guards_intact(w, nq, -7) for w, _ in outs.values()) and guards_intact(gss, nq, -7)
        return rc, st.cpu().tolist()[0], written, intact, outs

    rc, st, written, intact, outs = call(koff, lo_off, hi_off)
    assert (rc, st, written, intact) == (0, OK, True, True)
    want = [sm.scan_closed(sm.View(entries, 15), a, b, 5) for a, b in
            ((b"u00003", b"u00005"), (b"u00010", b"u00030"), (b"u00020", b"u00021"))]
    assert list(zip(outs["j"][1].cpu().tolist(), outs["c"][1].cpu().tolist())) == [(j, c) for j, c, _ in want]
    bad_lo = _dev(torch, np.array([0, 6, 5, 18], dtype=np.int64))       # decreases
    past_hi = _dev(torch, np.array([0, 6, 12, 19], dtype=np.int64))     # passes its buffer
    bad_entries = koff.clone()
    bad_entries[7] = bad_entries[8] - 7                                  # a 7-byte key (and its neighbour grows)
    for args in ((koff, bad_lo, hi_off), (koff, lo_off, past_hi), (bad_entries, lo_off, hi_off)):
        rc, st, written, intact, _ = call(*args)
        assert (rc, st, written, intact) == (0, BAD_INPUT, False, True)
    # aliasing: an output over an input, two outputs over each other
    same = torch.zeros(nq, dtype=torch.int64, device="cuda")
    assert call(koff, lo_off, hi_off, j_begin=same, count=same)[0] == ERR_INVALID
    assert call(koff, lo_off, hi_off, j_begin=lo_off[:nq])[0] == ERR_INVALID


# ---------------------------------------------------------------- the chain


def table_entries(data, uncompress, verify=True):
    """Every (internal key, value) of a table file, through the models of ReadBlock and Block::Iter."""
    _, index_handle = stm.decode_footer(data)
    st, index, _ = stm.read_block(data, index_handle, uncompress, verify)
    assert st == stm.READ_OK
    out = []
    for _, vo, vl, _ in bm.walk(index)[1]:
        st, contents, _ = stm.read_block(data, bm.decode_handle(bytes(index[vo:vo + vl])), uncompress, verify)
        assert st == stm.READ_OK
        out += [(k, bytes(contents[o:o + ln])) for k, o, ln, _ in bm.walk(contents)[1]]
    return out


def open_device_version(v, blob):
    from lsbm_amd import db
    bits = 10 if v["filter_policy"] else None
    files = [db.TableFile(blob[f["file"][0]:f["file"][0] + f["file"][1]], f["number"], bits,
                          bytes.fromhex(f["smallest"]), bytes.fromhex(f["largest"])) for f in v["files"]]
    return db.Version(files, [db.Run(idx, flags) for flags, idx in v["runs"]])


def dev_memtable(torch, entries):
    from lsbm_amd import db
    return db.MemTable(*dev_entries(torch, entries))


def merged_model(children):
    """The MergingIterator's order over children [[(key, value)]]: the stable merge."""
    return sm.sort_entries([e for child in children for e in child])


def test_version_view_scans_the_get_fixture_versions(torch_cuda, fx, snappy_oracle):
    from lsbm_amd import scan
    torch = torch_cuda
    fixture, blob = fx
    uncompress = codec(snappy_oracle)
    by = {v["name"]: v for v in fixture["versions"]}
    seen = set()
    for name in ("tree", "tree_flipped_block_no_verify", "wrong_bytes"):
        v = by[name]
        verify = bool(v["verify"])
        version = open_device_version(v, blob)
        mem_models = [memtable_of(m) for m in v["memtables"]]
        mems = [dev_memtable(torch, m) for m in mem_models]
        datas = [bytes(blob[f["file"][0]:f["file"][0] + f["file"][1]]) for f in v["files"]]
        runs = [[e for f in idx for e in table_entries(datas[f], uncompress, verify)] for _, idx in v["runs"]]
        merged = merged_model(mem_models + runs)
        users = sorted({bytes.fromhex(u) for u, _ in v["queries"]})
        rng = random.Random(len(users))
        queries = [(None, None, 1000)] + [(u, None, 1) for u in users] + \
            [(rng.choice(users), rng.choice(users), rng.choice([1, 2, 7, 1000])) for _ in range(60)]
        for s in sorted({s for _, s in v["queries"]}):
            view = version.view(s, mems, verify=verify)
            assert view.n == len(merged)
            for rev in (False, True):
                got = run_scan(torch, view, queries, rev)
                assert got == model_scan(merged, s, queries, rev), (name, s, rev)
                seen |= {st for _, st in got}
    assert seen == {scan.SCAN_OK, scan.SCAN_CORRUPTION}
    # runs: AddIterators leaves out Level 0's insertion part (empty in the fixture's tree: the same view)
    tree = open_device_version(by["tree"], blob)
    assert tree.scan_runs() == [r for r in range(len(tree.runs)) if r != 3]
    a, b = tree.view(9999), tree.view(9999, runs=tree.scan_runs())
    assert a.n == b.n and a.n_yield == b.n_yield
    # a table read error is raised when the view is built, as is a run whose files overlap
    with pytest.raises(ValueError, match="block checksum mismatch"):
        open_device_version(by["tree_flipped_block"], blob).view(9999)
    with pytest.raises(ValueError):
        open_device_version(by["bad_index_plain"], blob).view(9999)
    v = by["tree"]
    overlapping = open_device_version(dict(v, runs=[[0, [3, 4, 0]]]), blob)
    with pytest.raises(ValueError, match="not sorted"):
        overlapping.view(9999)
    with pytest.raises(ValueError, match="at most"):
        tree.view(9999, runs=[0] * 65)


def test_round_trip_flush_compact_scan_agrees_with_get(torch_cuda):
    """Two logs flushed by memtable.flush, compacted into a level by
    sstable.compact, a third log as the memtable: scan(lo=k, limit=1) yields k
    with Get's value iff Version.get says FOUND, and a full forward scan is a
    full reverse scan, reversed."""
    from lsbm_amd import db, memtable, sstable
    from lsbm_amd.table import kSnappyCompression
    torch = torch_cuda
    rng = random.Random(0x7218)
    users = [b"key%04d" % i for i in range(300)]

    def batches(seq0, n):
        out, seq = [], seq0
        for _ in range(n):
            ops = [(rng.choice((0, 1, 1, 1)), rng.choice(users), b"v%d-" % seq + b"x" * rng.randrange(0, 30))
                   for _ in range(rng.randrange(1, 9))]
            out.append(struct.pack("<QI", seq, len(ops)) + b"".join(
                bytes([t]) + bytes([len(k)]) + k + (bytes([len(v)]) + v if t else b"") for t, k, v in ops))
            seq += len(ops)
        return out, seq

    logs, seq = [], 1
    for _ in range(3):
        recs, seq = batches(seq, 60)
        logs.append(recs)

    def on_device(recs):
        buf = b"".join(recs)
        at = np.cumsum([0] + [len(r) for r in recs])
        pairs = [(int(at[i]), len(r)) for i, r in enumerate(recs)]
        return buf, pairs, _dev(torch, np.frombuffer(buf, dtype=np.uint8)), \
            _dev(torch, np.array(pairs, dtype=np.int64).reshape(-1))

    flushed, models = [], []
    for recs in logs[:2]:
        buf, pairs, image, records = on_device(recs)
        flushed.append(memtable.flush(image, records, compression=kSnappyCompression, block_size=256,
                                      restart_interval=4, bits_per_key=10))
        models.append(mt.entries(buf, pairs)[0])
    outs = sstable.compact([f.image for f in flushed], index_handles=[f.index_handle for f in flushed],
                           max_file_size=3000, block_size=256, restart_interval=4, bits_per_key=10,
                           compression=kSnappyCompression)
    assert len(outs) >= 2
    level = [db.TableFile(bytes(o.image.cpu().numpy()), 10 + i, 10) for i, o in enumerate(outs)]
    newest = db.TableFile(bytes(flushed[1].image.cpu().numpy()), 5, 10)
    version = db.Version.for_levels([newest], [], [(level, [])])
    buf, pairs, image, records = on_device(logs[2])
    e = memtable.entries(image, records)
    mem = db.MemTable(e.keys, e.key_offsets, e.values, image)
    mem_model = mt.entries(buf, pairs)[0]
    # the merged entries: the memtable, the newest flush, and the level (the compaction of both flushes, no drop)
    merged = merged_model([mem_model, models[1], merged_model([models[0], models[1]])])
    probes = users + [b"", b"key", b"key9999"]
    uk, uoff = dev_keys(torch, probes)
    found_any = 0
    for s in (30, seq // 2, seq + 5):
        view = version.view(s, [mem], runs=version.scan_runs())
        assert view.n == len(merged)
        got = version.get(uk, uoff, s, [mem])
        status, off = got.status.cpu().tolist(), got.value_offsets.cpu().tolist()
        vbuf = got.values.cpu().numpy().tobytes()
        r = run_scan(torch, view, [(u, None, 1) for u in probes], False)
        for q, u in enumerate(probes):
            hit = bool(r[q][0]) and r[q][0][0][0] == u
            assert hit == (status[q] == db.FOUND), (s, u)
            if hit:
                assert r[q][0][0][1] == vbuf[off[q]:off[q + 1]], (s, u)
                found_any += 1
        fwd = run_scan(torch, view, [(None, None, 1 << 40)], False)[0]
        rev = run_scan(torch, view, [(None, None, 1 << 40)], True)[0]
        assert fwd[0] == rev[0][::-1] and fwd[1] == rev[1] == 0
        assert fwd[0] == sm.scan_port(merged, s)[0]
    assert found_any > 100
