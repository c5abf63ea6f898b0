"""Batched DB::Get on the GPU (include/lsbm_get.h, lsbm_amd/db.py): every kernel
and the whole chain, exact against the reference's fixture
(tests/golden/get_fixture.json, get_tables.bin) and the plain-Python model
(tests/golden/getmodel.py, pinned to that fixture by tests/test_db_get.py).
"""
import ctypes
import random
import struct

import numpy as np
import pytest

from golden import getmodel as gm
from golden import memtablemodel as mt
from test_db_get import codec, fx, iteration, memtable_of  # noqa: F401 (fx is a fixture)

pytestmark = pytest.mark.gpu

GUARD = 0xEE
SIZES = (0, 1, 255, 256, 257)
ERR_INVALID = -1


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


def guarded(torch, n, dtype, fill, pad=16):
    """(whole tensor, the n-element view between two guard zones)."""
    whole = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
    return whole, whole[pad:pad + n]


def guards_intact(whole, n, fill, pad=16):
    h = whole.cpu().numpy()
    return bool(np.all(h[:pad] == fill) and np.all(h[pad + n:] == fill))


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_memtable(torch, entries):
    """db.MemTable of sorted [(internal key, value)]: the values side by side in an image."""
    from lsbm_amd import db
    keys, koff = dev_keys(torch, [k for k, _ in entries])
    image, voff = pack([v for _, v in entries])
    values = np.stack([voff[:-1], voff[1:] - voff[:-1]], 1) if entries else np.zeros((0, 2), dtype=np.int64)
    return db.MemTable(keys, koff, _dev(torch, values.astype(np.int64)), _dev(torch, image))


def values_of(result):
    """[bytes] per query of a DbGetResult."""
    off = result.value_offsets.cpu().tolist()
    buf = result.values.cpu().numpy().tobytes()
    return [buf[off[q]:off[q + 1]] for q in range(len(off) - 1)]


def tile(items, n):
    return [items[i % len(items)] for i in range(n)] if items else []


# ---------------------------------------------------------------- lookup keys


def test_lookup_keys_sizes_snapshots_and_guards(torch_cuda):
    from lsbm_amd import _lib, db
    torch = torch_cuda
    rng = random.Random(0x100C)
    pool = [b"", b"a", b"1234567", b"12345678", b"123456789", b"x" * 137] + \
        [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40))) for _ in range(40)]
    for n in SIZES:
        users = tile(pool, n)
        uk, uoff = dev_keys(torch, users)
        seqs = [rng.randrange(1 << 56) for _ in range(n)]
        for snaps in (12345, (1 << 56) - 1, _dev(torch, np.array(seqs, dtype=np.int64))):
            keys, off, st = db.lookup_keys(uk, uoff, snaps)
            assert st.cpu().tolist() == [0]
            off_h, keys_h = off.cpu().tolist(), keys.cpu().numpy().tobytes()
            assert off_h == [int(uoff[q]) + 8 * q for q in range(n + 1)]
            want = [gm.lookup_key(u, snaps if isinstance(snaps, int) else seqs[q]) for q, u in enumerate(users)]
            assert [keys_h[off_h[q]:off_h[q + 1]] for q in range(n)] == want
        # guard bytes around both outputs
        cap = uk.numel() + 8 * n
        gk, kview = guarded(torch, cap, torch.uint8, GUARD, 64)
        go, oview = guarded(torch, n + 1, torch.int64, -2)
        gs, sview = guarded(torch, 1, torch.int32, -2)
        rc = _lib.lib().lsbm_lookup_keys_dev(ptr(uk), uk.numel(), ptr(uoff), n, 77, None, ptr(kview), cap, ptr(oview),
                                             ptr(sview), stream_ptr(torch))
        assert rc == 0 and sview.cpu().tolist() == [0]
        assert guards_intact(gk, cap, GUARD, 64) and guards_intact(go, n + 1, -2) and guards_intact(gs, 1, -2)
        assert kview.cpu().numpy().tobytes() == b"".join(gm.lookup_key(u, 77) for u in users)


def test_lookup_keys_bad_input_and_aliasing(torch_cuda):
    from lsbm_amd import _lib, db
    torch = torch_cuda
    uk, uoff = dev_keys(torch, [b"abc", b"de", b"f"])
    for bad in ([0, 3, 2, 6], [0, 3, 5, 7], [1 << 40, 3, 5, 6]):
        keys, off, st = db.lookup_keys(uk, _dev(torch, np.array(bad, dtype=np.int64)), 5)
        assert st.cpu().tolist() == [db.MERGE_BAD_INPUT]
        assert not keys.cpu().numpy().any() and not off.cpu().numpy().any()  # nothing written
    # one byte of room too few
    out = torch.zeros(6 + 24, dtype=torch.uint8, device="cuda")
    off = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = _lib.lib()
    assert lib.lsbm_lookup_keys_dev(ptr(uk), 6, ptr(uoff), 3, 5, None, ptr(out), 29, ptr(off), ptr(st),
                                    stream_ptr(torch)) == 0
    assert st.cpu().tolist() == [db.MERGE_BAD_INPUT] and not out.cpu().numpy().any()
    # an output that aliases an input
    both = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.lsbm_lookup_keys_dev(ptr(both), 6, ptr(uoff), 3, 5, None, ptr(both[4:]), 30, ptr(off), ptr(st),
                                    stream_ptr(torch)) == ERR_INVALID
    assert lib.lsbm_lookup_keys_dev(ptr(uk), 6, ptr(uoff), 3, 5, None, ptr(out), 30, ptr(uoff), ptr(st),
                                    stream_ptr(torch)) == ERR_INVALID


# ---------------------------------------------------------------- the memtable


def test_memtable_get_reproduces_fixture(torch_cuda, fx):
    from lsbm_amd import db
    torch = torch_cuda
    fixture, blob = fx
    for m in fixture["memtables"]:
        entries = iteration(blob, m["iteration"], m["n_entries"])
        mem = dev_memtable(torch, entries)
        users = [bytes.fromhex(q[0]) for q in m["queries"]]
        seqs = [q[1] for q in m["queries"]]
        uk, uoff = dev_keys(torch, users)
        r = db.memtable_get(mem, uk, uoff, _dev(torch, np.array(seqs, dtype=np.int64)))
        status, where, values = r.status.cpu().tolist(), r.where.cpu().tolist(), values_of(r)
        for q, (_, _, got, text, vhex) in enumerate(m["queries"]):
            what = (m["name"], users[q], seqs[q])
            assert (status[q] != db.UNDECIDED) == bool(got), what
            assert where[q] == (0 if got else -1), what
            if got:
                assert db.status_string(status[q]) == text, what
            assert values[q].hex() == vhex, what
            verdict, value = gm.memtable_get(entries, users[q], seqs[q])
            assert (status[q], values[q]) == (verdict, value or b""), what


def test_memtable_get_sizes_canaries_and_guards(torch_cuda, fx):
    from lsbm_amd import db
    torch = torch_cuda
    fixture, blob = fx
    m = next(c for c in fixture["memtables"] if c["name"] == "entries_257")
    entries = iteration(blob, m["iteration"], m["n_entries"])
    mem = dev_memtable(torch, entries)
    pool = [(bytes.fromhex(q[0]), q[1]) for q in m["queries"]]
    for n in SIZES:
        qs = tile(pool, n)
        keys, off = dev_keys(torch, [gm.lookup_key(u, s) for u, s in qs])
        gv, verdict = guarded(torch, n, torch.int32, 0x7E)
        gw, where = guarded(torch, n, torch.int32, -9)
        gx, value = guarded(torch, 2 * n, torch.int64, -7)
        canary = [q % 3 == 1 for q in range(n)]  # decided on entry: left untouched
        verdict.copy_(_dev(torch, np.array([77 if c else 0 for c in canary], dtype=np.int32)))
        st = db.memtable_probe(mem, keys, off, 5, verdict, value.view(n, 2), where)
        assert st.cpu().tolist() == [0]
        assert guards_intact(gv, n, 0x7E) and guards_intact(gw, n, -9) and guards_intact(gx, 2 * n, -7)
        vh, wh, xh = verdict.cpu().tolist(), where.cpu().tolist(), value.view(n, 2).cpu().tolist()
        image = mem.image.cpu().numpy().tobytes()
        for q, (u, s) in enumerate(qs):
            if canary[q]:
                assert (vh[q], wh[q], xh[q]) == (77, -9, [-7, -7]), q
                continue
            want, wv = gm.memtable_get(entries, u, s)
            assert vh[q] == want, (n, q)
            if want == gm.UNDECIDED:
                assert (wh[q], xh[q]) == (-9, [-7, -7]), q
            else:
                assert wh[q] == 5 and image[xh[q][0]:xh[q][0] + xh[q][1]] == (wv or b""), q
                assert want == gm.FOUND or xh[q] == [0, 0]


def test_memtable_get_bad_input_and_aliasing(torch_cuda):
    from lsbm_amd import _lib, db
    torch = torch_cuda
    entries = [(gm.lookup_key(b"a", 5), b"x"), (gm.lookup_key(b"b", 5), b"y")]
    mem = dev_memtable(torch, entries)
    keys, off = dev_keys(torch, [gm.lookup_key(b"a", 9), gm.lookup_key(b"b", 9)])
    verdict, value, where = db.new_verdicts(2, keys.device)

    def untouched():
        return verdict.cpu().tolist() == [0, 0] and where.cpu().tolist() == [-1, -1] and not value.cpu().numpy().any()

    short_q = _dev(torch, np.array([0, 7, 18], dtype=np.int64))  # a lookup key under 8 bytes
    assert db.memtable_probe(mem, keys, short_q, 0, verdict, value, where).cpu().tolist() == [db.MERGE_BAD_INPUT]
    assert untouched()
    for bad in ([0, 7, 18], [0, 12, 9], [0, 9, 19]):  # a memtable key under 8 bytes, decreasing, past the keys
        broken = mem._replace(key_offsets=_dev(torch, np.array(bad, dtype=np.int64)))
        assert db.memtable_probe(broken, keys, off, 0, verdict, value, where).cpu().tolist() == [db.MERGE_BAD_INPUT]
        assert untouched()
    assert db.memtable_probe(mem, keys, off, 0, verdict, value, where).cpu().tolist() == [0]
    assert verdict.cpu().tolist() == [gm.FOUND, gm.FOUND]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = _lib.lib()
    args = [ptr(mem.keys), mem.keys.numel(), ptr(mem.key_offsets), ptr(mem.values), 2, ptr(keys), keys.numel(), ptr(off), 2,
            0, ptr(verdict), ptr(value), ptr(where), ptr(st), stream_ptr(torch)]
    assert lib.lsbm_memtable_get_dev(*args) == 0
    for slot, alias in ((10, mem.key_offsets), (11, mem.values), (12, off), (13, keys)):
        broken = list(args)
        broken[slot] = ptr(alias)
        assert lib.lsbm_memtable_get_dev(*broken) == ERR_INVALID, slot


# ---------------------------------------------------------------- the file pick


def dev_bounds(torch, bounds):
    return dev_keys(torch, [k for pair in bounds for k in pair])


def test_find_file_reproduces_fixture(torch_cuda, fx):
    from lsbm_amd import db
    torch = torch_cuda
    fixture, _ = fx
    for c in fixture["find_file"]:
        bounds = [(bytes.fromhex(s), bytes.fromhex(g)) for s, g, _ in c["files"]]
        nf = len(bounds)
        visible = _dev(torch, np.array([v for _, _, v in c["files"]], dtype=np.uint8))
        all_visible = torch.ones_like(visible)
        b, boff = dev_bounds(torch, bounds)
        queries = [bytes.fromhex(q[0]) for q in c["queries"]]
        keys, off = dev_keys(torch, queries)
        # one sorted run of every file
        first = _dev(torch, np.array([0, nf], dtype=np.int64))
        flags = _dev(torch, np.array([0], dtype=np.int32))
        seen, st = db.find_file(b, boff, first, flags, visible, keys, off)
        plain, st2 = db.find_file(b, boff, first, flags, all_visible, keys, off)
        assert st.cpu().tolist() == [0] and st2.cpu().tolist() == [0]
        seen, plain = seen[:, 0].cpu().tolist(), plain[:, 0].cpu().tolist()
        for q, (_, index, covered, covered_visible, _) in enumerate(c["queries"]):
            assert plain[q] == (index if covered else -1), (c["name"], q)
            assert seen[q] == (index if covered_visible else -1), (c["name"], q)
        # every file as a LEVEL0 run of its own, and an empty run between them
        first = _dev(torch, np.array(sorted(list(range(nf + 1)) + [nf // 2]), dtype=np.int64))
        flags = _dev(torch, np.array([db.RUN_LEVEL0] * (nf + 1), dtype=np.int32))
        got, st = db.find_file(b, boff, first, flags, torch.zeros_like(visible), keys, off)
        assert st.cpu().tolist() == [0]
        got = got.cpu().tolist()
        runs_of = [r for r in range(nf + 1) if r != nf // 2]  # (run nf // 2 is the empty one)
        for q, rec in enumerate(c["queries"]):
            assert got[q][nf // 2] == -1
            assert [got[q][r] for r in runs_of] == [f if bit else -1 for f, bit in enumerate(bytes.fromhex(rec[4]))]


def test_find_file_sizes_runs_and_guards(torch_cuda, fx):
    from lsbm_amd import _lib, db
    torch = torch_cuda
    fixture, _ = fx
    c = next(c for c in fixture["find_file"] if c["name"] == "files_65")
    bounds = [(bytes.fromhex(s), bytes.fromhex(g)) for s, g, _ in c["files"]]
    b, boff = dev_bounds(torch, bounds)
    cuts = [0, 0, 1, 3, 3, 64, 65]  # runs of 0, 1, 2, 0, 61 and 1 files
    flag_list = [0, db.RUN_LEVEL0, db.RUN_PRECHECKED, 0, 0, db.RUN_LEVEL0 | db.RUN_PRECHECKED]
    first = _dev(torch, np.array(cuts, dtype=np.int64))
    flags = _dev(torch, np.array(flag_list, dtype=np.int32))
    visible = _dev(torch, np.array([f % 5 != 4 for f in range(65)], dtype=np.uint8))
    pool = [bytes.fromhex(q[0]) for q in c["queries"]]
    nr = len(flag_list)
    for n in SIZES:
        qs = tile(pool, n)
        keys, off = dev_keys(torch, qs)
        gf, file = guarded(torch, n * nr, torch.int32, -5)
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = _lib.lib().lsbm_find_file_dev(ptr(b), b.numel(), ptr(boff), 65, ptr(first), ptr(flags), ptr(visible), nr,
                                           ptr(keys), keys.numel(), ptr(off), n, ptr(file), ptr(st), stream_ptr(torch))
        assert rc == 0 and st.cpu().tolist() == [0] and guards_intact(gf, n * nr, -5)
        got = file.view(n, nr).cpu().tolist()
        for q, k in enumerate(qs):
            for r in range(nr):
                lo, hi = cuts[r], cuts[r + 1]
                at = gm.pick(bounds[lo:hi], flag_list[r], k, [f % 5 != 4 for f in range(lo, hi)])
                assert got[q][r] == (lo + at if at >= 0 else -1), (n, q, r)


def test_find_file_bad_input_and_aliasing(torch_cuda):
    from lsbm_amd import _lib, db
    torch = torch_cuda
    bounds = [(gm.lookup_key(b"a", 9), gm.lookup_key(b"c", 1)), (gm.lookup_key(b"e", 9), gm.lookup_key(b"g", 1))]
    b, boff = dev_bounds(torch, bounds)
    keys, off = dev_keys(torch, [gm.lookup_key(b"b", 5), gm.lookup_key(b"f", 5)])
    visible = torch.ones(2, dtype=torch.uint8, device="cuda")
    flags = _dev(torch, np.array([0], dtype=np.int32))

    def call(first=(0, 2), run_flags=flags, bound_offsets=boff, key_offsets=off):
        file, st = db.find_file(b, bound_offsets, _dev(torch, np.array(first, dtype=np.int64)), run_flags, visible, keys,
                                key_offsets)
        return file.cpu().tolist(), st.cpu().tolist()

    assert call() == ([[0], [1]], [0])
    level0 = _dev(torch, np.array([db.RUN_LEVEL0], dtype=np.int32))
    for kw in ({"first": (0, 3)}, {"first": (2, 1)}, {"run_flags": level0},  # past the files, decreasing, LEVEL0 of two
               {"bound_offsets": _dev(torch, np.array([0, 9, 16, 27, 36], dtype=np.int64))},  # a bound of 7 bytes
               {"key_offsets": _dev(torch, np.array([0, 9, 30], dtype=np.int64))}):           # past the keys
        assert call(**kw) == ([[-1], [-1]], [db.MERGE_BAD_INPUT]), kw
    file = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    first = _dev(torch, np.array([0, 2], dtype=np.int64))
    args = [ptr(b), b.numel(), ptr(boff), 2, ptr(first), ptr(flags), ptr(visible), 1, ptr(keys), keys.numel(), ptr(off), 2,
            ptr(file), ptr(st), stream_ptr(torch)]
    lib = _lib.lib()
    assert lib.lsbm_find_file_dev(*args) == 0
    for slot, alias in ((12, boff), (12, first), (12, off), (13, flags), (13, keys)):
        broken = list(args)
        broken[slot] = ptr(alias)
        assert lib.lsbm_find_file_dev(*broken) == ERR_INVALID, slot


# ---------------------------------------------------------------- the callback


def save_inputs(torch, cases):
    """Device inputs of save_value for [(state, found key, value slice, lookup key, window length)]."""
    windows = [bytes(f[:w]) + b"\xcc" * max(0, w - len(f)) for _, f, _, _, w in cases]
    found, foff = dev_keys(torch, windows)
    keys, off = dev_keys(torch, [k for _, _, _, k, _ in cases])
    state = _dev(torch, np.array([s for s, _, _, _, _ in cases], dtype=np.int32))
    key_len = _dev(torch, np.array([len(f) for _, f, _, _, _ in cases], dtype=np.int64))
    value_in = _dev(torch, np.array([v for _, _, v, _, _ in cases], dtype=np.int64).reshape(-1))
    return state, key_len, found, foff, value_in, keys, off


def test_save_value_reproduces_fixture_and_states(torch_cuda, fx):
    from lsbm_amd import db
    torch = torch_cuda
    fixture, _ = fx
    pool = []
    for khex, vhex, uhex, state, _ in fixture["saver"]:
        found, user = bytes.fromhex(khex), bytes.fromhex(uhex)
        # the window holds the whole key; a key under 8 bytes needs none
        pool.append((gm.VALID, found, (1000 + len(pool), len(bytes.fromhex(vhex))), gm.lookup_key(user, 50),
                     len(found) if len(found) >= 8 else 0, state))
    for s in (gm.NOT_VALID, gm.BAD_ENTRY, gm.BAD_CONTENTS, gm.BAD_HANDLE, gm.FILTERED, gm.BAD_CHECKSUM, gm.BAD_TYPE,
              gm.BAD_COMPRESSED):
        want = gm.UNDECIDED if s in (gm.NOT_VALID, gm.FILTERED) else gm.ERROR + s
        pool.append((s, b"", (0, 0), gm.lookup_key(b"user-key", 50), 0, want))
    assert {p[5] for p in pool} >= {0, 1, 2, 3, gm.ERROR + gm.BAD_CHECKSUM}
    for n in SIZES:
        cases = tile(pool, n)
        inputs = save_inputs(torch, [c[:5] for c in cases])
        gv, verdict = guarded(torch, n, torch.int32, 0x7E)
        gw, where = guarded(torch, n, torch.int32, -9)
        gx, value = guarded(torch, 2 * n, torch.int64, -7)
        canary = [q % 4 == 2 for q in range(n)]
        verdict.copy_(_dev(torch, np.array([gm.ERROR + 1 if c else 0 for c in canary], dtype=np.int32)))
        st = db.save_value(*inputs, 3, verdict, value.view(n, 2), where)
        assert st.cpu().tolist() == [0]
        assert guards_intact(gv, n, 0x7E) and guards_intact(gw, n, -9) and guards_intact(gx, 2 * n, -7)
        vh, wh, xh = verdict.cpu().tolist(), where.cpu().tolist(), value.view(n, 2).cpu().tolist()
        for q, (state, found, slice_, key, _, want) in enumerate(cases):
            if canary[q]:
                assert (vh[q], wh[q], xh[q]) == (gm.ERROR + 1, -9, [-7, -7]), q
                continue
            model = gm.save_value(state, found, b"v", key[:-8])[0]
            assert vh[q] == want == model, (n, q)
            if want == gm.UNDECIDED:  # written only for the queries it decides
                assert (wh[q], xh[q]) == (-9, [-7, -7]), q
            else:
                assert wh[q] == 3 and xh[q] == (list(slice_) if want == gm.FOUND else [0, 0]), q


def test_save_value_bad_input_and_aliasing(torch_cuda):
    from lsbm_amd import _lib, db
    torch = torch_cuda
    key = gm.lookup_key(b"user", 9)
    longer = gm.lookup_key(b"user-longer", 4)
    verdict, value, where = db.new_verdicts(2, torch.device("cuda"))

    def run(cases):
        st = db.save_value(*save_inputs(torch, cases), 1, verdict, value, where)
        return st.cpu().tolist(), verdict.cpu().tolist()

    # a valid key of 8 bytes or more that does not fit its window: nothing changes, for any query
    assert run([(gm.VALID, key, (0, 1), key, len(key)), (gm.VALID, longer, (0, 1), key, len(key))]) == \
        ([db.MERGE_BAD_INPUT], [0, 0])
    assert run([(gm.VALID, key, (0, 1), key, len(key)), (99, b"", (0, 0), key, 0)]) == ([db.MERGE_BAD_INPUT], [0, 0])
    assert where.cpu().tolist() == [-1, -1] and not value.cpu().numpy().any()
    # the same keys with windows of their true lengths
    assert run([(gm.VALID, key, (0, 1), key, len(key)), (gm.VALID, longer, (0, 1), key, len(longer))]) == \
        ([0], [gm.FOUND, gm.UNDECIDED])
    inputs = save_inputs(torch, [(gm.VALID, key, (0, 1), key, len(key))] * 2)
    state, key_len, found, foff, value_in, keys, off = inputs
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = [ptr(state), ptr(key_len), ptr(found), found.numel(), ptr(foff), ptr(value_in), ptr(keys), keys.numel(),
            ptr(off), 2, 0, ptr(verdict), ptr(value), ptr(where), ptr(st), stream_ptr(torch)]
    lib = _lib.lib()
    verdict.zero_()
    assert lib.lsbm_save_value_dev(*args) == 0
    for slot, alias in ((11, state), (12, value_in), (13, key_len), (14, foff), (12, found)):
        broken = list(args)
        broken[slot] = ptr(alias)
        assert lib.lsbm_save_value_dev(*broken) == ERR_INVALID, slot


# ---------------------------------------------------------------- the values


def test_slices_gather_ranges_sizes_and_guards(torch_cuda):
    from lsbm_amd import _lib, db
    torch = torch_cuda
    rng = random.Random(0x6A7)
    image_h = bytes(rng.randrange(256) for _ in range(5000))
    image = _dev(torch, np.frombuffer(image_h, dtype=np.uint8))
    for n in SIZES:
        lens = [rng.choice((0, 1, 15, 16, 17, 100, 300)) for _ in range(n)]
        at = [rng.randrange(0, 5000 - ln + 1) for ln in lens]
        where_h = [rng.randrange(-1, 4) for _ in range(n)]
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        total = int(off[-1])
        go, out = guarded(torch, total, torch.uint8, GUARD, 64)
        slices = _dev(torch, np.array([x for p in zip(at, lens) for x in p], dtype=np.int64))
        where = _dev(torch, np.array(where_h, dtype=np.int32))
        st = db.slices_gather(image, slices, where, 1, 3, out, _dev(torch, off))
        assert st.cpu().tolist() == [0] and guards_intact(go, total, GUARD, 64)
        got = out.cpu().numpy().tobytes()
        for q in range(n):
            want = image_h[at[q]:at[q] + lens[q]] if 1 <= where_h[q] < 3 else bytes([GUARD]) * lens[q]
            assert got[off[q]:off[q + 1]] == want, (n, q)
    # a slice past the image, a slice longer than its window: not copied, the others are
    slices = _dev(torch, np.array([4990, 11, 0, 5, 10, 4], dtype=np.int64))
    where = torch.zeros(3, dtype=torch.int32, device="cuda")
    out = torch.full((12,), GUARD, dtype=torch.uint8, device="cuda")
    st = db.slices_gather(image, slices, where, 0, 1, out, _dev(torch, np.array([0, 4, 8, 12], dtype=np.int64)))
    assert st.cpu().tolist() == [db.MERGE_BAD_INPUT]
    assert out.cpu().numpy().tobytes() == bytes([GUARD]) * 8 + image_h[10:14]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    off = _dev(torch, np.array([0, 4, 8, 12], dtype=np.int64))
    lib = _lib.lib()
    assert lib.lsbm_slices_gather_dev(ptr(image), 5000, ptr(slices), ptr(where), 0, 1, ptr(image[100:]), 12, ptr(off), 3,
                                      ptr(st), stream_ptr(torch)) == ERR_INVALID
    assert lib.lsbm_slices_gather_dev(ptr(image), 5000, ptr(slices), ptr(where), 0, 1, ptr(out), 12, ptr(off), 3,
                                      ptr(off), stream_ptr(torch)) == ERR_INVALID


# ---------------------------------------------------------------- a version


def open_device_version(torch, v, blob):
    from lsbm_amd import db
    bits = 10 if v["filter_policy"] else None
    files = [db.TableFile(blob[f["file"][0]:f["file"][0] + f["file"][1]], f["number"], bits,
                          bytes.fromhex(f["smallest"]), bytes.fromhex(f["largest"])) for f in v["files"]]
    version = db.Version(files, [db.Run(idx, flags) for flags, idx in v["runs"]])
    version.visible.copy_(_dev(torch, np.array([f["visible"] for f in v["files"]], dtype=np.uint8)))
    return version


def test_version_get_reproduces_fixture(torch_cuda, fx):
    from lsbm_amd import db
    torch = torch_cuda
    fixture, blob = fx
    for v in fixture["versions"]:
        version = open_device_version(torch, v, blob)
        mems = [dev_memtable(torch, memtable_of(m)) for m in v["memtables"]]
        users = [bytes.fromhex(u) for u, _ in v["queries"]]
        uk, uoff = dev_keys(torch, users)
        seqs = _dev(torch, np.array([s for _, s in v["queries"]], dtype=np.int64))
        r = version.get(uk, uoff, seqs, mems, verify=bool(v["verify"]))
        status, where, values = r.status.cpu().tolist(), r.where.cpu().tolist(), values_of(r)
        for q, want in enumerate(v["results"]):
            what = (v["name"], users[q], v["queries"][q][1])
            assert db.status_string(status[q], users[q]) == want["status"], what
            assert values[q].hex() == want["value"], what
            assert where[q] == want["where"], what


def test_version_for_levels_equals_the_fixture_tree(torch_cuda, fx):
    """for_levels builds the probe list the fixture's driver walked, and reads
    smallest / largest from the files themselves."""
    from lsbm_amd import db
    torch = torch_cuda
    fixture, blob = fx
    v = next(v for v in fixture["versions"] if v["name"] == "tree")
    by = {f["name"]: db.TableFile(blob[f["file"][0]:f["file"][0] + f["file"][1]], f["number"], 10) for f in v["files"]}
    version = db.Version.for_levels([by["l0_old"], by["l0_mid"], by["l0_new"]], [],
                                    [([by["l1_a"], by["l1_b"]], []), ([], [by["l2_a"], by["l2_b"], by["l2_c"]])])
    assert [(r.flags, [version.files[f].number for f in r.files]) for r in version.runs] == \
        [(flags, [v["files"][f]["number"] for f in idx]) for flags, idx in v["runs"]]
    assert version.smallest == [bytes.fromhex(f["smallest"]) for f in v["files"]]
    assert version.largest == [bytes.fromhex(f["largest"]) for f in v["files"]]
    mems = [dev_memtable(torch, memtable_of(m)) for m in v["memtables"]]
    users = [bytes.fromhex(u) for u, _ in v["queries"]]
    uk, uoff = dev_keys(torch, users)
    r = version.get(uk, uoff, _dev(torch, np.array([s for _, s in v["queries"]], dtype=np.int64)), mems)
    assert [db.status_string(s, u) for s, u in zip(r.status.cpu().tolist(), users)] == [w["status"] for w in v["results"]]
    assert [x.hex() for x in values_of(r)] == [w["value"] for w in v["results"]]
    # no query, and one query
    at = next(q for q, (_, seq) in enumerate(v["queries"]) if seq == 9999)
    for qs in ([], [users[at]]):
        uk1, uoff1 = dev_keys(torch, qs)
        r1 = version.get(uk1, uoff1, 9999, mems)
        assert [db.status_string(s, users[at]) for s in r1.status.cpu().tolist()] == \
            [v["results"][at]["status"]] * len(qs)
        assert [x.hex() for x in values_of(r1)] == [v["results"][at]["value"]] * len(qs)


def test_version_rejects_a_file_that_does_not_open(torch_cuda, fx):
    from lsbm_amd import db
    fixture, blob = fx
    f = fixture["versions"][0]["files"][0]
    data = bytes(blob[f["file"][0]:f["file"][0] + f["file"][1]])
    for broken in (data[:40], data[:-1] + b"\0", data[:-48] + b"\xff" * 40 + data[-8:]):
        with pytest.raises(ValueError):
            db.Version([db.TableFile(broken, 7, 10)], [db.Run([0])])


def test_round_trip_flush_compact_get(torch_cuda, snappy_oracle):
    """Two logs flushed by memtable.flush, compacted into a level by
    sstable.compact, a third log as the memtable: Version.get over the
    project's own writers equals the model over the same inputs."""
    from lsbm_amd import db, memtable, sstable
    from lsbm_amd.table import kSnappyCompression
    torch = torch_cuda
    rng = random.Random(0x7217)
    uncompress = codec(snappy_oracle)
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
        """The records of a log side by side: (bytes, [(offset, length)], image, records)."""
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
    # the third log is the memtable
    buf, pairs, image, records = on_device(logs[2])
    e = memtable.entries(image, records)
    mem = db.MemTable(e.keys, e.key_offsets, e.values, image)
    mem_model = mt.entries(buf, pairs)[0]
    # the model over the same files
    tables = [gm.open_table(bytes(f.data), 10, uncompress) for f in version.files]
    bounds = list(zip(version.smallest, version.largest))
    runs = [(list(r.files), r.flags) for r in version.runs]
    assert bounds[0] == (models[1][0][0], models[1][-1][0])
    queries = [(u, s) for u in users[::3] + [b"", b"key", b"key9999"] for s in (30, seq // 2, seq + 5)]
    uk, uoff = dev_keys(torch, [u for u, _ in queries])
    r = version.get(uk, uoff, _dev(torch, np.array([s for _, s in queries], dtype=np.int64)), [mem])
    status, where, values = r.status.cpu().tolist(), r.where.cpu().tolist(), values_of(r)
    seen = set()
    for q, (u, s) in enumerate(queries):
        verdict, value, src = gm.version_get([mem_model], tables, bounds, runs, u, s, uncompress)
        assert (status[q], values[q], where[q]) == (verdict, value or b"", src), (u, s)
        seen.add((verdict, src))
    assert {w for _, w in seen} >= {-1, 0, 1, 3} and {v for v, _ in seen} >= {gm.UNDECIDED, gm.FOUND, gm.DELETED}
