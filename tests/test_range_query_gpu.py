"""LSbM's range query on the GPU (include/lsbm_range.h, lsbm_amd/rangequery.py):
the whole query against the reference's fixture (tests/golden/range_fixture.json,
range_tables.bin), the plan's two calls and the count alone against the
plain-Python model (tests/golden/rangemodel.py, pinned to that fixture by
tests/test_range_query.py).
"""
import random

import numpy as np
import pytest

from golden import range_cases as rc
from golden import rangemodel as rgm
from test_db_get_gpu import _dev, dev_keys, guarded, guards_intact, ptr, stream_ptr

pytestmark = pytest.mark.gpu

OK, NO_ROOM, BAD_INPUT = 0, 1, 2


@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


def run_query(torch, rq, queries):
    """RangeQuery.query of [(start, end, snapshot)] as host lists:
    (found, checked, total, per query [(file number, count, flags)])."""
    sk, so = dev_keys(torch, [a for a, _, _ in queries])
    ek, eo = dev_keys(torch, [b for _, b, _ in queries])
    snap = _dev(torch, np.array([s for _, _, s in queries], dtype=np.int64))
    r = rq.query(sk, so, ek, eo, snap)
    first = r.pair_first.cpu().tolist()
    numbers = rq.numbers[r.pair_file.to(torch.int64)].cpu().tolist()
    pairs = list(zip(numbers, r.pair_count.cpu().tolist(), r.pair_flags.cpu().tolist()))
    assert r.status.cpu().tolist() == [OK] and len(pairs) == first[-1]
    return (r.found.cpu().tolist(), r.checked.cpu().tolist(), r.total.cpu().tolist(),
            [pairs[first[q]:first[q + 1]] for q in range(len(queries))])


# ---------------------------------------------------------------- the fixture


def test_every_fixture_run(torch_cuda, fx):
    """Every run of the reference's fixture through from_manifest: the files
    read, in order and by number, each file's count, found and checked."""
    from lsbm_amd import buffered, rangequery
    torch = torch_cuda
    _, body = fx
    seen_flags = set()
    for name, case in body["cases"].items():
        files = rc.case_files(body, case)
        numbers = sorted(files)
        image = _dev(torch, np.frombuffer(bytes.fromhex(case["manifest"]), dtype=np.uint8))
        bv = buffered.BufferedVersion.from_manifest(image, files, case["compaction_buffer_length"],
                                                    bits_per_key=rc.BITS)
        assert {"%d,%d" % k: [[e[0] for e in t] for t in ts] for k, ts in bv.tables.items()} == case["lists"], name
        rq = rangequery.RangeQuery(bv)
        queries = rc.case_queries(case)
        for r, run in enumerate(case["runs"]):
            p = rc.run_params(run)
            bv.configure(p.use_length, p.buffered_merge, p.read_cursor_keys)
            rq.configure(read_upto_key=p.read_upto_key)
            found, checked, total, pairs = run_query(torch, rq, queries)
            for q, (want_found, want_read) in enumerate(run["results"]):
                what = (name, r, q)
                assert [n for n, _, _ in pairs[q]] == want_read, what
                assert [c for _, c, _ in pairs[q]] == [case["file_counts"][q][numbers.index(n)] for n in want_read], what
                assert found[q] == want_found and checked[q] == len(want_read), what
                assert total[q] == sum(c for _, c, _ in pairs[q]), what
                for n, c, flags in pairs[q]:
                    assert bool(flags & rangequery.RANGE_NO_ENTRIES) == (n in case["damaged"]), what
                    seen_flags.add(flags & 3)
    assert seen_flags == {0, 1, 2, 3}


# ---------------------------------------------------------------- the plan alone


class PlanInput:
    """The device tensors of one plan call over a tree of file metadata."""

    def __init__(self, torch, lists, p, queries):
        from lsbm_amd import rangequery
        self.slots = rangequery.layout_range_slots(rgm.structure_of(lists), p.use_length, p.buffered_merge)
        self.p, self.queries = p, queries
        first, bounds = [0], []
        for s in self.slots:
            for e in s.files:
                bounds += [e[2], e[3]]
            first.append(len(bounds) // 2)
        self.info = _dev(torch, np.array([s.kind | s.level << 8 | s.flags << 16 for s in self.slots], dtype=np.int32))
        self.first = _dev(torch, np.array(first, dtype=np.int64))
        self.bounds, self.boff = dev_keys(torch, bounds)
        self.use = _dev(torch, np.array(p.use_length, dtype=np.int32))
        self.wb = _dev(torch, np.array(rgm.wb_enabled(p), dtype=np.int32))
        self.cursors = list(p.read_cursor_keys) + [p.read_upto_key]
        self.ckeys, self.coff = dev_keys(torch, self.cursors)
        self.skeys, self.soff = dev_keys(torch, [rgm.lookup_key(a, 77) for a, _ in queries])
        self.ekeys, self.eoff = dev_keys(torch, [rgm.lookup_key(b, 77) for _, b in queries])
        self.run_base = first

    def inputs(self):
        return (self.info, self.first, self.bounds, self.boff, self.use, self.wb, self.ckeys, self.coff, self.skeys,
                self.soff, self.ekeys, self.eoff)

    def model(self):
        """Per query [(run entry, flag word)]."""
        out = []
        for a, b in self.queries:
            pairs = rgm.rule_plan(self.slots, self.p.use_length, rgm.wb_enabled(self.p), self.cursors, a, b)
            out.append([(self.run_base[s] + i, flags) for s, i, flags in pairs])
        return out


def run_plan(torch, x, n):
    """(counts, per query [(run entry, flag word)], checked) through both calls, the cap exact."""
    from lsbm_amd import rangequery
    whole_c, count = guarded(torch, n, torch.int32, -7)
    _, st = rangequery.range_plan(*x.inputs(), count=count)
    assert st.cpu().tolist() == [OK] and guards_intact(whole_c, n, -7)
    counts = count.cpu().tolist()
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(first[-1])
    whole_r, run = guarded(torch, total, torch.int32, -7)
    whole_f, flags = guarded(torch, total, torch.int32, -7)
    whole_k, checked = guarded(torch, n, torch.int32, -7)
    st = rangequery.range_emit(*x.inputs(), _dev(torch, first), run, flags, checked, total)
    assert st.cpu().tolist() == [OK]
    assert guards_intact(whole_r, total, -7) and guards_intact(whole_f, total, -7) and guards_intact(whole_k, n, -7)
    pairs = list(zip(run.cpu().tolist(), flags.cpu().tolist()))
    return counts, [pairs[first[q]:first[q + 1]] for q in range(n)], checked.cpu().tolist()


@pytest.mark.parametrize("n", [0, 1, 65, 300])
def test_plan_and_emit_on_random_trees(torch_cuda, n):
    torch = torch_cuda
    rng = random.Random(3000 + n)
    seen = 0
    for _ in range(4):
        lists, p = rc.random_tree(rng)
        x = PlanInput(torch, lists, p, rc.random_queries(rng, n))
        want = x.model()
        counts, pairs, checked = run_plan(torch, x, n)
        assert counts == [len(w) for w in want] == checked
        assert pairs == want
        seen += sum(counts)
    assert seen > 0 or n <= 1


def good_plan_input(torch, n=70):
    rng = random.Random(11)
    while True:
        lists, p = rc.random_tree(rng)
        x = PlanInput(torch, lists, p, rc.random_queries(rng, n))
        if sum(len(w) for w in x.model()) > 100 and len(x.slots) >= 10:
            return x


def test_bad_input_leaves_the_outputs(torch_cuda):
    from lsbm_amd import _lib, rangequery
    torch = torch_cuda
    n = 70
    x0 = good_plan_input(torch, n)
    kinds = [(s.level, s.kind, s.flags) for s in x0.slots]
    info = lambda ks: _dev(torch, np.array([k | level << 8 | flags << 16 for level, k, flags in ks], dtype=np.int32))
    at = lambda level, kind: next(i for i, k in enumerate(kinds) if k[:2] == (level, kind))

    def bad_cases():
        x = good_plan_input(torch, n)
        i = at(2, rgm.RSLOT_DEL)
        x.info = info(kinds[:i] + [(2, 6, 0)] + kinds[i + 1:])
        yield "an unknown kind", x
        x = good_plan_input(torch, n)
        x.info = info(kinds[:-1] + [(4, rgm.RSLOT_INS, 0)])
        yield "a level above 3", x
        x = good_plan_input(torch, n)
        x.info = info(kinds[:-1] + [(3, rgm.RSLOT_INS, 4)])
        yield "an unknown flag", x
        x = good_plan_input(torch, n)
        x.info = info([(0, rgm.RSLOT_DEL, 0)] + kinds[1:])
        yield "a level-0 slot of another kind", x
        x = good_plan_input(torch, n)
        i, j = at(1, rgm.RSLOT_DEL), at(1, rgm.RSLOT_INS)
        swapped = list(kinds)
        swapped[i], swapped[j] = swapped[j], swapped[i]
        x.info = info(swapped)
        yield "kinds out of order in a level", x
        x = good_plan_input(torch, n)
        i = at(3, rgm.RSLOT_INS)
        x.info = info(kinds[:i] + [(3, rgm.RSLOT_DEL, 0)] + kinds[i + 1:])
        yield "two DEL slots in a level", x
        x = good_plan_input(torch, n)
        x.first = x.first.clone()
        x.first[3] += 100
        yield "a run list that decreases", x
        x = good_plan_input(torch, n)
        x.first = x.first.clone()
        x.first[-1] -= 1
        yield "a run list that does not end at n_runs", x
        x = good_plan_input(torch, n)
        x.boff = x.boff.clone()
        x.boff[5] = x.boff[4] + 7
        yield "a bound under 8 bytes", x
        x = good_plan_input(torch, n)
        x.boff = x.boff.clone()
        x.boff[-1] += 1
        yield "a bound offset past the buffer", x
        x = good_plan_input(torch, n)
        x.coff = _dev(torch, np.array([0, 0, 5, 1, 5, 5], dtype=np.int64))
        yield "a cursor offset that decreases", x
        x = good_plan_input(torch, n)
        x.coff = x.coff.clone()
        x.coff[5] += 1
        yield "a cursor offset past its buffer", x
        x = good_plan_input(torch, n)
        x.soff = x.soff.clone()
        x.soff[7] += 9
        yield "a start user key under 8 bytes", x
        x = good_plan_input(torch, n)
        x.skeys, x.soff = dev_keys(torch, [rgm.lookup_key(b"k" * 7, 77)] * n)
        yield "every start user key of 7 bytes", x
        x = good_plan_input(torch, n)
        x.ekeys, x.eoff = dev_keys(torch, [rgm.lookup_key(b"k" * 8, 77)] * (n - 1) + [b"k" * 15])
        yield "an end lookup key under 16 bytes", x
        x = good_plan_input(torch, n)
        x.eoff = x.eoff.clone()
        x.eoff[n] += 1
        yield "an end offset past the buffer", x

    n_cases = 0
    for what, x in bad_cases():
        whole, view = guarded(torch, n, torch.int32, -7)
        _, st = rangequery.range_plan(*x.inputs(), count=view)
        assert st.cpu().tolist() == [BAD_INPUT], what
        assert set(whole.cpu().tolist()) == {-7}, what
        first = _dev(torch, np.arange(n + 1, dtype=np.int64))
        outs = [guarded(torch, n, torch.int32, -7) for _ in range(3)]
        st = rangequery.range_emit(*x.inputs(), first, outs[0][1], outs[1][1], outs[2][1], n)
        assert st.cpu().tolist() == [BAD_INPUT], what
        assert all(set(whole.cpu().tolist()) == {-7} for whole, _ in outs), what
        n_cases += 1
    assert n_cases == 16
    # emit alone: pair_first that does not step by the counts, or decreases; a cap one short
    x = x0
    count, _ = rangequery.range_plan(*x.inputs())
    first = np.concatenate([[0], np.cumsum(count.cpu().tolist())]).astype(np.int64)
    total = int(first[-1])
    for q, delta, cap, want in ((3, 1, total + 4, BAD_INPUT), (9, -1, total + 4, BAD_INPUT),
                                (n, 2, total + 4, BAD_INPUT), (0, 0, total - 1, NO_ROOM), (0, 0, total, OK)):
        wrong = first.copy()
        wrong[q] += delta
        outs = [guarded(torch, total + 4, torch.int32, -7) for _ in range(2)] + [guarded(torch, n, torch.int32, -7)]
        st = rangequery.range_emit(*x.inputs(), _dev(torch, wrong), outs[0][1], outs[1][1], outs[2][1], cap)
        assert st.cpu().tolist() == [want], (q, delta, cap)
        if want != OK:
            assert all(set(whole.cpu().tolist()) == {-7} for whole, _ in outs), (q, delta, cap)
        else:
            assert -7 not in outs[0][1][:total].cpu().tolist() and guards_intact(outs[0][0], total + 4, -7)
    # an output that overlaps an input is refused before anything is enqueued
    args = [ptr(x.info), x.info.numel(), ptr(x.first), x.boff.numel() // 2, ptr(x.bounds), x.bounds.numel(),
            ptr(x.boff), ptr(x.use), ptr(x.wb), ptr(x.ckeys), x.ckeys.numel(), ptr(x.coff), ptr(x.skeys),
            x.skeys.numel(), ptr(x.soff), ptr(x.ekeys), x.ekeys.numel(), ptr(x.eoff), n]
    assert _lib.lib().lsbm_range_plan_dev(*args, ptr(x.soff), ptr(x.wb), stream_ptr(torch)) == -1


# ---------------------------------------------------------------- the count alone


def synthetic_index(torch, files, base=0, arena=None):
    """A RangeIndex of [[internal key]] per file (None: a file without entries, state 1)."""
    from lsbm_amd import rangequery
    keys = [k for f in files if f for k in f]
    blob, off = dev_keys(torch, keys)
    first = np.concatenate([[0], np.cumsum([len(f) if f else 0 for f in files])]).astype(np.int64)
    state = np.array([int(f is None) for f in files], dtype=np.int32)
    if arena is not None:
        arena[base:base + blob.numel()] = blob
        blob = arena
    return rangequery.RangeIndex(blob, off + base, _dev(torch, first), _dev(torch, state))


def count_on(torch, index, files, pairs, guard=True):
    """range_count of [(start, end, snapshot, file, flags)], one query per pair:
    (counts, errors, found, total), with guards round every output."""
    from lsbm_amd import rangequery
    n = len(pairs)
    sk, so = dev_keys(torch, [rgm.lookup_key(a, s) for a, _, s, _, _ in pairs])
    ek, eo = dev_keys(torch, [rgm.lookup_key(b, s) for _, b, s, _, _ in pairs])
    first = _dev(torch, np.arange(n + 1, dtype=np.int64))
    pf = _dev(torch, np.array([f for _, _, _, f, _ in pairs], dtype=np.int32))
    fl = _dev(torch, np.array([g for _, _, _, _, g in pairs], dtype=np.int32))
    outs = [guarded(torch, n, dt, -7) for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
    *_, st = rangequery.range_count(index, sk, so, ek, eo, first, pf, fl, *[view for _, view in outs])
    assert st.cpu().tolist() == [OK]
    assert all(guards_intact(whole, n, -7) for whole, _ in outs)
    return [view.cpu().tolist() for _, view in outs]


def model_count(keys, start, end, snapshot):
    return rgm.get_range(None if keys is None else [(keys[-1], keys)] if keys else [], rgm.lookup_key(start, snapshot),
                         rgm.lookup_key(end, snapshot))


def count_files():
    u = lambda i: b"key%05d" % i
    ik = lambda i, s=10: rc.ikey(u(i), s)
    return [[ik(i) for i in range(200)], [ik(7)], None, [ik(i) for i in range(64)],
            [ik(i, s) for i in range(3) for s in (512, 256, 255, 1)], []]


def count_pairs():
    u = lambda i: b"key%05d" % i
    pairs = []
    for lo in (0, 1, 70, 199):  # lower bounds at entry 0, inside and at the last entry
        for span in (0, 1, 63, 64, 65, 128, 129, 130, 500):  # stops at lanes 0, 63, 64, and none within 129 entries
            pairs.append((u(lo), u(lo + span - 1) if span else u(lo)[:7] + b"\x00", 1000, 0, span % 2))
    pairs += [(u(0), u(300), 1000, 0, 1), (u(200), u(300), 1000, 0, 0), (u(199) + b"\x00", u(300), 1000, 0, 1)]
    pairs += [(u(7), u(7), 1000, 1, 1), (u(8), u(9), 1000, 1, 0), (u(0), u(9), 1000, 1, 1)]
    pairs += [(u(0), u(9), 1000, 2, 1), (u(0), u(9), 1000, 5, 1)]  # a file without entries; an empty file
    pairs += [(u(0), u(63), 1000, 3, 1), (u(63), u(63), 1000, 3, 0), (u(0), u(62), 1000, 3, 1)]
    pairs += [(u(0), u(1), s, 4, 1) for s in (1000, 512, 256, 255, 1, 0)]
    return pairs


def test_count_on_a_synthetic_index(torch_cuda):
    torch = torch_cuda
    files, pairs = count_files(), count_pairs()
    counts, errors, found, total = count_on(torch, synthetic_index(torch, files), files, pairs)
    want = [model_count(files[f], a, b, s) for a, b, s, f, _ in pairs]
    assert counts == want and total == want
    assert found == [w if g & 1 else 0 for w, (_, _, _, _, g) in zip(want, pairs)]
    assert errors == [int(files[f] is None) for _, _, _, f, _ in pairs]
    assert {0, 1, 63, 64, 65, 128, 129, 130, 200} <= set(want)
    # one query with many pairs: found sums the flagged ones only
    from lsbm_amd import rangequery
    sk, so = dev_keys(torch, [rgm.lookup_key(b"key00000", 1000)])
    ek, eo = dev_keys(torch, [rgm.lookup_key(b"key00009", 1000)])
    pf = _dev(torch, np.array([0, 1, 2, 3, 4, 5, 0], dtype=np.int32))
    fl = _dev(torch, np.array([0, 1, 1, 0, 1 | 2 << 8, 0, 1], dtype=np.int32))
    c, e, f, t, st = rangequery.range_count(synthetic_index(torch, files), sk, so, ek, eo,
                                            _dev(torch, np.array([0, 7], dtype=np.int64)), pf, fl)
    assert st.cpu().tolist() == [OK] and c.cpu().tolist() == [10, 1, 0, 10, 12, 0, 10]
    assert f.cpu().tolist() == [1 + 0 + 12 + 10] and t.cpu().tolist() == [43] and e.cpu().tolist() == [0, 0, 1, 0, 0, 0, 0]


def test_count_bad_input_leaves_the_outputs(torch_cuda):
    from lsbm_amd import rangequery
    torch = torch_cuda
    files = count_files()
    pairs = count_pairs()[:20]
    n = len(pairs)
    sk, so = dev_keys(torch, [rgm.lookup_key(a, s) for a, _, s, _, _ in pairs])
    ek, eo = dev_keys(torch, [rgm.lookup_key(b, s) for _, b, s, _, _ in pairs])
    first = _dev(torch, np.arange(n + 1, dtype=np.int64))
    pf = _dev(torch, np.array([f for _, _, _, f, _ in pairs], dtype=np.int32))
    fl = _dev(torch, np.zeros(n, dtype=np.int32))
    good = synthetic_index(torch, files)

    def bad_cases():
        off = good.key_offsets.clone()
        off[9] = off[8] + 7
        yield "an index key under 8 bytes", good._replace(key_offsets=off), first, pf, so
        off = good.key_offsets.clone()
        off[-1] += 1
        yield "an index offset past the arena", good._replace(key_offsets=off), first, pf, so
        ff = good.file_first_entry.clone()
        ff[2] = ff[1] - 1
        yield "file_first_entry that decreases", good._replace(file_first_entry=ff), first, pf, so
        ff = good.file_first_entry.clone()
        ff[-1] += 1
        yield "file_first_entry past the entries", good._replace(file_first_entry=ff), first, pf, so
        wrong = first.clone()
        wrong[3] = wrong[4] + 1
        yield "pair_first that decreases", good, wrong, pf, so
        wrong = first.clone()
        wrong[-1] += 1
        yield "pair_first that does not end at n_pairs", good, wrong, pf, so
        wrong = pf.clone()
        wrong[5] = len(files)
        yield "a pair's file that is not there", good, first, wrong, so
        wrong = so.clone()
        wrong[4] += 9
        yield "a start lookup key under 16 bytes", good, first, pf, wrong

    n_cases = 0
    for what, index, pfirst, pfile, soff in bad_cases():
        outs = [guarded(torch, n, dt, -7) for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
        *_, st = rangequery.range_count(index, sk, soff, ek, eo, pfirst, pfile, fl, *[view for _, view in outs])
        assert st.cpu().tolist() == [BAD_INPUT], what
        assert all(set(whole.cpu().tolist()) == {-7} for whole, _ in outs), what
        n_cases += 1
    assert n_cases == 8


def test_n_0_and_a_short_start_key(torch_cuda, fx):
    from lsbm_amd import buffered, rangequery
    torch = torch_cuda
    _, body = fx
    case = body["cases"]["counts"]
    files = rc.case_files(body, case)
    image = _dev(torch, np.frombuffer(bytes.fromhex(case["manifest"]), dtype=np.uint8))
    bv = buffered.BufferedVersion.from_manifest(image, files, case["compaction_buffer_length"], bits_per_key=rc.BITS)
    rq = rangequery.RangeQuery(bv)
    found, checked, total, pairs = run_query(torch, rq, [])
    assert found == [] and checked == [] and total == [] and pairs == []
    with pytest.raises(ValueError, match="bad input"):
        run_query(torch, rq, [(b"aaaaa000", b"aaaaa009", 5), (b"short", b"zz", 5)])


# ---------------------------------------------------------------- placement, stream, host reads


def test_index_keys_past_4gib(torch_cuda):
    """One tiny file's keys placed past 4 GiB in an arena that nothing fills,
    a decoy of the same layout 2^32 below: the answers of the same file at
    offset 0."""
    torch = torch_cuda
    files = [count_files()[0][:150]]
    decoy = [[rc.ikey(b"kez%05d" % i, 10) for i in range(150)]]
    pairs = [p for p in count_pairs() if p[3] == 0][:24]
    low = count_on(torch, synthetic_index(torch, files), files, pairs)
    arena = torch.empty((1 << 32) + (1 << 20), dtype=torch.uint8, device="cuda")
    base = (1 << 32) + 4099
    synthetic_index(torch, decoy, base - (1 << 32), arena)
    index = synthetic_index(torch, files, base, arena)
    assert int(index.key_offsets.min().cpu()) > 1 << 32
    high = count_on(torch, index, files, pairs)
    assert high == low and low[0] == [model_count(files[0], a, b, s) for a, b, s, _, _ in pairs]
    assert len(set(low[0])) > 5


def small_tree(torch, fx):
    from lsbm_amd import buffered, rangequery
    _, body = fx
    case = body["cases"]["gates"]
    files = rc.case_files(body, case)
    image = _dev(torch, np.frombuffer(bytes.fromhex(case["manifest"]), dtype=np.uint8))
    bv = buffered.BufferedVersion.from_manifest(image, files, case["compaction_buffer_length"], bits_per_key=rc.BITS)
    p = rc.run_params(case["runs"][3])
    bv.configure(p.use_length, p.buffered_merge, p.read_cursor_keys)
    return rangequery.RangeQuery(bv, p.read_upto_key), rc.case_queries(case), case["runs"][3]["results"]


def test_the_whole_query_on_a_side_stream(torch_cuda, fx):
    torch = torch_cuda
    rq, queries, want = small_tree(torch, fx)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = run_query(torch, rq, queries)  # (the range index is built on the side stream too)
    side.synchronize()
    rq2, _, _ = small_tree(torch, fx)
    assert run_query(torch, rq2, queries) == on_side
    assert on_side[0] == [w[0] for w in want] and [[n for n, _, _ in ps] for ps in on_side[3]] == [w[1] for w in want]


def test_host_reads_do_not_grow_with_the_sorted_tables(torch_cuda, monkeypatch):
    """The same queries over trees whose compaction-buffer lists hold 2, 8 and
    20 tables: as many .cpu() / .item() / .tolist() calls in each, once the
    range index is built."""
    from golden import memtablemodel
    from lsbm_amd import buffered, rangequery
    torch = torch_cuda
    counts = {}

    def counted(name):
        real = getattr(torch.Tensor, name)

        def call(self, *a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return real(self, *a, **kw)
        return call

    users = [rc.user(i) for i in range(40)]
    sk, so = dev_keys(torch, [users[i] for i in range(0, 40, 3)] * 5)
    ek, eo = dev_keys(torch, [users[min(i + 6, 39)] for i in range(0, 40, 3)] * 5)
    reads, checked = [], []
    for n_tables in (2, 8, 20):
        files, tables, number = {}, {}, 1000 * n_tables

        def add(keys):
            nonlocal number
            number += 1
            kv = [(rc.ikey(u, 50), b"v") for u in sorted(set(keys))]
            files[number] = memtablemodel.table_file(kv, 256, 4, rc.BITS)
            return (number, len(files[number]), kv[0][0], kv[-1][0])

        for level in (2, 3):
            tables[(level, 2)] = [[]] + [[add(users[t::n_tables] + users[:1] + users[-1:])] for t in range(n_tables)]
            tables[(level, 1)] = [[add(users)]]
        bv = buffered.BufferedVersion(tables, files, (0, 0, 25, 25), True, bits_per_key=rc.BITS)
        rq = rangequery.RangeQuery(bv, b"zz")
        r = rq.query(sk, so, ek, eo, 100)  # (builds the range index)
        checked.append(int(r.checked.max().cpu()))
        with monkeypatch.context() as m:
            counts.clear()
            for name in ("cpu", "item", "tolist"):
                m.setattr(torch.Tensor, name, counted(name))
            rq.query(sk, so, ek, eo, 100)
            reads.append(dict(counts))
    assert checked == [4, 16, 40]  # every table of the two compaction buffers is read
    assert reads[0] == reads[1] == reads[2] and 0 < sum(reads[0].values()) <= 4, reads
