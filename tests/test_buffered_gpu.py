"""LSbM's buffered Get on the GPU (include/lsbm_probe.h, lsbm_amd/buffered.py):
the probe plan's two calls alone, and the whole chain, exact against the
reference's fixture (tests/golden/buffered_fixture.json, buffered_tables.bin) and
the plain-Python model (tests/golden/buffermodel.py, pinned to that fixture by
tests/test_buffered.py).
"""
import random

import numpy as np
import pytest

from golden import buffered_cases as bc
from golden import buffermodel as bfm
from golden import getmodel as gm
from golden import memtablemodel
from test_db_get_gpu import _dev, dev_keys, guarded, guards_intact, ptr, stream_ptr, values_of

pytestmark = pytest.mark.gpu

OK, NO_ROOM, BAD_INPUT = 0, 1, 2


@pytest.fixture(scope="module")
def fx():
    return bc.load_fixture()


@pytest.fixture(scope="module")
def random_pool():
    files = bc.pool()
    return files, {f[0]: gm.open_table(f[2], bc.BITS, None, False) for f in files}


def structure_of(lists):
    return {k: [[(f.number, f.file_size, f.smallest, f.largest) for f in t] for t in ts] for k, ts in lists.items()}


def visible_of(bv, lists):
    """FileMeta.visible in the order of BufferedVersion.entries."""
    return [int(f.visible) for level in range(4) for kind in range(4) for t in lists.get((level, kind), []) for f in t]


def gpu_get(torch, bv, queries, memtables=(), verify=True):
    uk, uoff = dev_keys(torch, [u for u, _ in queries])
    snap = _dev(torch, np.array([s for _, s in queries], dtype=np.int64))
    r = bv.get(uk, uoff, snap, memtables, verify)
    return r.status.cpu().tolist(), values_of(r), r.where.cpu().tolist()


def same_as_model(torch, bv, v, tables, p, queries, verify=True, what=None):
    """bv.get against the rule model: status_string, values and where all
    equal.  Returns the model's reads per query; the GPU's (status, values,
    where) stay in same_as_model.last."""
    from lsbm_amd import db
    layout, memo = bfm.slots(v, p), {}
    assert [(s.level, s.kind, [e[0] for e in s.files]) for s in bv.slots] == \
        [(level, kind, [f.number for f in fs]) for level, kind, fs, _ in layout], what
    status, values, where = gpu_get(torch, bv, queries, verify=verify)
    reads = []
    for q, (key, seq) in enumerate(queries):
        want = bfm.rule_get(v, tables, p, key, seq, verify=verify, layout=layout, memo=memo)
        assert db.status_string(status[q], key) == gm.status_string(want[0], key), (what, key, seq)
        assert values[q] == (want[1] or b""), (what, key, seq)
        assert where[q] == want[3], (what, key, seq)
        reads.append(want[4])
    same_as_model.last = (status, values, where)
    return reads


# ---------------------------------------------------------------- the fixture


def test_every_fixture_case(torch_cuda, fx):
    """Every case of the reference's fixture through from_manifest: the lists,
    then per run status_string, values and where."""
    from lsbm_amd import buffered, db
    torch = torch_cuda
    _, body = fx
    for name, case in body["cases"].items():
        files = bc.case_files(body, case)
        v, tables = bc.case_version(case, files)
        image = _dev(torch, np.frombuffer(bytes.fromhex(case["manifest"]), dtype=np.uint8))
        bv = buffered.BufferedVersion.from_manifest(image, files, case["compaction_buffer_length"],
                                                    bits_per_key=bc.BITS)
        assert {"%d,%d" % k: [[e[0] for e in t] for t in ts] for k, ts in bv.tables.items()} == case["lists"], name
        for r, run in enumerate(case["runs"]):
            p = bc.run_params(run)
            bc.set_visible(v, run)
            bv.configure(p.use_length, p.buffered_merge, p.read_cursor_keys)
            bv.visible.copy_(torch.tensor(visible_of(bv, v.lists()), dtype=torch.uint8))
            queries = [(bytes.fromhex(k), s) for k, s in run["queries"]]
            same_as_model(torch, bv, v, tables, p, queries, what=(name, r))
            status, values, _ = same_as_model.last
            for q, ((key, _), (want_status, want_value)) in enumerate(zip(queries, run["results"])):
                assert db.status_string(status[q], key) == want_status, (name, r, key)
                assert values[q] == want_value.encode("latin-1"), (name, r, key)


def test_a_number_without_bytes_raises(torch_cuda, fx):
    from lsbm_amd import buffered
    _, body = fx
    case = body["cases"]["lists"]
    files = bc.case_files(body, case)
    items, live, keys, offs = bc.case_added(case, files)
    tables = buffered.sorted_tables(items, live, keys, offs)
    del files[137]
    with pytest.raises(ValueError, match="file 137"):
        buffered.BufferedVersion(tables, files, bits_per_key=bc.BITS)


def test_all_buffers_empty_equals_for_levels(torch_cuda, fx):
    from lsbm_amd import buffered, db
    torch = torch_cuda
    _, body = fx
    case = body["cases"]["empty_buffers"]
    files = bc.case_files(body, case)
    items, live, keys, offs = bc.case_added(case, files)
    tables = buffered.sorted_tables(items, live, keys, offs)
    bv = buffered.BufferedVersion(tables, files, bits_per_key=bc.BITS)
    tf = lambda e: db.TableFile(files[e[0]], e[0], bc.BITS, e[2], e[3])
    plain = db.Version.for_levels([tf(e) for e in tables[(0, 0)][0]], [tf(e) for e in tables[(0, 1)][0]],
                                  [([tf(e) for e in tables[(level, 0)][0]], [tf(e) for e in tables[(level, 1)][0]])
                                   for level in range(1, 4)])
    queries = [(bytes.fromhex(k), s) for k, s in case["runs"][0]["queries"]]
    uk, uoff = dev_keys(torch, [u for u, _ in queries])
    snap = _dev(torch, np.array([s for _, s in queries], dtype=np.int64))
    a, b = bv.get(uk, uoff, snap), plain.get(uk, uoff, snap)
    assert a.status.cpu().tolist() == b.status.cpu().tolist() and a.where.cpu().tolist() == b.where.cpu().tolist()
    assert values_of(a) == values_of(b) and a.value_offsets.cpu().tolist() == b.value_offsets.cpu().tolist()
    assert set(a.status.cpu().tolist()) >= {db.FOUND, db.UNDECIDED}


# ---------------------------------------------------------------- the plan alone


def slot_table(rng, n_slots):
    """[(level, kind)] of n_slots slots, sorted, one DEL / HEAD / INS a level at most."""
    out = []
    for _ in range(n_slots):
        level = rng.randrange(4)
        out.append((level, bfm.SLOT_LEVEL0 if level == 0 else rng.choice((bfm.SLOT_WB, bfm.SLOT_REST, bfm.SLOT_REST,
                                                                          bfm.SLOT_DEL, bfm.SLOT_HEAD, bfm.SLOT_INS))))
    out.sort()
    seen = set()
    for i, (level, kind) in enumerate(out):  # a second DEL / HEAD / INS becomes a REST
        if kind in (bfm.SLOT_DEL, bfm.SLOT_HEAD, bfm.SLOT_INS):
            if (level, kind) in seen:
                out[i] = (level, bfm.SLOT_REST)
            seen.add((level, kind))
    out.sort()
    return out


class PlanInput:
    """The device tensors of one plan call and the host values beside them."""

    def __init__(self, torch, kinds, cand, use, wb, cursors, users):
        self.kinds, self.cand, self.use, self.wb, self.cursors, self.users = kinds, cand, use, wb, cursors, users
        n = len(users)
        self.d_cand = _dev(torch, np.array(cand, dtype=np.uint8).reshape(len(kinds), n).reshape(-1))
        self.d_info = _dev(torch, np.array([kind | (level << 8) for level, kind in kinds], dtype=np.int32))
        self.d_use = _dev(torch, np.array(use, dtype=np.int32))
        self.d_wb = _dev(torch, np.array(wb, dtype=np.int32))
        self.d_ckeys, self.d_coff = dev_keys(torch, cursors)
        self.d_keys, self.d_koff = dev_keys(torch, [gm.lookup_key(u, 77) for u in users])

    def inputs(self):
        return (self.d_cand, self.d_info, self.d_use, self.d_wb, self.d_ckeys, self.d_coff, self.d_keys, self.d_koff)

    def model(self):
        return plan_model(self.kinds, self.cand, self.use, self.wb, self.cursors, self.users)


def plan_model(kinds, cand, use, wb, cursors, users):
    """The probe list of every query, from the model."""
    return [bfm.plan(kinds, [cand[s][q] for s in range(len(kinds))], use, wb, cursors, users[q])
            for q in range(len(users))]


def random_plan_values(rng, n, n_slots):
    """(kinds, cand, use, wb, cursors, users) of a random plan input, on the host."""
    kinds = slot_table(rng, n_slots)
    users = [rng.choice((b"", b"k", b"k1", b"k12", b"k123456789", bytes(rng.randrange(256) for _ in range(rng.randrange(12)))))
             for _ in range(n)]
    # cursors: empty, equal to a query key, a prefix of it, just past it
    cursors = [rng.choice((b"", b"k1", b"k12", b"k12\x00", b"k123456789", b"k1234567", b"\xff")) for _ in range(4)]
    cand = [[rng.choice((0, 1, 2, 2, 2, 3)) for _ in range(n)] for _ in kinds]
    use = [rng.choice((0, 0, 1, 3)) for _ in range(4)]
    wb = [0] + [rng.randrange(2) for _ in range(3)]
    return kinds, cand, use, wb, cursors, users


def random_plan_input(torch, rng, n, n_slots):
    return PlanInput(torch, *random_plan_values(rng, n, n_slots))


def run_plan(torch, x):
    """(count, probe lists per query) through both calls, the cap exact."""
    from lsbm_amd import buffered
    count, st = buffered.probe_plan(*x.inputs())
    assert st.cpu().tolist() == [OK]
    counts = count.cpu().tolist()
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(first[-1])
    whole, view = guarded(torch, total, torch.int32, -7)
    st = buffered.probe_emit(*x.inputs(), _dev(torch, first), view, total)
    assert st.cpu().tolist() == [OK] and guards_intact(whole, total, -7)
    slots = view.cpu().tolist()
    return counts, [slots[first[q]:first[q + 1]] for q in range(len(counts))]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_plan_and_emit_on_synthetic_candidates(torch_cuda, n):
    torch = torch_cuda
    rng = random.Random(1000 + n)
    seen = set()
    for n_slots in (1, 63, 64, 65, 130):
        x = random_plan_input(torch, rng, n, n_slots)
        want = x.model()
        counts, probes = run_plan(torch, x)
        assert counts == [len(w) for w in want], (n, n_slots)
        assert probes == want, (n, n_slots)
        seen |= {x.kinds[s][1] for w in want for s in w}
    if n >= 63:
        assert seen == set(range(6))


def test_counts_0_and_all_side_by_side(torch_cuda):
    """Queries that probe nothing between queries that probe every slot."""
    torch = torch_cuda
    kinds = [(0, 0)] * 3 + [(2, bfm.SLOT_WB)] * 40 + [(2, bfm.SLOT_DEL), (2, bfm.SLOT_HEAD)] + \
        [(2, bfm.SLOT_REST)] * 60 + [(2, bfm.SLOT_INS)] + [(3, bfm.SLOT_DEL)] + [(3, bfm.SLOT_REST)] * 20 + \
        [(3, bfm.SLOT_INS)]
    n = 130
    cand = [[(2 if q % 2 == 0 else (0 if q % 4 == 1 else 1)) for q in range(n)] for _ in kinds]
    x = PlanInput(torch, kinds, cand, [0, 5, 0, 30], [0, 0, 1, 0], [b"", b"", b"a", b""], [b"k%03d" % q for q in range(n)])
    counts, probes = run_plan(torch, x)
    want = x.model()
    assert probes == want
    # level 2 with use 0: covered_by_del, so WB and DEL, then REST and INS (no HEAD); level 3: HEAD-less, REST, INS
    everything = [s for s, (level, kind) in enumerate(kinds) if kind != bfm.SLOT_HEAD and (level, kind) != (3, bfm.SLOT_DEL)]
    assert [c for c in counts[:4]] == [len(everything), 0, len(everything), 0] and probes[0] == everything


def test_probe_cap_exact_and_one_short(torch_cuda):
    from lsbm_amd import buffered
    torch = torch_cuda
    x = random_plan_input(torch, random.Random(77), 65, 64)
    count, st = buffered.probe_plan(*x.inputs())
    counts = count.cpu().tolist()
    first = _dev(torch, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    total = sum(counts)
    assert total > 100
    whole, view = guarded(torch, total, torch.int32, -7)
    assert buffered.probe_emit(*x.inputs(), first, view, total).cpu().tolist() == [OK]
    assert guards_intact(whole, total, -7) and -7 not in view.cpu().tolist()
    whole, view = guarded(torch, total, torch.int32, -7)
    assert buffered.probe_emit(*x.inputs(), first, view, total - 1).cpu().tolist() == [NO_ROOM]
    assert set(whole.cpu().tolist()) == {-7}  # nothing stored


def test_bad_input_leaves_the_outputs(torch_cuda):
    from lsbm_amd import _lib, buffered
    torch = torch_cuda
    rng = random.Random(5)
    kinds = [(0, 0), (1, bfm.SLOT_DEL), (1, bfm.SLOT_INS), (2, bfm.SLOT_WB), (2, bfm.SLOT_DEL), (2, bfm.SLOT_HEAD),
             (2, bfm.SLOT_REST), (2, bfm.SLOT_INS)]
    n = 70
    users = [b"key%02d" % q for q in range(n)]

    def good():
        return PlanInput(torch, list(kinds), [[rng.choice((0, 1, 2, 3)) for _ in range(n)] for _ in kinds],
                         [0, 1, 0, 2], [0, 0, 1, 1], [b"", b"a", b"key3", b""], users)

    def info(x, pairs):
        x.d_info = _dev(torch, np.array([kind | (level << 8) for level, kind in pairs], dtype=np.int32))

    def bad_cases():
        x = good()
        x.d_cand[5 * n + 3] = 4
        yield "a candidate code out of range", x
        x = good()
        info(x, kinds[:3] + [kinds[4], kinds[3]] + kinds[5:])
        yield "kinds out of order in a level", x
        x = good()
        info(x, [(0, 0), (2, bfm.SLOT_DEL), (2, bfm.SLOT_INS)] + [(1, k) for _, k in kinds[3:]])
        yield "levels not ascending", x
        for kind in (bfm.SLOT_DEL, bfm.SLOT_HEAD, bfm.SLOT_INS):
            x = good()
            info(x, kinds[:3] + sorted([(2, kind)] + [k for k in kinds[3:] if k[1] != bfm.SLOT_REST]))
            yield "two slots of kind %d" % kind, x
        x = good()
        info(x, kinds[:7] + [(4, bfm.SLOT_INS)])
        yield "a level above 3", x
        x = good()
        info(x, [(0, bfm.SLOT_WB)] + kinds[1:])
        yield "a level-0 slot of another kind", x
        x = good()
        info(x, kinds[:7] + [(2, 6)])
        yield "an unknown kind", x
        x = good()
        x.d_coff = _dev(torch, np.array([0, 0, 5, 1, 5], dtype=np.int64))
        yield "a cursor offset that decreases", x
        x = good()
        x.d_coff = _dev(torch, np.array([0, 0, 1, 5, 6], dtype=np.int64))
        yield "a cursor offset past its buffer", x
        x = good()
        x.d_koff = x.d_koff.clone()
        x.d_koff[7] += 9
        yield "a lookup key under 8 bytes", x
        x = good()
        x.d_koff = x.d_koff.clone()
        x.d_koff[n] += 1
        yield "a key offset past the buffer", x

    n_cases = 0
    for what, x in bad_cases():
        whole, view = guarded(torch, n, torch.int32, -7)
        _, st = buffered.probe_plan(*x.inputs(), count=view)
        assert st.cpu().tolist() == [BAD_INPUT], what
        assert set(whole.cpu().tolist()) == {-7}, what
        first = _dev(torch, np.arange(n + 1, dtype=np.int64))
        whole, view = guarded(torch, n, torch.int32, -7)
        assert buffered.probe_emit(*x.inputs(), first, view, n).cpu().tolist() == [BAD_INPUT], what
        assert set(whole.cpu().tolist()) == {-7}, what
        n_cases += 1
    assert n_cases == 13
    # emit alone: probe_first that does not step by the counts, or decreases
    x = good()
    count, _ = buffered.probe_plan(*x.inputs())
    first = np.concatenate([[0], np.cumsum(count.cpu().tolist())]).astype(np.int64)
    total = int(first[-1])
    for q, delta in ((3, 1), (9, -1), (n, 2)):
        wrong = first.copy()
        wrong[q] += delta
        whole, view = guarded(torch, total + 4, torch.int32, -7)
        assert buffered.probe_emit(*x.inputs(), _dev(torch, wrong), view, total + 4).cpu().tolist() == [BAD_INPUT]
        assert set(whole.cpu().tolist()) == {-7}
    # an output that overlaps an input is refused before anything is enqueued
    x = good()
    alias = x.d_use
    rc = _lib.lib().lsbm_probe_plan_dev(ptr(x.d_cand), len(kinds), ptr(x.d_info), ptr(x.d_use), ptr(x.d_wb),
                                        ptr(x.d_ckeys), x.d_ckeys.numel(), ptr(x.d_coff), ptr(x.d_keys),
                                        x.d_keys.numel(), ptr(x.d_koff), n, ptr(alias), ptr(x.d_wb),
                                        stream_ptr(torch))
    assert rc == -1


# ---------------------------------------------------------------- the whole chain


def test_random_tree_against_the_model(torch_cuda, random_pool):
    """About 2,000 random queries over a random tree with lists of up to 21
    tables per level (damaged files, invisible files and non-empty sentinels
    among them)."""
    from lsbm_amd import buffered
    torch = torch_cuda
    files, tables = random_pool
    rng = random.Random(424242)
    p = bfm.Params([0, 3, 26, 21], True, [b"", b"k10", b"k30", b"k5"])
    while True:  # (the first tree of the seed whose buffer lists are long)
        lists, _ = bc.random_tree(rng, files, max_tables=21)
        v = bfm.ModelVersion.from_lists(lists)
        if len(bfm.slots(v, p)) > 60:
            break
    bv = buffered.BufferedVersion(structure_of(lists), {f[0]: f[2] for f in files}, p.use_length, p.buffered_merge,
                                  p.read_cursor_keys, bits_per_key=bc.BITS, verify=False)
    bv.visible.copy_(torch.tensor(visible_of(bv, lists), dtype=torch.uint8))
    assert max(len(t) for t in lists.values()) >= 15 and len(bv.slots) > 60
    queries = bc.random_queries(rng, 2000)
    reads = same_as_model(torch, bv, v, tables, p, queries, verify=False, what="random")
    assert max(reads) >= 3 and min(reads) == 0


def test_rounds_with_widely_different_probe_counts(torch_cuda):
    """A key that every table may hold (a newer sequence than the snapshot's
    everywhere) between keys no table offers: ranks 0..S-1 beside rank 0."""
    from lsbm_amd import buffered
    torch = torch_cuda
    users = [b"k%02d" % i for i in range(12)]
    files, lists = {}, {(level, kind): [[]] for level in range(4) for kind in range(4)}

    def add(number, with_old):
        ents = [(u, 500, 1) for u in users] + ([(users[3], 20, 1)] if with_old else [])
        ents.sort(key=lambda e: (e[0], -e[1]))
        kv = [(u + (s << 8 | t).to_bytes(8, "little"), b"f%d:" % number + u) for u, s, t in ents]
        files[number] = memtablemodel.table_file(kv, 256, 4, bc.BITS)
        return bfm.FileMeta(number, len(files[number]), kv[0][0], kv[-1][0])

    lists[(2, 2)] = [[]] + [[add(200 + i, False)] for i in range(12)]
    lists[(2, 3)] = [[]] + [[add(300 + i, False)] for i in range(6)]
    lists[(2, 0)] = [[add(400, False)]]
    lists[(2, 1)] = [[add(401, False)]]
    lists[(3, 1)] = [[add(402, True)]]
    lists[(1, 2)] = [[], [add(403, False)]]
    p = bfm.Params([0, 9, 0, 0], True, [b"", b"", b"", b""])
    v = bfm.ModelVersion.from_lists(lists)
    tables = {n: gm.open_table(d, bc.BITS, None) for n, d in files.items()}
    bv = buffered.BufferedVersion(structure_of(lists), files, p.use_length, p.buffered_merge, p.read_cursor_keys,
                                  bits_per_key=bc.BITS)
    queries = []
    for i in range(40):
        queries += [(users[3], 100), (b"a", 100), (users[i % 12], 100), (b"zz", 100), (users[3], 10)]
    reads = same_as_model(torch, bv, v, tables, p, queries, what="wide")
    # use 0 at level 2: the six warm-up tables and the sentinel's slot, DEL, INS, then level 3's INS decides
    assert reads[0] == 6 + 1 + 1 + 1 and reads[1] == 0 and reads[3] == 0
    for use2 in (1, 13):  # HEAD and the rest of the buffer as well
        p.use_length[2] = use2
        bv.configure(p.use_length)
        reads = same_as_model(torch, bv, v, tables, p, queries, what=("wide", use2))
        assert reads[0] == 6 + 1 + min(use2 - 1, 11) + 1 + 1 and reads[1] == 0


def test_from_manifest_over_flushed_tables(torch_cuda):
    """Tables written by flush_many, named by manifest_image at buffer types,
    read back by from_manifest: the same answers as a BufferedVersion built
    directly, and the model's."""
    from lsbm_amd import buffered, manifest as mf
    from golden import manifest_cases as cases
    from test_manifest_chain_gpu import flushed_tables
    from test_manifest_gpu import i64, tobytes
    torch = torch_cuda
    logs, last, fs, _ = flushed_tables(torch)
    numbers = list(cases.DIRECTORY["table_numbers"])
    # (type, level, which table): the older table as level 2's insertion part and in its warm-up list, the newer one
    # in level 2's compaction buffer and as level 3's deletion part
    placed = [(1, 2, 0), (3, 2, 0), (2, 2, 1), (0, 3, 1), (1, 3, 0)]
    keys, offs = dev_keys(torch, [k for _, _, t in placed for k in (bytes(fs[t].smallest), bytes(fs[t].largest))])
    table = mf.FileTable(i64(torch, [numbers[t] for _, _, t in placed]), i64(torch, [fs[t].image.numel() for _, _, t in placed]),
                         i64(torch, [level for _, level, _ in placed]), i64(torch, [kind for kind, _, _ in placed]),
                         keys, offs)
    m = mf.manifest_image(table, log_number=9, next_file=50, last_sequence=last[1])
    views = {numbers[t]: fs[t].image for t in range(2)}
    params = dict(use_length=(0, 1, 2, 0), buffered_merge=True, read_cursor_keys=(b"", b"", b"", b""))
    a = buffered.BufferedVersion.from_manifest(m.log, views, **params)
    structure = {(level, kind): [[], [(numbers[t], fs[t].image.numel(), bytes(fs[t].smallest), bytes(fs[t].largest))]]
                 if kind >= 2 else [[(numbers[t], fs[t].image.numel(), bytes(fs[t].smallest), bytes(fs[t].largest))]]
                 for kind, level, t in placed}
    assert {k: t for k, t in a.tables.items() if any(t)} == structure
    b = buffered.BufferedVersion(structure, {n: tobytes(img) for n, img in views.items()}, **params)
    users = sorted({k for recs in logs for _, k, _ in cases.directory_ops(recs)})[::2] + [b"", b"key", b"key9999"]
    queries = [(u, s) for u in users for s in (last[0] // 2, last[0], last[2] + 5)]
    got_a, got_b = gpu_get(torch, a, queries), gpu_get(torch, b, queries)
    assert got_a == got_b
    lists = {k: [[bfm.FileMeta(*e) for e in t] for t in ts] for k, ts in structure.items()}
    for level in range(4):
        for kind in range(4):
            lists.setdefault((level, kind), [[]])
    v = bfm.ModelVersion.from_lists(lists)
    tables = {n: gm.open_table(tobytes(img), None, None) for n, img in views.items()}
    reads = same_as_model(torch, a, v, tables, bfm.Params(**params), queries, what="flushed")
    assert max(reads) >= 2 and len({w for w in got_a[2]}) >= 3


def test_host_reads_do_not_grow_with_the_sorted_tables(torch_cuda, monkeypatch):
    """The same queries over trees whose compaction-buffer lists hold 2, 8 and
    20 tables: as many .cpu() / .item() / .tolist() calls in each.  The queries
    are chosen with the model so that every tree needs the same number of
    rounds (a condition of the comparison, checked here)."""
    from lsbm_amd import buffered
    torch = torch_cuda
    counts = {}

    def counted(name):
        real = getattr(torch.Tensor, name)

        def call(self, *a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return real(self, *a, **kw)
        return call

    def reads_of(call):
        with monkeypatch.context() as m:
            counts.clear()
            for name in ("cpu", "item", "tolist"):
                m.setattr(torch.Tensor, name, counted(name))
            call()
            return dict(counts)

    users = {2: [b"k%02d" % i for i in range(40)], 3: [b"m%02d" % i for i in range(40)]}
    wide = lambda u: (u[:1] + b"\x00" + (100 << 8 | 1).to_bytes(8, "little"), u[:1] + b"zz" + (1 << 8 | 1).to_bytes(8, "little"))
    trees = []
    for n_tables in (2, 8, 20):
        files, lists = {}, {(level, kind): [[]] for level in range(4) for kind in range(4)}
        number = [1000 * n_tables]

        def add(keys, prefix):
            number[0] += 1
            kv = [(u + (50 << 8 | 1).to_bytes(8, "little"), b"f%d:" % number[0] + u) for u in sorted(keys)]
            files[number[0]] = memtablemodel.table_file(kv, 256, 4, bc.BITS)
            return bfm.FileMeta(number[0], len(files[number[0]]), *wide(prefix))

        for level in (2, 3):
            # every key lives in one table of the compaction buffer, and in the insertion part (the gate)
            lists[(level, 2)] = [[]] + [[add(users[level][t::n_tables], users[level][0])] for t in range(n_tables)]
            lists[(level, 1)] = [[add(users[level], users[level][0])]]
        trees.append((files, lists))
    p = bfm.Params([0, 0, 25, 25], True, [b"", b"", b"", b""])
    candidates = [(u, 100) for level in (2, 3) for u in users[level]] + [(b"j", 100), (b"zzz", 100)]
    opened, per_query = [], []
    for files, lists in trees:
        v = bfm.ModelVersion.from_lists(lists)
        tables = {n: gm.open_table(d, bc.BITS, None) for n, d in files.items()}
        opened.append((v, tables))
        memo = {}
        per_query.append([bfm.rule_get(v, tables, p, u, s, memo=memo)[4] for u, s in candidates])
    # the queries whose reads are the same in the three trees (a filter's false positive adds a read in one of them)
    queries = [c for q, c in enumerate(candidates) if len({r[q] for r in per_query}) == 1]
    assert len(queries) >= 60
    rounds = [max(r[q] for q, c in enumerate(candidates) if c in queries) for r in per_query]
    assert rounds[0] == rounds[1] == rounds[2] >= 1, rounds
    uk, uoff = dev_keys(torch, [u for u, _ in queries])
    reads = []
    for (files, lists), (v, tables) in zip(trees, opened):
        bv = buffered.BufferedVersion(structure_of(lists), files, p.use_length, p.buffered_merge, p.read_cursor_keys,
                                      bits_per_key=bc.BITS)
        same_as_model(torch, bv, v, tables, p, queries, what="host reads")
        reads.append(reads_of(lambda: bv.get(uk, uoff, 100)))
    assert len(trees[2][1][(2, 2)]) == 21 and reads[0] == reads[1] == reads[2] and sum(reads[0].values()) > 0, reads
