"""The plain-Python model of LSbM's buffered read path (tests/golden/buffermodel.py)
against the reference's own results (tests/golden/buffered_fixture.json,
buffered_tables.bin, written by tests/golden/make_buffered_fixture.py from lsbm's
Recover and Version::Get): every recovered sorted-table list, every status and
every value.  Then the rule the device runs (slots, candidates, the probe plan)
against the literal model on seeded random trees, the library's own host-side
list and slot builders (lsbm_amd/buffered.py) against the model's, and the
all-buffers-empty case against getmodel's for_levels answer.  CPU only; the GPU
Get is compared with the same fixture and the same model in
tests/test_buffered_gpu.py.
"""
import random

import pytest

from golden import buffered_cases as bc
from golden import buffermodel as bfm
from golden import getmodel as gm


@pytest.fixture(scope="module")
def fx():
    return bc.load_fixture()


@pytest.fixture(scope="module")
def opened(fx):
    """{case: (ModelVersion, tables, files)}"""
    _, body = fx
    out = {}
    for name, case in body["cases"].items():
        files = bc.case_files(body, case)
        v, tables = bc.case_version(case, files)
        out[name] = (v, tables, files)
    return out


def test_fixture_covers_the_cases(fx):
    index, body = fx
    assert set(index["cases"]) == set(body["cases"]) >= {"gates", "damaged_walk", "damaged_ins", "damaged_del",
                                                         "lists", "empty_buffers"}
    assert index["cases"]["damaged_walk"]["statuses"]["Corruption: bad block contents"] > 0
    assert "Corruption: bad block contents" not in index["cases"]["damaged_ins"]["statuses"]
    assert "Corruption: bad block contents" not in index["cases"]["damaged_del"]["statuses"]
    lists = body["cases"]["lists"]["lists"]
    assert lists["3,2"][0] == [] and len(lists["3,2"]) == 4  # evicted down to compaction_buffer_length + 1
    assert [] in lists["2,2"][1:]                            # an empty table in the middle of a list
    assert lists["0,0"] == [[155, 151, 153]]                 # Level 0 keeps the added order
    assert all(t == [] for t in lists["2,3"])
    for name, case in body["cases"].items():
        assert len(case["runs"]) == index["cases"][name]["runs"]
    # level 2 of the gates case: every table of WB, DEL, the compaction buffer and INS decides somewhere, and level 3
    winners = {res[1].split(":")[0] for r in body["cases"]["gates"]["runs"] for res in r["results"]}
    assert winners >= {"f21", "f22", "f23", "f31", "f41", "f42", "f43", "f44", "f51", "f61"}, winners
    # k07..k09 sit in the rest of the compaction buffer one table deeper each: use lengths 1, 2, 3, 5 differ
    by_use = {r["use_length"][2]: [res[1].split(":")[0] for res in r["results"][2:5]]
              for r in body["cases"]["gates"]["runs"][:12]}
    assert by_use == {0: ["f51"] * 3, 1: ["f51"] * 3, 2: ["f43", "f51", "f51"], 3: ["f43", "f42", "f51"],
                      5: ["f43", "f42", "f41"], 10: ["f43", "f42", "f41"]}, by_use


def test_model_reproduces_the_recovered_lists(fx, opened):
    _, body = fx
    for name, case in body["cases"].items():
        v = opened[name][0]
        got = {"%d,%d" % k: t for k, t in v.numbers().items()}
        assert got == case["lists"], name


def test_model_reproduces_every_status_and_value(fx, opened):
    _, body = fx
    n = 0
    for name, case in body["cases"].items():
        v, tables, _ = opened[name]
        for r, run in enumerate(case["runs"]):
            p = bc.run_params(run)
            bc.set_visible(v, run)
            for (khex, seq), (status, value) in zip(run["queries"], run["results"]):
                key = bytes.fromhex(khex)
                verdict, got, _ = bfm.version_get(v, tables, p, key, seq)
                assert gm.status_string(verdict, key) == status, (name, r, key, seq)
                assert (got or b"") == value.encode("latin-1"), (name, r, key, seq)
                n += 1
    assert n > 2000


def test_rule_equals_the_model_on_the_fixture(fx, opened):
    _, body = fx
    for name, case in body["cases"].items():
        v, tables, _ = opened[name]
        for run in case["runs"]:
            p = bc.run_params(run)
            bc.set_visible(v, run)
            layout = bfm.slots(v, p)
            for khex, seq in run["queries"]:
                key = bytes.fromhex(khex)
                want = bfm.version_get(v, tables, p, key, seq)
                got = bfm.rule_get(v, tables, p, key, seq, layout=layout)
                assert (got[0], got[1]) == (want[0], want[1]) and got[2] is want[2], (name, key, seq)


@pytest.fixture(scope="module")
def random_pool():
    files = bc.pool()
    return files, {f[0]: gm.open_table(f[2], bc.BITS, None, False) for f in files}


def test_rule_equals_the_model_on_random_trees(random_pool):
    files, tables = random_pool
    rng = random.Random(20240607)
    decided, errors, kinds = 0, 0, set()
    for t in range(600):
        lists, p = bc.random_tree(rng, files)
        v = bfm.ModelVersion.from_lists(lists)
        layout = bfm.slots(v, p)
        for key, seq in bc.random_queries(rng, 6):
            want = bfm.version_get(v, tables, p, key, seq, verify=False)
            got = bfm.rule_get(v, tables, p, key, seq, verify=False, layout=layout)
            assert (got[0], got[1]) == (want[0], want[1]) and got[2] is want[2], (t, key, seq)
            if got[3] >= 0:
                decided += 1
                kinds.add(layout[got[3]][1])
                errors += got[0] >= gm.ERROR
    # the trees reach every kind of slot, and errors too
    assert kinds == set(range(6)) and decided > 1000 and errors > 10, (kinds, decided, errors)


def _as_structure(lists):
    return {k: [[(f.number, f.file_size, f.smallest, f.largest) for f in t] for t in ts] for k, ts in lists.items()}


def test_library_lists_and_slots_equal_the_model(fx, random_pool):
    from lsbm_amd import buffered
    _, body = fx
    for name, case in body["cases"].items():
        files = bc.case_files(body, case)
        items, live, keys, offs = bc.case_added(case, files)
        got = buffered.sorted_tables(items, live, keys, offs, case["compaction_buffer_length"])
        assert {"%d,%d" % k: [[e[0] for e in t] for t in ts] for k, ts in got.items()} == case["lists"], name
        for (level, kind), ts in got.items():
            for t in ts:
                for number, size, smallest, largest in t:
                    assert size == len(files.get(number, b""))
    pool_files, _ = random_pool
    rng = random.Random(5)
    for _ in range(200):
        lists, p = bc.random_tree(rng, pool_files)
        v = bfm.ModelVersion.from_lists(lists)
        want = [(level, kind, [f.number for f in fs], level0) for level, kind, fs, level0 in bfm.slots(v, p)]
        got = buffered.layout_slots(_as_structure(lists), p.use_length, p.buffered_merge)
        assert [(s.level, s.kind, [e[0] for e in s.files], bool(s.flags & 1)) for s in got] == want
        structure = _as_structure(lists)
        for s in got:  # refs name the entries
            for e, (kind, t, i) in zip(s.files, s.refs):
                assert structure[(s.level, kind)][t][i] == e


def test_eviction_keeps_length_plus_one():
    from lsbm_amd import buffered
    for length in (0, 1, 3):
        ours, v = [[]], bfm.ModelVersion((0, length, length, length))
        for i in range(8):
            ours[0].append(i)
            v.levels_[1][2].files_.append(bfm.FileMeta(i, 0, b"a" * 9, b"b" * 9))
            buffered.new_sorted_table(ours, 1, 2, (0, length, length, length))
            v.new_sorted_table(1, 2)
            assert ours == [[f.number for f in t] for t in v.lists()[(1, 2)]]
            assert len(ours) == min(i + 2, length + 1)


def test_all_buffers_empty_equals_for_levels(fx, opened):
    _, body = fx
    case = body["cases"]["empty_buffers"]
    v, tables, files = opened["empty_buffers"]
    lists = v.lists()
    entry = lambda f: (f.number, f)
    level0_del = [entry(f) for f in lists[(0, 0)][0]]
    runs = gm.for_levels(level0_del, [entry(f) for f in lists[(0, 1)][0]],
                         [([entry(f) for f in lists[(level, 0)][0]], [entry(f) for f in lists[(level, 1)][0]])
                          for level in range(1, 4)])
    order, flat_runs = [], []
    for fs, flags in runs:
        flat_runs.append((list(range(len(order), len(order) + len(fs))), flags))
        order += [f for _, f in fs]
    flat_tables = [tables[f.number] for f in order]
    bounds = [(f.smallest, f.largest) for f in order]
    compared = 0
    for run in case["runs"]:
        p = bc.run_params(run)
        if any(p.use_length):  # (a use length above 0 takes the deletion part out of the walk: not for_levels' tree)
            continue
        for khex, seq in run["queries"]:
            key = bytes.fromhex(khex)
            want = gm.version_get([], flat_tables, bounds, flat_runs, key, seq, None)
            got = bfm.version_get(v, tables, p, key, seq)
            assert (got[0], got[1]) == (want[0], want[1]), (key, seq)
            # with nothing in the buffers the slots are for_levels' runs, one for one
            assert bfm.rule_get(v, tables, p, key, seq)[3] == want[2], (key, seq)
            compared += 1
    assert compared >= 50
