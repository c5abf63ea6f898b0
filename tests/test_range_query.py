"""LSbM's range query, on the CPU: the literal model of Version::RangeQuery and
TableCache::GetRange (tests/golden/rangemodel.py) against the reference's own
results (tests/golden/range_fixture.json, range_tables.bin; made by
make_range_fixture.py), the rule the device runs (layout_range_slots and the
gates as include/lsbm_range.h states them) against the literal model, and the
header against _lib.RANGE_SIGNATURES.
"""
import ctypes
import os
import random
import re

import pytest

from golden import buffermodel as bfm
from golden import range_cases as rc
from golden import rangemodel as rgm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return rc.load_fixture()


@pytest.fixture(scope="module")
def opened(fx):
    """{case: (ModelVersion, blocks per file, {number: bytes})}"""
    _, body = fx
    out = {}
    for name, case in body["cases"].items():
        files = rc.case_files(body, case)
        out[name] = rc.case_version(case, files) + (files,)
    return out


def test_fixture_covers_the_cases(fx, opened):
    index, body = fx
    assert set(body["cases"]) == {"gates", "gates_level3", "damaged", "counts"}
    for name, c in index["cases"].items():
        assert c["files"] <= 40 and c["entries"] <= 300, name
    trace, by_case = set(), {}
    for name, case in body["cases"].items():
        v, _, _ = opened[name]
        mine = set()
        for run in case["runs"]:
            p = rc.run_params(run)
            for a, b, _ in rc.case_queries(case):
                rgm.version_range_files(v, p, a, b, mine)
        by_case[name] = mine
        trace |= mine
    # every gate, both ways, at levels 2 and 3; level 1 never walks the warm-up buffer
    for level in (2, 3):
        for what in ("checkwb", "wb_covered", "wb_dropped", "dl_covered", "dl_not_covered", "upto_closed",
                     "cb_from_head", "cb_from_next", "cb_covered", "cb_dropped", "reads_nothing"):
            assert (level, what) in trace, (level, what)
    assert (1, "checkwb") not in trace and (1, "cb_covered") in trace and (1, "cb_from_next") in trace
    assert (1, "reads_nothing") in by_case["counts"] or (2, "reads_nothing") in by_case["counts"]
    # circular lists of 1, 2 and 4 tables for both buffers
    lengths = {kind: {len(case["lists"]["%d,%d" % (level, kind)]) for case in body["cases"].values()
                      for level in (1, 2, 3)} for kind in (2, 3)}
    assert lengths[2] >= {1, 2, 4} and lengths[3] >= {1, 2, 4}
    gates = body["cases"]["gates"]
    uses = {tuple(r["use_length"]) for r in gates["runs"]}
    assert {u[2] for u in uses} >= {0, 1, 2, 3, 5} and {u[1] for u in uses} >= {0, 1, 2, 3, 9}
    assert {r["buffered_merge"] for r in gates["runs"]} == {True, False}
    uptos = {bytes.fromhex(r["read_upto_key"]) for r in gates["runs"]}
    ends = {b for _, b, _ in rc.case_queries(gates)}
    # read_upto_key: empty, below some end key (its gate closed for that query) and above every end key
    assert b"" in uptos and any(u and any(not e < u for e in ends) for u in uptos)
    assert any(all(e < u for e in ends) for u in uptos)
    # the cursor: a start below, equal to and above a cursor key of level 2
    cursors = {bytes.fromhex(r["read_cursor_keys"][2]) for r in gates["runs"]} - {b""}
    starts = {a for a, _, _ in rc.case_queries(gates)}
    assert any(any(s < c for s in starts) and c in starts and any(s > c for s in starts) for c in cursors)
    # a Level-0 insertion list that is not in key order; start keys of exactly 8 bytes and longer
    v, _, _ = opened["gates"]
    l0 = [f.largest for f in v.levels_[0][bfm.INSERTION_PART].files_]
    assert len(l0) == 2 and l0[0] > l0[1]
    assert {len(s) for s in starts} >= {8, 9, 16} and min(len(s) for s in starts) == 8
    # damaged index blocks; two files of one sorted table that share a boundary user key
    assert body["cases"]["damaged"]["damaged"] == [3, 211, 301]
    v, blocks, _ = opened["damaged"]
    assert blocks[211] is None and blocks[301] is None and blocks[3] is None
    v, blocks, _ = opened["counts"]
    ins = v.levels_[1][bfm.INSERTION_PART].files_
    assert any(a.largest[:-8] == b.smallest[:-8] for a, b in zip(ins, ins[1:]))
    # the counts: 0, 1, 63, 64, 65 and 130 entries inside one file; a file of one entry; 40-byte keys
    counts = body["cases"]["counts"]
    numbers = sorted(int(n) for n in counts["files"])
    of = lambda n: {row[numbers.index(n)] for row in counts["file_counts"]}
    assert of(11) >= {0, 1, 63, 64, 65, 130, 200, 10} and of(13) == {0, 1} and of(12) >= {12, 1, 24}
    assert len(blocks[13]) == 1 and len(blocks[13][0][1]) == 1
    assert all(len(k) == 48 for _, keys in blocks[12] for k in keys)


def test_model_reproduces_the_recovered_lists(fx, opened):
    _, body = fx
    for name, case in body["cases"].items():
        v, _, _ = opened[name]
        assert {"%d,%d" % k: t for k, t in v.numbers().items()} == case["lists"], name


def test_model_reproduces_every_count(fx, opened):
    """TableCache::GetRange of every query on every file of its tree."""
    _, body = fx
    n = 0
    for name, case in body["cases"].items():
        _, blocks, files = opened[name]
        numbers = sorted(files)
        for q, (a, b, s) in enumerate(rc.case_queries(case)):
            lkstart, lkend = rgm.lookup_key(a, s), rgm.lookup_key(b, s)
            got = [rgm.get_range(blocks[number], lkstart, lkend) for number in numbers]
            assert got == case["file_counts"][q], (name, q, a, b, s)
            n += len(got)
    assert n == sum(c["files"] * c["queries"] for c in fx[0]["cases"].values()) > 1000


def test_the_stop_predicate_is_not_monotone(fx, opened):
    """The end key's versions under snapshot 256: sequence 512 stops the count
    before 256 (counted) and 255 (stops); a user key that extends the end key
    by 0x00 is counted, by 0x02 stops, a proper prefix is counted."""
    _, body = fx
    case = body["cases"]["counts"]
    numbers = sorted(int(n) for n in case["files"])
    queries = rc.case_queries(case)
    q = queries.index((b"bbbbb000", b"bbbbb100", 256))
    row = dict(zip(numbers, case["file_counts"][q]))
    # 21: b050, the prefix, then @512 stops.  22: b050, @256, then @255 stops.  23: b050, the deletion @1 (a type byte
    # of 0), the 0x00 extension, then 0x02 stops.  24: b050, the prefix, both 0x00 extensions, then 0x02 stops.
    assert (row[21], row[22], row[23], row[24]) == (2, 2, 3, 4)


def test_model_reproduces_every_file_list_and_return_value(fx, opened):
    _, body = fx
    n_reads = 0
    for name, case in body["cases"].items():
        v, blocks, _ = opened[name]
        for r, run in enumerate(case["runs"]):
            p = rc.run_params(run)
            for q, (a, b, s) in enumerate(rc.case_queries(case)):
                found, checked, read, _ = rgm.range_query(v, blocks, p, a, b, s)
                assert [found, read] == run["results"][q], (name, r, q)
                assert checked == len(read)
                n_reads += checked
    assert n_reads == sum(c["reads"] for c in fx[0]["cases"].values()) > 5000


def rule_files(lists, p, start, end):
    """(file numbers in read order, flag words) by the device's rule."""
    from lsbm_amd import rangequery
    slots = rangequery.layout_range_slots(rgm.structure_of(lists), p.use_length, p.buffered_merge)
    pairs = rgm.rule_plan(slots, p.use_length, rgm.wb_enabled(p), list(p.read_cursor_keys) + [p.read_upto_key],
                          start, end)
    return [slots[s].files[i][0] for s, i, _ in pairs], [flags for _, _, flags in pairs]


def literal_files(v, p, start, end):
    groups = rgm.version_range_files(v, p, start, end)
    numbers = [f.number for g in groups for f in g]
    last, at = [], 0
    for g in groups:
        at += len(g)
        if g:
            last.append(at - 1)
    return numbers, last


def test_rule_equals_the_model_on_the_fixture(fx, opened):
    _, body = fx
    for name, case in body["cases"].items():
        v, _, _ = opened[name]
        for run in case["runs"]:
            p = rc.run_params(run)
            for a, b, _ in rc.case_queries(case):
                numbers, flags = rule_files(v.lists(), p, a, b)
                want, last = literal_files(v, p, a, b)
                assert numbers == want, (name, run, a, b)
                assert [i for i, f in enumerate(flags) if f & rgm.RANGE_LAST] == last, (name, run, a, b)


def test_rule_equals_the_model_on_random_trees():
    rng = random.Random(20250)
    trace, n = set(), 0
    for _ in range(150):
        lists, p = rc.random_tree(rng)
        v = bfm.ModelVersion.from_lists(lists)
        for a, b in rc.random_queries(rng, 25):
            want, last = literal_files(v, p, a, b)
            rgm.version_range_files(v, p, a, b, trace)
            numbers, flags = rule_files(lists, p, a, b)
            assert numbers == want, (lists, vars(p), a, b)
            assert [i for i, f in enumerate(flags) if f & rgm.RANGE_LAST] == last
            n += len(want)
    assert n > 3000
    for level in (2, 3):
        for what in ("wb_covered", "wb_dropped", "dl_covered", "cb_from_next", "cb_covered", "cb_dropped"):
            assert (level, what) in trace, (level, what)


def test_slot_flags_on_lists_of_one_two_and_four_tables():
    from lsbm_amd import rangequery as rq
    e = lambda n: (n, 100, rc.ikey(rc.user(1), 9), rc.ikey(rc.user(5), 1))
    tables = {(2, 2): [[]], (2, 3): [[]], (3, 2): [[], [e(1)]], (3, 3): [[], [e(2)]],
              (1, 2): [[], [e(3)], [e(4)], [e(5)]]}
    slots = rq.layout_range_slots(tables, (0, 9, 9, 9), True)
    of = lambda level, kind: [(s.flags, [f[0] for f in s.files]) for s in slots if (s.level, s.kind) == (level, kind)]
    assert of(2, rq.RSLOT_CB) == [(rq.RANGE_COVERS | rq.RANGE_SOLE, [])]
    assert of(2, rq.RSLOT_WB) == [(rq.RANGE_COVERS, [])]
    assert of(3, rq.RSLOT_CB) == [(rq.RANGE_COVERS, [1]), (0, [])]   # cb, then the sentinel
    assert of(3, rq.RSLOT_WB) == [(rq.RANGE_COVERS, []), (0, [2])]   # the sentinel itself covers
    assert of(1, rq.RSLOT_CB) == [(0, [3]), (0, [4]), (rq.RANGE_COVERS, [5]), (0, [])]
    assert of(1, rq.RSLOT_WB) == []  # level 1 never walks the warm-up buffer
    assert [s.kind for s in slots if s.level == 0] == [rq.RSLOT_ALL, rq.RSLOT_L0INS]
    # the use lengths cut the walks, not the flag
    slots = rq.layout_range_slots(tables, (0, 2, 0, 0), True)
    assert [(s.flags, [f[0] for f in s.files]) for s in slots if (s.level, s.kind) == (1, rq.RSLOT_CB)] == \
        [(0, [3]), (0, [4])]


def test_header_declarations_equal_the_signature_table():
    from lsbm_amd import _lib
    text = open(os.path.join(REPO, "include", "lsbm_range.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {}
    for ret, fn, params in re.findall(r"\b(\w+)\s+(lsbm_\w+)\s*\(([^;{]*)\)\s*;", text):
        args = []
        for p in params.split(","):
            p = p.strip()
            args.append(ctypes.c_void_p if "*" in p else {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
                                                          "int": ctypes.c_int}[p.split()[0]])
        declared[fn] = ({"int": ctypes.c_int}[ret], args)
    assert sorted(declared) == ["lsbm_range_count_dev", "lsbm_range_emit_dev", "lsbm_range_plan_dev"]
    assert declared == {k: (res, list(args)) for k, (res, args) in _lib.RANGE_SIGNATURES.items()}
    from lsbm_amd import rangequery as rq
    consts = dict(re.findall(r"#define\s+LSBM_RANGE_(\w+)\s+(\d+)u", text))
    assert [int(consts["SLOT_" + k]) for k in ("ALL", "L0INS", "WB", "DEL", "CB", "INS")] == \
        [rq.RSLOT_ALL, rq.RSLOT_L0INS, rq.RSLOT_WB, rq.RSLOT_DEL, rq.RSLOT_CB, rq.RSLOT_INS]
    assert (int(consts["COVERS"]), int(consts["SOLE"]), int(consts["LAST"]), int(consts["NO_ENTRIES"])) == \
        (rq.RANGE_COVERS, rq.RANGE_SOLE, rq.RANGE_LAST, rq.RANGE_NO_ENTRIES)
    assert int(consts["CURSORS"]) == rq.N_CURSORS and int(consts["LEVELS"]) == rq.kNumLevels


def test_no_range_callable_takes_a_stream():
    import inspect
    from lsbm_amd import rangequery as rq
    for name, obj in vars(rq).items():
        if inspect.isfunction(obj) and obj.__module__ == rq.__name__:
            assert "stream" not in inspect.signature(obj).parameters, name
    for name, member in vars(rq.RangeQuery).items():
        if inspect.isfunction(member):
            assert "stream" not in inspect.signature(member).parameters, name


def test_symbols_exported(product_lib):
    from lsbm_amd import _lib
    for name in _lib.RANGE_SIGNATURES:
        assert hasattr(product_lib, name), name
