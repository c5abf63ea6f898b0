"""The range-scan model (CPU): tests/golden/scanmodel.py against the reference's
own DBIter, and its closed form against its port.

* the line-by-line port of lsbm/db_iter.cc reproduces every record of
  tests/golden/scan_fixture.json (entries and status().ToString()), over the
  merged iteration the reference's MergingIterator produced;
* that merged iteration is the stable merge of the children's iterations;
* the closed form (the arithmetic of lsbm_dbiter_plan_dev / _range_dev) equals
  the port in entries and status on seeded random histories with error keys,
  under several snapshots (0 and kMaxSequenceNumber among them), in both
  directions, with random lo, hi and limit -- and on every fixture query;
* ParseKey runs on exactly the positions the closed form's ranges name.
"""
import random

import pytest

from golden import scan_cases
from golden import scanmodel as sm

SEEDS = range(300)


def test_fixture_has_the_cases():
    names = [c[0] for c in scan_cases.cases()]
    assert names == ["semantics", "empty", "tables_only"]
    total = sum(len(c[3]) for c in scan_cases.cases())
    assert total > 5000
    statuses = {q[6] for c in scan_cases.cases() for q in c[3]}
    assert statuses == set(sm.STATUS_STRING.values())


def test_merged_iteration_is_the_stable_merge_of_the_children():
    for name, children, merged, _ in scan_cases.cases():
        tagged = [(k[:-8], -sm.tag_of(k), c, i, (k, v)) for c, child in enumerate(children)
                  for i, (k, v) in enumerate(child)]
        assert [t[4] for t in sorted(tagged, key=lambda t: t[:4])] == merged, name
        assert merged == sm.sort_entries(merged), name


@pytest.mark.parametrize("case", range(3))
def test_port_reproduces_every_fixture_record(case):
    name, _, merged, queries = scan_cases.cases()[case]
    for s, lo, hi, limit, rev, want, status in queries:
        got, st, _ = sm.scan_port(merged, s, lo, hi, limit, rev)
        assert got == want, (name, s, lo, hi, limit, rev)
        assert sm.STATUS_STRING[st] == status, (name, s, lo, hi, limit, rev)


@pytest.mark.parametrize("case", range(3))
def test_closed_form_reproduces_every_fixture_record(case):
    name, _, merged, queries = scan_cases.cases()[case]
    views = {}
    for s, lo, hi, limit, rev, want, status in queries:
        if s not in views:
            views[s] = sm.View(merged, s)
        jb, count, st = sm.scan_closed(views[s], lo, hi, limit, rev)
        assert sm.scan_entries(views[s], jb, count, rev) == want, (name, s, lo, hi, limit, rev)
        assert sm.STATUS_STRING[st] == status, (name, s, lo, hi, limit, rev)


def test_closed_form_equals_port_on_random_histories():
    checked = corrupt = 0
    for seed in SEEDS:
        entries, users = scan_cases.random_history(seed)
        rng = random.Random(seed)
        for s in (0, sm.kMaxSequenceNumber, rng.randint(1, 30), rng.randint(1, 30)):
            view = sm.View(entries, s)
            for lo, hi, limit in scan_cases.random_queries(seed + s % 31, users, 8):
                for rev in (False, True):
                    want, st, _ = sm.scan_port(entries, s, lo, hi, limit, rev)
                    jb, count, st2 = sm.scan_closed(view, lo, hi, limit, rev)
                    assert sm.scan_entries(view, jb, count, rev) == want, (seed, s, lo, hi, limit, rev)
                    assert st2 == st, (seed, s, lo, hi, limit, rev)
                    checked += 1
                    corrupt += st
    assert checked >= 300 * 4 * 8 * 2 and corrupt > checked // 20  # (the error keys are met often enough)


def test_forward_and_reverse_yield_the_same_set():
    for seed in SEEDS:
        entries, _ = scan_cases.random_history(seed)
        for s in (0, 15, sm.kMaxSequenceNumber):
            fwd, _, _ = sm.scan_port(entries, s)
            rev, _, _ = sm.scan_port(entries, s, reverse=True)
            assert fwd == rev[::-1], (seed, s)
            view = sm.View(entries, s)
            assert fwd == sm.scan_entries(view, 0, view.n_yield), (seed, s)


def _walked(view, lo, hi, limit, reverse):
    """The positions ParseKey runs on, from the view's arrays."""
    v, n, ny, s = view, view.n, view.n_yield, view.snapshot
    if limit <= 0:
        return set()
    p_lo = 0 if lo is None else sm.lower_bound(v.entries, sm.ikey(lo, s))
    p_hi = n if hi is None else sm.lower_bound(v.entries, sm.ikey(hi, s))
    j_lo, j_hi = v.yield_rank[p_lo], v.yield_rank[p_hi]
    if not reverse:
        jl = max(j_lo, min(j_lo + limit - 1, j_hi))
        return set(range(p_lo, v.live[jl] + 1 if jl < ny else n))
    out, upper = set(), n
    if hi is not None and j_hi < ny:
        out |= set(range(p_hi, v.live[j_hi] + 1))
        upper = v.first[j_hi]
    elif hi is not None:
        out |= set(range(p_hi, n))
    jt = min(j_hi - 1, max(j_hi - limit, j_lo - 1))
    lower = v.back[jt] if jt >= 0 and v.back[jt] >= 0 else 0
    return out | set(range(lower, upper))


def test_parsekey_runs_on_the_positions_the_ranges_name():
    for seed in SEEDS:
        entries, users = scan_cases.random_history(seed)
        for s in (0, 12, 20, sm.kMaxSequenceNumber):
            view = sm.View(entries, s)
            for lo, hi, limit in scan_cases.random_queries(seed, users, 6):
                for rev in (False, True):
                    _, _, parsed = sm.scan_port(entries, s, lo, hi, limit, rev)
                    assert set(parsed) == _walked(view, lo, hi, limit, rev), (seed, s, lo, hi, limit, rev)


def test_view_refuses_what_the_plan_refuses():
    with pytest.raises(ValueError, match="BAD_INPUT"):
        sm.View([(b"7 bytes", b"")], 5)
    with pytest.raises(ValueError, match="UNSORTED"):
        sm.View([(sm.ikey(b"b", 1), b""), (sm.ikey(b"a", 1), b"")], 5)
    with pytest.raises(ValueError, match="UNSORTED"):
        sm.View([(sm.ikey(b"a", 1), b""), (sm.ikey(b"a", 2), b"")], 5)
    assert sm.View([(sm.ikey(b"a", 2), b"x"), (sm.ikey(b"a", 2), b"y")], 5).live == [0]  # equal neighbours are legal
