"""Batched range scans (lsbm's DBIter, lsbm/db_iter.cc: NewIterator / Seek /
SeekToFirst / SeekToLast / Next / Prev / status) on the GPU.

Thin wrappers over include/lsbm_iter.h and the chain between them.  Device
tensors in, device tensors out; every call runs on `stream` (default:
torch's current stream; the contract is engine.py's).

    plan(keys, key_offsets, snapshot)   the snapshot view of sorted entries:
                                       which merged positions a DBIter at
                                       `snapshot` yields, and the ranks that
                                       place a query among them
    view(keys, key_offsets, values, value_image, snapshot)
                                       plan + merge.gather of the live entries
                                       + the prefix of their value lengths: a
                                       SnapshotView
    SnapshotView.range(lo, lo_offsets, ...)
                                       each query's window of live entries and
                                       its status
    SnapshotView.scan(lo, lo_offsets, hi, hi_offsets, limit, reverse, ...)
                                       range + emit: the user keys and values
                                       of every query's window
    SnapshotView.seek / seek_to_first / seek_to_last
                                       scans with limit 1
    status_string(code)                the reference's Status::ToString()

Entries are what block.decode and merge.merge return: a uint8 key buffer of
internal keys in InternalKeyComparator order plus int64 offsets and int64
{offset, length} value slices into a value image.  Query keys are user keys: a
uint8 buffer plus int64 offsets, and an optional uint8 presence flag per query
(0: that bound is absent, i.e. SeekToFirst / SeekToLast).

A query is the half-open user-key interval [lo, hi), a limit and a direction;
each is a fresh iterator.  Forward is Seek(lo) and Next() while key() < hi;
reverse is Seek(hi) and Prev() (SeekToLast() where Seek ends invalid) and
Prev() while key() >= lo; both stop after `limit` entries.
"""
from collections import namedtuple

from ._lib import check, lib
from .engine import (_buf, _check_tensors, _ptr, _raise_on as _raise_on_status, _require_cuda, _stream_ptr, _torch,
                     on_stream)
from .merge import MERGE_BAD_INPUT, MERGE_NO_ROOM, MERGE_OK, MERGE_UNSORTED, PlanResult, kMaxSequenceNumber
from . import merge as _merge

# per-query status (include/lsbm_iter.h)
SCAN_OK = 0
SCAN_CORRUPTION = 1

STATUS_MESSAGE = {MERGE_NO_ROOM: "output window too small",
                  MERGE_BAD_INPUT: "bad input (offsets that decrease or pass their buffer, a key shorter than 8 "
                                   "bytes, or arrays that do not belong together)",
                  MERGE_UNSORTED: "entries are not sorted"}

ViewPlan = namedtuple("ViewPlan", "source out_key_offsets counts yield_rank corrupt_rank first back status")
RangeResult = namedtuple("RangeResult", "j_begin count status key_bytes value_bytes call_status")
ScanResult = namedtuple("ScanResult", "status entry_first keys key_offsets values value_offsets")


def status_string(code):
    """Status::ToString() of an iterator's status(): "OK", or the text
    DBIter::ParseKey leaves when it meets a corrupt internal key."""
    code = int(code)
    if code == SCAN_OK:
        return "OK"
    if code == SCAN_CORRUPTION:
        return "Corruption: corrupted internal key in DBIter"
    raise ValueError(f"unknown status {code}")


def _check(**ts):
    _check_tensors(ts, u8=("keys", "lo", "hi", "lo_present", "hi_present", "value_image"))


def _raise_on(status, what):
    _raise_on_status(status, what, MERGE_OK, STATUS_MESSAGE)  # (one status word per call)


def _snapshot(snapshot):
    snapshot = int(snapshot)
    if not 0 <= snapshot <= kMaxSequenceNumber:
        raise ValueError("snapshot is a 56-bit sequence number")
    return snapshot


@on_stream
def plan(keys, key_offsets, snapshot, stream=None):
    """ViewPlan(source int64[n] = live, out_key_offsets int64[n + 1], counts
    int64[3] = {n_yield, live key bytes, corrupt entries}, yield_rank int64[n +
    1], corrupt_rank int64[n + 1], first int64[n], back int64[n], status
    int32[1]); source, out_key_offsets, first and back are used up to n_yield.
    With a status other than MERGE_OK nothing else was written (counts stay 0)."""
    torch = _torch()
    _require_cuda(keys, key_offsets)
    _check(keys=keys, key_offsets=key_offsets)
    snapshot = _snapshot(snapshot)
    n = key_offsets.numel() - 1
    if n < 0:
        raise ValueError("key_offsets needs at least one entry")
    dev = key_offsets.device
    source = _buf(n, torch.int64, dev)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    yield_rank = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    corrupt_rank = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    first = _buf(n, torch.int64, dev)
    back = _buf(n, torch.int64, dev, -1)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch_bytes = lib().lsbm_dbiter_scratch_bytes(n)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().lsbm_dbiter_plan_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), n, snapshot, _ptr(source),
                                     _ptr(out_off), _ptr(counts), _ptr(yield_rank), _ptr(corrupt_rank), _ptr(first),
                                     _ptr(back), _ptr(status), _ptr(scratch), scratch.numel() * 8,
                                     _stream_ptr(stream)), "lsbm_dbiter_plan_dev")
    return ViewPlan(source, out_off, counts, yield_rank, corrupt_rank, first, back, status)


@on_stream
def view(keys, key_offsets, values, value_image, snapshot, stream=None):
    """The SnapshotView of sorted entries at `snapshot`: plan, merge.gather of
    the live entries (plan's source / out_key_offsets / counts are a merge
    plan) and the prefix of their value lengths by torch.cumsum.  One host read
    (the status words and n_yield) follows the three.  Raises ValueError for
    entries that are not sorted or not well formed."""
    torch = _torch()
    _require_cuda(keys, key_offsets, values, value_image)
    values = values.reshape(-1)
    _check(keys=keys, key_offsets=key_offsets, values=values, value_image=value_image)
    n = key_offsets.numel() - 1
    if values.numel() != 2 * n:
        raise ValueError("values must be one {offset, length} pair per entry")
    p = plan(keys, key_offsets, snapshot)
    g = _merge.gather(keys, key_offsets, values, PlanResult(p.source, p.out_key_offsets, p.counts[:2], None))
    _raise_on(p.status, "plan")
    _raise_on(g.status, "gather")
    n_yield, key_bytes, _ = (int(x) for x in p.counts.cpu())
    live_values = g.values[:n_yield].contiguous()
    prefix = torch.zeros(n_yield + 1, dtype=torch.int64, device=keys.device)
    if n_yield:
        torch.cumsum(live_values[:, 1], 0, out=prefix[1:])
    return SnapshotView(keys, key_offsets, value_image, _snapshot(snapshot), p, g.keys[:key_bytes],
                        g.key_offsets[:n_yield + 1], live_values, prefix, n_yield)


class SnapshotView:
    """The user-visible sequence of a set of sorted entries at one snapshot.

    live_keys / live_key_offsets / live_values are the yielded entries
    (internal keys and value slices) in ascending order, n_yield of them;
    plan holds the ranks that place a query among them."""

    def __init__(self, keys, key_offsets, value_image, snapshot, plan_result, live_keys, live_key_offsets,
                 live_values, value_prefix, n_yield):
        self.keys, self.key_offsets, self.value_image, self.snapshot = keys, key_offsets, value_image, snapshot
        self.plan = plan_result
        self.live_keys, self.live_key_offsets, self.live_values = live_keys, live_key_offsets, live_values
        self.value_prefix, self.n_yield = value_prefix, n_yield
        self.n = key_offsets.numel() - 1

    def _bounds(self, lo, lo_offsets, hi, hi_offsets, lo_present, hi_present):
        torch = _torch()
        dev = self.key_offsets.device
        if (lo is None) != (lo_offsets is None) or (hi is None) != (hi_offsets is None):
            raise ValueError("a bound is a key buffer and its offsets")
        if lo_offsets is None and hi_offsets is None:
            raise ValueError("give lo or hi offsets (absent bounds are presence flags of 0): they count the queries")
        q = (lo_offsets if lo_offsets is not None else hi_offsets).numel() - 1
        if q < 0:
            raise ValueError("offsets need at least one entry")
        if lo_offsets is None:  # no query has a lower bound
            lo, lo_offsets, lo_present = _buf(0, torch.uint8, dev), torch.zeros(q + 1, dtype=torch.int64, device=dev), \
                _buf(q, torch.uint8, dev)
        _require_cuda(lo, lo_offsets, hi, hi_offsets, lo_present, hi_present)
        _check(lo=lo, lo_offsets=lo_offsets, hi=hi, hi_offsets=hi_offsets, lo_present=lo_present,
               hi_present=hi_present)
        if hi_offsets is not None and hi_offsets.numel() != q + 1:
            raise ValueError("lo_offsets and hi_offsets count different queries")
        for present in (lo_present, hi_present):
            if present is not None and present.numel() != q:
                raise ValueError("one presence flag per query")
        if hi_offsets is None and hi_present is not None:
            raise ValueError("hi_present without hi")
        return q, lo, lo_offsets, hi, hi_offsets, lo_present, hi_present

    @on_stream
    def range(self, lo=None, lo_offsets=None, hi=None, hi_offsets=None, limit=None, reverse=False, lo_present=None,
              hi_present=None, stream=None):
        """RangeResult(j_begin int64[q], count int64[q], status int32[q],
        key_bytes int64[q], value_bytes int64[q], call_status int32[1]): query
        q's window is live entries [j_begin, j_begin + count).  limit: an int,
        None for no limit, or an int64 device tensor of one limit per query."""
        torch = _torch()
        q, lo, lo_offsets, hi, hi_offsets, lo_present, hi_present = self._bounds(lo, lo_offsets, hi, hi_offsets,
                                                                                 lo_present, hi_present)
        limits = limit if hasattr(limit, "dtype") else None
        if limits is not None:
            _require_cuda(limits)
            _check(limits=limits)
            if limits.numel() != q:
                raise ValueError("one limit per query")
            if q and int(limits.min().cpu()) < 0:
                raise ValueError("limit must be >= 0")
        scalar = 0 if limits is not None else (self.n if limit is None else int(limit))
        if scalar < 0:
            raise ValueError("limit must be >= 0")
        dev = self.key_offsets.device
        j_begin, count = _buf(q, torch.int64, dev), _buf(q, torch.int64, dev)
        status = _buf(q, torch.int32, dev)
        key_bytes, value_bytes = _buf(q, torch.int64, dev), _buf(q, torch.int64, dev)
        call_status = torch.zeros(1, dtype=torch.int32, device=dev)
        p = self.plan
        check(lib().lsbm_dbiter_range_dev(
            _ptr(self.keys), self.keys.numel(), _ptr(self.key_offsets), self.n, self.snapshot, _ptr(p.source),
            _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(p.yield_rank), _ptr(p.corrupt_rank), _ptr(p.first),
            _ptr(p.back), _ptr(self.value_prefix), _ptr(lo), lo.numel(), _ptr(lo_offsets), _ptr(lo_present),
            _ptr(hi), hi.numel() if hi is not None else 0, _ptr(hi_offsets), _ptr(hi_present), q, scalar,
            _ptr(limits), 1 if reverse else 0, _ptr(j_begin), _ptr(count), _ptr(status), _ptr(key_bytes),
            _ptr(value_bytes), _ptr(call_status), _stream_ptr(stream)), "lsbm_dbiter_range_dev")
        return RangeResult(j_begin, count, status, key_bytes, value_bytes, call_status)

    @on_stream
    def emit(self, j_begin, entry_first, key_first, value_first, reverse=False, out_keys=None, out_key_offsets=None,
             out_values=None, out_value_offsets=None, totals=None, stream=None):
        """lsbm_dbiter_emit_dev: (keys, key_offsets, values, value_offsets,
        status int32[1]).  Without out_* the outputs are sized from `totals` =
        (entries, key bytes, value bytes)."""
        torch = _torch()
        dev = self.key_offsets.device
        q = entry_first.numel() - 1
        if out_keys is None:
            n_out, kb, vb = totals
            out_keys, out_values = _buf(kb, torch.uint8, dev), _buf(vb, torch.uint8, dev)
            out_key_offsets = torch.zeros(n_out + 1, dtype=torch.int64, device=dev)
            out_value_offsets = torch.zeros(n_out + 1, dtype=torch.int64, device=dev)
        _require_cuda(j_begin, entry_first, key_first, value_first, out_keys, out_key_offsets, out_values,
                      out_value_offsets)
        _check(j_begin=j_begin, entry_first=entry_first, key_first=key_first, value_first=value_first,
               out_key_offsets=out_key_offsets, out_value_offsets=out_value_offsets)
        if j_begin.numel() != q or key_first.numel() != q + 1 or value_first.numel() != q + 1:
            raise ValueError("j_begin needs one entry per query, the sums one more")
        cap = min(out_key_offsets.numel(), out_value_offsets.numel()) - 1
        if cap < 0:
            raise ValueError("the output offsets need at least one entry")
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        image = self.value_image
        check(lib().lsbm_dbiter_emit_dev(
            _ptr(j_begin), _ptr(entry_first), _ptr(key_first), _ptr(value_first), q, 1 if reverse else 0,
            _ptr(self.live_keys), self.live_keys.numel(), _ptr(self.live_key_offsets),
            _ptr(self.live_values), self.n_yield, _ptr(self.value_prefix), _ptr(image), image.numel(), _ptr(out_keys),
            out_keys.numel(), _ptr(out_key_offsets), _ptr(out_values), out_values.numel(), _ptr(out_value_offsets),
            cap, _ptr(status), _stream_ptr(stream)), "lsbm_dbiter_emit_dev")
        return out_keys, out_key_offsets, out_values, out_value_offsets, status

    @on_stream
    def scan(self, lo=None, lo_offsets=None, hi=None, hi_offsets=None, limit=None, reverse=False, lo_present=None,
             hi_present=None, stream=None):
        """ScanResult(status int32[q], entry_first int64[q + 1], keys uint8,
        key_offsets int64[total + 1], values uint8, value_offsets int64[total +
        1]): query q's entries are numbers [entry_first[q], entry_first[q + 1])
        of the output, user key and value each, ascending or (reverse)
        descending; status[q] is SCAN_OK or SCAN_CORRUPTION (status_string).
        range, three cumsums over the queries, one host read of the three
        totals (and the call's status word) to size the outputs, then emit."""
        torch = _torch()
        r = self.range(lo, lo_offsets, hi, hi_offsets, limit, reverse, lo_present, hi_present)
        q = r.count.numel()
        dev = r.count.device
        sums = torch.zeros((3, q + 1), dtype=torch.int64, device=dev)
        if q:
            torch.cumsum(r.count, 0, out=sums[0, 1:])
            torch.cumsum(r.key_bytes, 0, out=sums[1, 1:])
            torch.cumsum(r.value_bytes, 0, out=sums[2, 1:])
        head = torch.cat([sums[:, -1], r.call_status.to(torch.int64)]).cpu().tolist()
        if head[3] != MERGE_OK:
            raise ValueError(f"range: {STATUS_MESSAGE.get(head[3], head[3])}")
        keys, key_offsets, values, value_offsets, st = self.emit(r.j_begin, sums[0], sums[1], sums[2], reverse,
                                                                 totals=head[:3])
        _raise_on(st, "emit")
        return ScanResult(r.status, sums[0], keys, key_offsets, values, value_offsets)

    @on_stream
    def seek(self, keys, offsets, stream=None):
        """DBIter::Seek(k) for a batch of user keys: the first yielded entry at or after each, if any."""
        return self.scan(keys, offsets, limit=1, stream=stream)

    @on_stream
    def seek_to_first(self, stream=None):
        return self._end(False, stream)

    @on_stream
    def seek_to_last(self, stream=None):
        return self._end(True, stream)

    def _end(self, reverse, stream):
        torch = _torch()
        dev = self.key_offsets.device
        return self.scan(_buf(0, torch.uint8, dev), torch.zeros(2, dtype=torch.int64, device=dev), limit=1,
                         reverse=reverse, lo_present=torch.zeros(1, dtype=torch.uint8, device=dev), stream=stream)
