"""Plain-Python restatement of lsbm's DBIter (lsbm/db_iter.cc) -- the model the
GPU range scan (include/lsbm_iter.h, lsbm_amd/scan.py) is compared with.

Two statements of the same thing:

  DBIter        a line-by-line port of the class over a Python list of
                (internal key, value): Seek, SeekToFirst, SeekToLast, Next,
                Prev, FindNextUserEntry, FindPrevUserEntry, ParseKey, status().
                scan_port() drives it through the two idioms of a range query.
  view() / scan_closed()
                the closed form the kernels compute: the flags of every merged
                position, the view arrays, and a query's window and status from
                two lower bounds.

tests/test_scan.py pins the port to the reference's own results
(tests/golden/scan_fixture.json) and the closed form to the port.

The idioms, for the half-open user-key interval [lo, hi) and a limit:

  forward   Seek(lo) (SeekToFirst() without lo), then
            while n < limit and Valid() and key() < hi: take; n += 1;
                if n == limit: stop; Next()
  reverse   Seek(hi), then Prev() if Valid() else SeekToLast()
            (SeekToLast() without hi), then
            while n < limit and Valid() and key() >= lo: take; n += 1;
                if n == limit: stop; Prev()

limit 0 makes no call.  Each query is a fresh iterator.
"""
import struct

TYPE_DELETION, TYPE_VALUE = 0, 1
kMaxSequenceNumber = (1 << 56) - 1
OK, CORRUPTION = 0, 1
STATUS_STRING = {OK: "OK", CORRUPTION: "Corruption: corrupted internal key in DBIter"}


def ikey(user, seq, kind=TYPE_VALUE):
    return bytes(user) + struct.pack("<Q", (seq << 8) | kind)


def tag_of(key):
    return struct.unpack("<Q", key[-8:])[0]


def compare(a, b):
    """InternalKeyComparator::Compare (common/dbformat.cc:50-66) over the bytewise user comparator."""
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return -1 if ua < ub else 1
    ta, tb = tag_of(a), tag_of(b)
    return -1 if ta > tb else (1 if ta < tb else 0)


def sort_entries(entries):
    """[(internal key, value)] in the comparator's order; equal keys keep their order (the merge's tie rule)."""
    return sorted(entries, key=lambda e: (e[0][:-8], -tag_of(e[0])))


def lower_bound(entries, key):
    lo, hi = 0, len(entries)
    while lo < hi:
        mid = (lo + hi) // 2
        if compare(entries[mid][0], key) < 0:
            lo = mid + 1
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------- the port


class _ListIter:
    """The internal iterator: a position in the sorted list, len(entries) or -1 when not Valid()."""

    def __init__(self, entries):
        self.e, self.p = entries, len(entries)

    def Valid(self):
        return 0 <= self.p < len(self.e)

    def SeekToFirst(self):
        self.p = 0

    def SeekToLast(self):
        self.p = len(self.e) - 1

    def Seek(self, target):
        self.p = lower_bound(self.e, target)

    def Next(self):
        self.p += 1

    def Prev(self):
        self.p -= 1

    def key(self):
        return self.e[self.p][0]

    def value(self):
        return self.e[self.p][1]


class DBIter:
    """db_iter.cc:39-303, without the read sampling (bytes_counter_ changes no result)."""

    FORWARD, REVERSE = 0, 1

    def __init__(self, entries, sequence):
        self.iter_ = _ListIter(entries)
        self.sequence_ = sequence
        self.status_ = OK
        self.saved_key_ = b""
        self.saved_value_ = b""
        self.direction_ = self.FORWARD
        self.valid_ = False
        self.parsed = []  # the positions ParseKey ran on, in order

    def Valid(self):
        return self.valid_

    def key(self):
        return self.iter_.key()[:-8] if self.direction_ == self.FORWARD else self.saved_key_

    def value(self):
        return self.iter_.value() if self.direction_ == self.FORWARD else self.saved_value_

    def status(self):
        return self.status_  # (the list iterator's own status is always OK)

    def ParseKey(self):
        """(ok, user key, sequence, type): ParseInternalKey (common/dbformat.h)."""
        k = self.iter_.key()
        self.parsed.append(self.iter_.p)
        if len(k) < 8 or k[-8] > TYPE_VALUE:
            self.status_ = CORRUPTION
            return False, None, None, None
        return True, k[:-8], tag_of(k) >> 8, k[-8]

    def Next(self):
        assert self.valid_
        if self.direction_ == self.REVERSE:
            self.direction_ = self.FORWARD
            if not self.iter_.Valid():
                self.iter_.SeekToFirst()
            else:
                self.iter_.Next()
            if not self.iter_.Valid():
                self.valid_ = False
                self.saved_key_ = b""
                return
        else:
            self.saved_key_ = self.iter_.key()[:-8]
        self.FindNextUserEntry(True, self.saved_key_)

    def FindNextUserEntry(self, skipping, skip):
        assert self.iter_.Valid() and self.direction_ == self.FORWARD
        while True:
            ok, user, seq, kind = self.ParseKey()
            if ok and seq <= self.sequence_:
                if kind == TYPE_DELETION:
                    skip = user
                    skipping = True
                elif kind == TYPE_VALUE:
                    if skipping and user <= skip:
                        pass  # entry hidden
                    else:
                        self.valid_ = True
                        self.saved_key_ = b""
                        return
            self.iter_.Next()
            if not self.iter_.Valid():
                break
        self.saved_key_ = b""
        self.valid_ = False

    def Prev(self):
        assert self.valid_
        if self.direction_ == self.FORWARD:
            assert self.iter_.Valid()
            self.saved_key_ = self.iter_.key()[:-8]
            while True:
                self.iter_.Prev()
                if not self.iter_.Valid():
                    self.valid_ = False
                    self.saved_key_ = b""
                    self.saved_value_ = b""
                    return
                if self.iter_.key()[:-8] < self.saved_key_:
                    break
            self.direction_ = self.REVERSE
        self.FindPrevUserEntry()

    def FindPrevUserEntry(self):
        assert self.direction_ == self.REVERSE
        value_type = TYPE_DELETION
        if self.iter_.Valid():
            while True:
                ok, user, seq, kind = self.ParseKey()
                if ok and seq <= self.sequence_:
                    if value_type != TYPE_DELETION and user < self.saved_key_:
                        break
                    value_type = kind
                    if value_type == TYPE_DELETION:
                        self.saved_key_ = b""
                        self.saved_value_ = b""
                    else:
                        self.saved_key_ = self.iter_.key()[:-8]
                        self.saved_value_ = self.iter_.value()
                self.iter_.Prev()
                if not self.iter_.Valid():
                    break
        if value_type == TYPE_DELETION:
            self.valid_ = False
            self.saved_key_ = b""
            self.saved_value_ = b""
            self.direction_ = self.FORWARD
        else:
            self.valid_ = True

    def Seek(self, target):
        self.direction_ = self.FORWARD
        self.saved_value_ = b""
        self.saved_key_ = ikey(target, self.sequence_, TYPE_VALUE)
        self.iter_.Seek(self.saved_key_)
        if self.iter_.Valid():
            self.FindNextUserEntry(False, self.saved_key_)
        else:
            self.valid_ = False

    def SeekToFirst(self):
        self.direction_ = self.FORWARD
        self.saved_value_ = b""
        self.iter_.SeekToFirst()
        if self.iter_.Valid():
            self.FindNextUserEntry(False, self.saved_key_)
        else:
            self.valid_ = False

    def SeekToLast(self):
        self.direction_ = self.REVERSE
        self.saved_value_ = b""
        self.iter_.SeekToLast()
        self.FindPrevUserEntry()


def scan_port(entries, snapshot, lo=None, hi=None, limit=1 << 62, reverse=False):
    """([(user key, value)], status, parsed positions) of one query through the port."""
    it = DBIter(entries, snapshot)
    out = []
    if limit <= 0:
        return out, it.status(), it.parsed
    if not reverse:
        if lo is None:
            it.SeekToFirst()
        else:
            it.Seek(lo)
        while len(out) < limit and it.Valid() and (hi is None or it.key() < hi):
            out.append((it.key(), it.value()))
            if len(out) == limit:
                break
            it.Next()
    else:
        if hi is None:
            it.SeekToLast()
        else:
            it.Seek(hi)
            if it.Valid():
                it.Prev()
            else:
                it.SeekToLast()
        while len(out) < limit and it.Valid() and (lo is None or it.key() >= lo):
            out.append((it.key(), it.value()))
            if len(out) == limit:
                break
            it.Prev()
    return out, it.status(), it.parsed


# ---------------------------------------------------------------- the closed form


class View:
    """The snapshot view of sorted entries: what lsbm_dbiter_plan_dev writes."""

    def __init__(self, entries, snapshot):
        n = len(entries)
        self.entries, self.snapshot, self.n = entries, snapshot, n
        self.live, self.first, self.back = [], [], []
        self.yield_rank, self.corrupt_rank = [0] * (n + 1), [0] * (n + 1)
        self.flags = []
        seg, last_visible, n_corrupt = 0, -1, 0  # the last seg_start at or before p; the last visible position before p
        for p, (k, _) in enumerate(entries):
            if len(k) < 8:
                raise ValueError("BAD_INPUT")
            if p and compare(entries[p - 1][0], k) > 0:
                raise ValueError("UNSORTED")
            parses = k[-8] <= TYPE_VALUE
            visible = parses and (tag_of(k) >> 8) <= snapshot
            if p == 0 or entries[p - 1][0][:-8] != k[:-8]:
                seg = p
            head = visible and last_visible < seg
            yields = head and k[-8] == TYPE_VALUE
            self.flags.append((visible, not parses, seg == p, head, yields))
            self.yield_rank[p], self.corrupt_rank[p] = len(self.live), n_corrupt
            n_corrupt += 0 if parses else 1
            if yields:
                self.live.append(p)
                self.first.append(seg)
                self.back.append(last_visible)
            if visible:
                last_visible = p
        self.yield_rank[n] = len(self.live)
        self.corrupt_rank[n] = n_corrupt
        self.n_yield = len(self.live)

    def corrupt_in(self, lo, hi):
        return hi > lo and self.corrupt_rank[hi] > self.corrupt_rank[lo]


def scan_closed(view, lo=None, hi=None, limit=1 << 62, reverse=False):
    """(j_begin, count, status) of one query: the window live[j_begin, j_begin +
    count), returned last first by a reverse scan, and whether ParseKey met a
    corrupt entry.  The arithmetic of iter_range_kernel."""
    v, n, ny, s = view, view.n, view.n_yield, view.snapshot
    p_lo = 0 if lo is None else lower_bound(v.entries, ikey(lo, s))
    p_hi = n if hi is None else lower_bound(v.entries, ikey(hi, s))
    j_lo, j_hi = v.yield_rank[p_lo], v.yield_rank[p_hi]
    if limit <= 0:
        return j_lo, 0, OK
    limit = min(limit, n) if n else limit
    count = min(limit, max(0, j_hi - j_lo))
    if not reverse:
        # ParseKey runs on [p_lo, stop): up to the yield the iterator rests on, the one that fails key() < hi included
        jl = max(j_lo, min(j_lo + limit - 1, j_hi))
        stop = v.live[jl] + 1 if jl < ny else n
        return j_lo, count, CORRUPTION if v.corrupt_in(p_lo, stop) else OK
    corrupt = False
    upper = n
    if hi is not None and j_hi < ny:  # Seek(hi) ends valid; Prev() then steps over its user key without ParseKey
        corrupt = v.corrupt_in(p_hi, v.live[j_hi] + 1)
        upper = v.first[j_hi]
    elif hi is not None:  # Seek(hi) walks off the end, then SeekToLast()
        corrupt = v.corrupt_in(p_hi, n)
    # the yield the iterator rests on at the end: the limit-th, or the one that fails key() >= lo
    jt = min(j_hi - 1, max(j_hi - limit, j_lo - 1))
    lower = 0
    if jt >= 0 and v.back[jt] >= 0:
        lower = v.back[jt]
    corrupt = corrupt or v.corrupt_in(lower, upper)
    return j_hi - count, count, CORRUPTION if corrupt else OK


def scan_entries(view, j_begin, count, reverse=False):
    """[(user key, value)] of a window."""
    js = range(j_begin, j_begin + count)
    out = [(view.entries[view.live[j]][0][:-8], view.entries[view.live[j]][1]) for j in js]
    return out[::-1] if reverse else out
