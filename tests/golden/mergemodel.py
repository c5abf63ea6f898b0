"""Plain-Python restatement of the middle of lsbm's DoCompactionWork: the
MergingIterator over sorted runs (table/merger.cc:155-168 FindSmallest), the
comparators (util/comparator.cc, common/dbformat.cc:50-66), the drop rule
(lsbm/db_impl.cc:999-1032) and the output-file cut (lsbm/db_impl.cc:1056-1064)
-- the model the GPU compaction merge (include/lsbm_merge.h) is compared with.
tests/test_merge.py pins the merge to the reference's own results
(tests/golden/merge_fixture.json, merge_tables.bin), the pairwise drop rule to
the sequential loop below and to a snapshot-visibility property, and the cut to
an entry-by-entry emulation over buildmodel.

Statuses are those of include/lsbm_merge.h.
"""
import struct

from golden import buildmodel as bd
from golden.blockmodel import BYTEWISE, INTERNAL_KEY

OK, NO_ROOM, BAD_INPUT, UNSORTED = 0, 1, 2, 3
MAX_SEQ = (1 << 56) - 1  # kMaxSequenceNumber
TYPE_DELETION, TYPE_VALUE = 0, 1


def internal_key(user, seq, typ=TYPE_VALUE):
    return user + struct.pack("<Q", (seq << 8) | typ)


def tag_of(key):
    return struct.unpack("<Q", key[-8:])[0]


def compare(a, b, cmp):
    """Comparator::Compare: < 0, 0, > 0."""
    if cmp == INTERNAL_KEY:
        ua, ub = a[:-8], b[:-8]
        if ua != ub:
            return -1 if ua < ub else 1
        ta, tb = tag_of(a), tag_of(b)
        return -1 if ta > tb else (1 if ta < tb else 0)  # the tag descending
    return -1 if a < b else (1 if a > b else 0)


def run_status(keys, cmp):
    """A run's status: a key too short for its comparator, or a pair out of order."""
    st = OK
    for i, k in enumerate(keys):
        if cmp == INTERNAL_KEY and len(k) < 8:
            st = max(st, BAD_INPUT)
        elif i + 1 < len(keys) and not (cmp == INTERNAL_KEY and len(keys[i + 1]) < 8) \
                and compare(k, keys[i + 1], cmp) > 0:
            st = max(st, UNSORTED)
    return st


def merge(runs, cmp):
    """MergingIterator: SeekToFirst, then key() / Next() until !Valid().  runs:
    [[key]].  Returns [(run, position)] in merged order.  FindSmallest replaces
    its candidate only on a strict Compare < 0, so among equal keys the
    lowest-numbered child wins."""
    at = [0] * len(runs)
    out = []
    while True:
        smallest = None
        for r, run in enumerate(runs):
            if at[r] < len(run) and (smallest is None
                                     or compare(run[at[r]], runs[smallest][at[smallest]], cmp) < 0):
                smallest = r
        if smallest is None:
            return out
        out.append((smallest, at[smallest]))
        at[smallest] += 1


def parse(key):
    """ParseInternalKey: (user, seq, type), or None for an error key."""
    if len(key) < 8:
        return None
    t = tag_of(key)
    return (key[:-8], t >> 8, t & 0xFF) if (t & 0xFF) <= TYPE_VALUE else None


def drop_sequential(keys, smallest_snapshot, bottom_level):
    """lsbm/db_impl.cc:999-1032 line by line over internal keys in merged
    order: [drop]."""
    out = []
    current_user_key, has_current_user_key, last_sequence_for_key = b"", False, MAX_SEQ
    for key in keys:
        drop = False
        ikey = parse(key)
        if ikey is None:
            current_user_key = b""
            has_current_user_key = False
            last_sequence_for_key = MAX_SEQ
        else:
            user, seq, typ = ikey
            if not has_current_user_key or user != current_user_key:
                current_user_key = user
                has_current_user_key = True
                last_sequence_for_key = MAX_SEQ
            if last_sequence_for_key <= smallest_snapshot:
                drop = True
            elif typ == TYPE_DELETION and seq <= smallest_snapshot and bottom_level:
                drop = True
            last_sequence_for_key = seq
        out.append(drop)
    return out


def drop_pairwise(keys, smallest_snapshot, bottom_level):
    """The same rule from each position's immediate predecessor alone."""
    out = []
    for p, key in enumerate(keys):
        ikey = parse(key)
        if ikey is None:
            out.append(False)
            continue
        user, seq, typ = ikey
        prev = parse(keys[p - 1]) if p else None
        first = prev is None or prev[0] != user
        last_seq = MAX_SEQ if first else prev[1]
        out.append(last_seq <= smallest_snapshot
                   or (typ == TYPE_DELETION and seq <= smallest_snapshot and bool(bottom_level)))
    return out


def merge_entries(runs, cmp, drop=False, smallest_snapshot=0, bottom_level=False):
    """runs: [[(key, value)]].  ([(key, value)] of the output, [source index in
    the runs laid back to back])."""
    order = merge([[k for k, _ in run] for run in runs], cmp)
    base = [0]
    for run in runs:
        base.append(base[-1] + len(run))
    keys = [runs[r][i][0] for r, i in order]
    dropped = drop_pairwise(keys, smallest_snapshot, bottom_level) if drop else [False] * len(order)
    kept = [(r, i) for (r, i), d in zip(order, dropped) if not d]
    return [runs[r][i] for r, i in kept], [base[r] + i for r, i in kept]


def visible(keys_values, user, snapshot):
    """What a Get(user) at `snapshot` reads from entries in internal-key order:
    the first entry of `user` with seq <= snapshot -- its value, or None for a
    deletion or for no entry."""
    for key, value in keys_values:
        ikey = parse(key)
        if ikey is not None and ikey[0] == user and ikey[1] <= snapshot:
            return value if ikey[2] == TYPE_VALUE else None
    return None


def cut_tables(block_first, block_bytes, max_file_size):
    """The cut over a single-table plan: (table_first, table_block_first)."""
    table_first, table_block_first, size = [block_first[0]], [0], 0
    for b, nbytes in enumerate(block_bytes):
        size += nbytes + 5
        if size >= max_file_size or b + 1 == len(block_bytes):
            table_first.append(block_first[b + 1])
            table_block_first.append(b + 1)
            size = 0
    return table_first, table_block_first


def cut_emulation(entries, block_size, restart_interval, max_file_size):
    """DoCompactionWork's output loop entry by entry: builder->Add (the body of
    buildmodel.plan's loop, one entry at a time), then "close the file once
    builder->FileSize() >= MaxOutputFileSize()", where TableBuilder::FileSize()
    is the offset that only a Flush advances, by the block and its trailer.
    entries: [(key, value length)].  Returns (first entry of each table + [n],
    [per table: (first entry of each block + [end], block sizes)])."""
    table_first, tables = [0], []
    state = {}

    def open_table():
        state.update(first=[], sizes=[], offset=0)
        open_block()

    def open_block():
        state.update(buf=0, restarts=1, counter=0, last=b"", n_in=0)

    def estimate():
        return state["buf"] + 4 * state["restarts"] + 4

    def flush():
        state["sizes"].append(estimate())
        state["offset"] += estimate() + 5
        open_block()

    def finish(end):  # TableBuilder::Finish: Flush what is left
        if state["n_in"]:
            flush()
        tables.append((state["first"] + [end], state["sizes"]))
        table_first.append(end)
        open_table()

    open_table()
    for i, (key, vlen) in enumerate(entries):
        if state["n_in"] == 0:
            state["first"].append(i)
        shared = 0
        if state["counter"] < restart_interval:
            shared = bd.shared_prefix(state["last"], key)
        else:
            state["restarts"] += 1
            state["counter"] = 0
        ns = len(key) - shared
        state["buf"] += bd.varint_len(shared) + bd.varint_len(ns) + bd.varint_len(vlen) + ns + vlen
        state["last"] = key
        state["counter"] += 1
        state["n_in"] += 1
        if estimate() >= block_size:
            flush()
        if state["offset"] >= max_file_size:
            finish(i + 1)
    if state["first"]:
        finish(len(entries))
    return table_first, tables


def compact(runs, cmp, max_file_size, drop=False, smallest_snapshot=0, bottom_level=False, block_size=4096,
            restart_interval=16, bits_per_key=None):
    """The output table files: [bytes]."""
    entries, _ = merge_entries(runs, cmp, drop, smallest_snapshot, bottom_level)
    first, sizes = bd.plan([(k, len(v)) for k, v in entries], block_size, restart_interval)
    table_first, _ = cut_tables(first, sizes, max_file_size)
    return [bd.table_file(entries[table_first[t]:table_first[t + 1]], cmp, block_size, restart_interval,
                          bits_per_key)[0] for t in range(len(table_first) - 1)]
