"""Plain-Python restatement of LSbM's range read over the sorted-table lists:
Version::RangeQuery (lsbm/version_set.cc:1043-1214) line by line over
buffermodel's ModelVersion, and TableCache::GetRange / Table::InternalGetRange
(table/table.cc:340-368) over the two-level iterator -- the model the GPU's
range query (include/lsbm_range.h, lsbm_amd/rangequery.py) is compared with.
tests/test_range_query.py pins it to the reference's own results
(tests/golden/range_fixture.json, range_tables.bin).

Beside the literal model stands the rule the device runs: rule_plan() picks a
query's files from the slots of rangequery.layout_range_slots, as the header
states it.  test_range_query.py holds the two equal on random trees.
"""
import struct

from golden import blockmodel as bm
from golden import buffermodel as bfm
from golden import snappytablemodel as stm
from golden.blockmodel import INTERNAL_KEY

kNumLevels = 4
DELETION_PART, INSERTION_PART, COMPACTION_BUFFER, WARMINGUP_BUFFER = 0, 1, 2, 3
RSLOT_ALL, RSLOT_L0INS, RSLOT_WB, RSLOT_DEL, RSLOT_CB, RSLOT_INS = range(6)
RANGE_COVERS, RANGE_SOLE, RANGE_LAST = 1, 2, 1


class RangeParams(bfm.Params):
    """bfm.Params and runtime::read_upto_key_."""

    def __init__(self, use_length=(0, 0, 0, 0), buffered_merge=False, read_cursor_keys=(b"", b"", b"", b""),
                 read_upto_key=b""):
        super().__init__(use_length, buffered_merge, read_cursor_keys)
        self.read_upto_key = bytes(read_upto_key)


def lookup_key(user_key, sequence):
    return bytes(user_key) + struct.pack("<Q", (sequence << 8) | 1)


def find_file(files, key):
    """FindFile (:130-150) with whatever key it is handed: RangeQuery hands it
    the user key `start`, whose last 8 bytes the comparator reads as a tag."""
    left, right = 0, len(files)
    while left < right:
        mid = (left + right) // 2
        if bm.compare(files[mid].largest, key, INTERNAL_KEY) < 0:
            left = mid + 1
        else:
            right = mid
    return right


# ---------------------------------------------------------------- Version::RangeQuery, literally


def version_range_files(v, p, start, end, trace=None):
    """The files Version::RangeQuery reads: [[FileMeta]] per level group 1..3,
    each in read order (level 0's files are in level 1's group).  trace: a set
    that collects (level, what) for the branches taken."""
    start, end = bytes(start), bytes(end)
    note = (lambda level, what: trace.add((level, what))) if trace is not None else (lambda level, what: None)
    levels_ = v.levels_
    overlaps = lambda f: end >= f.smallest[:-8] and start <= f.largest[:-8]
    tmp, groups = [], []

    def walk(table, out):
        """index = FindFile(...); push what overlaps; break after end < smallest.  True if anything was pushed."""
        pushed = False
        index = find_file(table.files_, start)
        while index < len(table.files_):
            f = table.files_[index]
            if overlaps(f):
                out.append(f)
                pushed = True
            if end < f.smallest[:-8]:
                break
            index += 1
        return pushed

    # level 0
    for f in levels_[0][DELETION_PART].files_:
        if overlaps(f):
            tmp.append(f)
    walk(levels_[0][INSERTION_PART], tmp)
    for level in range(1, kNumLevels):
        cb_covered = wb_covered = dl_covered = False
        use = p.use_length
        checkwb = p.buffered_merge and level > 1 and use[level - 1] > 0 and start > p.read_cursor_keys[level]
        tmptmp = []
        if checkwb:
            note(level, "checkwb")
            head = levels_[level][WARMINGUP_BUFFER]
            cur = head
            tablecount = 0
            while True:
                if tablecount > use[level - 1]:
                    break
                tablecount += 1
                if walk(cur, tmptmp) and cur.next is head.prev:
                    wb_covered = True
                cur = cur.next
                if cur is head:
                    break
        if wb_covered:
            note(level, "wb_covered")
            tmp += tmptmp
        else:
            if tmptmp:
                note(level, "wb_dropped")
            dl_covered = walk(levels_[level][DELETION_PART], tmp)
            note(level, "dl_covered" if dl_covered else "dl_not_covered")
        tmptmp = []
        if use[level] > 0 and not end < p.read_upto_key:
            note(level, "upto_closed")
        if use[level] > 0 and end < p.read_upto_key:
            head = levels_[level][COMPACTION_BUFFER].next
            cur = head
            tablecount = 1
            note(level, "cb_from_head")
            if wb_covered or dl_covered:
                note(level, "cb_from_next")
                tablecount = 2
                cur = head.next
            while True:
                if tablecount > use[level]:
                    break
                tablecount += 1
                if walk(cur, tmptmp) and cur.next is head.prev:
                    cb_covered = True
                cur = cur.next
                if cur is head:
                    break
        if cb_covered:
            note(level, "cb_covered")
            tmp += tmptmp
        else:
            if tmptmp:
                note(level, "cb_dropped")
            walk(levels_[level][INSERTION_PART], tmp)
        if not tmp:
            note(level, "reads_nothing")
        groups.append(tmp)
        tmp = []
    return groups


# ---------------------------------------------------------------- TableCache::GetRange


def open_range_table(data, verify=True):
    """What Table::Open keeps for iteration: the file and its index block."""
    _, index_handle = stm.decode_footer(data)
    st, contents, _ = stm.read_block(data, index_handle, None, verify)
    if st != stm.READ_OK:
        raise ValueError("index block")
    return {"data": data, "index": contents}


def table_blocks(table, verify=True):
    """[[internal key]] per data block, through the index block; None when the
    index block does not parse (the iterator is then never valid)."""
    st, idx = bm.walk(table["index"])
    if st != bm.OK:
        return None
    out = []
    for key, vo, vl, _ in idx:
        handle = bm.decode_handle(bytes(table["index"][vo:vo + vl]))
        if handle is None:
            raise ValueError("bad block handle")
        rs, contents, _ = stm.read_block(table["data"], handle, None, verify)
        if rs != stm.READ_OK:
            raise ValueError("data block")
        ds, entries = bm.walk(contents)
        if ds != bm.OK:
            raise ValueError("data block entries")
        out.append((key, [e[0] for e in entries]))
    return out


def get_range(blocks, lkstart, lkend):
    """Table::InternalGetRange over table_blocks' result: the two-level
    iterator's Seek(lkstart) -- the index block's Seek, the data block's Seek,
    then on to the next blocks while the data iterator is not valid -- and the
    count of entries until the first with ucmp(key, lkend) > 0: the bytewise
    comparator over whole internal keys."""
    if blocks is None:
        return 0
    found = 0
    b = 0
    while b < len(blocks) and bm.compare(blocks[b][0], lkstart, INTERNAL_KEY) < 0:
        b += 1
    sought = False
    while b < len(blocks):
        keys = blocks[b][1]
        i = 0
        if not sought:
            while i < len(keys) and bm.compare(keys[i], lkstart, INTERNAL_KEY) < 0:
                i += 1
            sought = True
        for key in keys[i:]:
            if key > lkend:
                return found
            found += 1
        b += 1
    return found


def range_query(v, blocks_of, p, start, end, snapshot):
    """DBImpl::RangeQuery: (found, checked, [file numbers read], [count per file read])."""
    lkstart, lkend = lookup_key(start, snapshot), lookup_key(end, snapshot)
    found, read, counts = 0, [], []
    for group in version_range_files(v, p, start, end):
        levelfound = 0
        for f in group:
            levelfound = get_range(blocks_of[f.number], lkstart, lkend)
            read.append(f.number)
            counts.append(levelfound)
        found += levelfound
    return found, len(read), read, counts


# ---------------------------------------------------------------- the rule the device runs


def structure_of(lists):
    """ModelVersion.lists() as the structure rangequery.layout_range_slots takes."""
    return {k: [[(f.number, f.file_size, f.smallest, f.largest) for f in t] for t in ts] for k, ts in lists.items()}


def wb_enabled(p):
    return [int(p.buffered_merge and level > 1 and p.use_length[level - 1] > 0) for level in range(kNumLevels)]


def walk_slot(files, find, start, end):
    """The positions in `files` ((number, size, smallest, largest) entries) one slot's walk pushes."""
    out = []
    i = 0
    if find:
        left, right = 0, len(files)
        while left < right:
            mid = (left + right) // 2
            if bm.compare(files[mid][3], start, INTERNAL_KEY) < 0:
                left = mid + 1
            else:
                right = mid
        i = right
    while i < len(files):
        c = (end > files[i][2][:-8]) - (end < files[i][2][:-8])
        if c >= 0 and start <= files[i][3][:-8]:
            out.append(i)
        if find and c < 0:
            break
        i += 1
    return out


def rule_plan(slots, use_length, wb, cursor_keys, start, end):
    """The pairs of one query as include/lsbm_range.h states them: [(slot,
    position in the slot, flag word)] in read order.  slots: RangeSlot-like
    (level, kind, flags, files, ...); cursor_keys: the four read cursor keys,
    then read_upto_key."""
    start, end = bytes(start), bytes(end)
    pairs = []
    for s, slot in enumerate(slots):
        if slot[0] == 0:
            pairs += [(s, i, 0) for i in walk_slot(slot[3], slot[1] != RSLOT_ALL, start, end)]
    for level in range(1, kNumLevels):
        mine = [s for s, slot in enumerate(slots) if slot[0] == level]
        u, w = use_length[level], use_length[level - 1]
        checkwb = bool(wb[level]) and start > bytes(cursor_keys[level])
        hits = lambda s: [(s, i, level << 8) for i in walk_slot(slots[s][3], True, start, end)]
        wb_files, wb_covered = [], False
        if checkwb:
            for j, s in enumerate(t for t in mine if slots[t][1] == RSLOT_WB):
                if j <= w:
                    h = hits(s)
                    wb_files += h
                    wb_covered = wb_covered or (bool(h) and bool(slots[s][2] & RANGE_COVERS))
        read = []
        dl_covered = False
        if wb_covered:
            read += wb_files
        else:
            for s in mine:
                if slots[s][1] == RSLOT_DEL:
                    h = hits(s)
                    read += h
                    dl_covered = bool(h)
        cb_files, cb_covered = [], False
        if u > 0 and end < bytes(cursor_keys[kNumLevels]):
            for j, s in enumerate(t for t in mine if slots[t][1] == RSLOT_CB):
                if wb_covered or dl_covered:
                    visit = u >= 2 if slots[s][2] & RANGE_SOLE else (j >= 1 and j < u)
                else:
                    visit = j < u
                if visit:
                    h = hits(s)
                    cb_files += h
                    cb_covered = cb_covered or (bool(h) and bool(slots[s][2] & RANGE_COVERS))
        if cb_covered:
            read += cb_files
        else:
            for s in mine:
                if slots[s][1] == RSLOT_INS:
                    read += hits(s)
        pairs += read
        if level == 1 and pairs or read:
            s, i, flags = pairs[-1]
            pairs[-1] = (s, i, flags | RANGE_LAST)
    return pairs
