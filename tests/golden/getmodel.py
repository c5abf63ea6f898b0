"""Plain-Python restatement of lsbm's read path: LookupKey (common/dbformat.cc),
MemTable::Get (common/memtable.cc:109-144), FindFile with the tests beside it
(lsbm/version_set.cc:130-150, :364-379), Table::InternalGet / ContainKey /
SkipFilterGet (table/table.cc:309-416) with the filter probe
(table/filter_block.cc:95-109, util/bloom.cc:65-89), SaveValue and the switch
after it (lsbm/version_set.cc:227-240, :392-407) -- the model the GPU Get
(include/lsbm_get.h, lsbm_amd/db.py) is compared with.  tests/test_db_get.py
pins it to the reference's own results (tests/golden/get_fixture.json,
get_tables.bin).

Verdicts and states are those of include/lsbm_get.h.
"""
import struct

from golden import blockmodel as bm
from golden import buildmodel as bd
from golden import snappytablemodel as stm
from golden.blockmodel import INTERNAL_KEY
from golden.memtablemodel import bloom_hash

UNDECIDED, FOUND, DELETED, CORRUPT, ERROR = 0, 1, 2, 3, 16
VALID, NOT_VALID, BAD_ENTRY, BAD_CONTENTS, BAD_HANDLE = 0, 1, 2, 3, 4
FILTERED, BAD_CHECKSUM, BAD_TYPE, BAD_COMPRESSED = 6, 7, 8, 9
RUN_LEVEL0, RUN_PRECHECKED = 1, 2
STATE_MESSAGE = {BAD_ENTRY: "bad entry in block", BAD_CONTENTS: "bad block contents", BAD_HANDLE: "bad block handle",
                 BAD_CHECKSUM: "block checksum mismatch", BAD_TYPE: "bad block type",
                 BAD_COMPRESSED: "corrupted compressed block contents"}
# ReadBlock's status -> the state of the Get that ran into it (lsbm_amd/sstable.py)
READ_STATE = {stm.READ_OK: VALID, stm.READ_TRUNCATED: BAD_HANDLE, stm.READ_BAD_CHECKSUM: BAD_CHECKSUM,
              stm.READ_BAD_COMPRESSED: BAD_COMPRESSED, stm.READ_BAD_TYPE: BAD_TYPE,
              stm.READ_TOO_LARGE: BAD_COMPRESSED}
TYPE_DELETION, TYPE_VALUE = 0, 1


def lookup_key(user_key, sequence):
    """LookupKey::internal_key(): user key || fixed64(seq << 8 | kValueTypeForSeek)."""
    return bytes(user_key) + struct.pack("<Q", ((sequence << 8) | TYPE_VALUE) & ((1 << 64) - 1))


def status_string(verdict, user_key=b""):
    """Status::ToString() of DB::Get's result."""
    if verdict == FOUND:
        return "OK"
    if verdict in (UNDECIDED, DELETED):
        return "NotFound: "
    if verdict == CORRUPT:
        # (Status joins its two messages with ": ")
        return "Corruption: corrupted key for : " + bytes(user_key).decode("latin-1")
    return "Corruption: " + STATE_MESSAGE[verdict - ERROR]


# ---------------------------------------------------------------- the memtable


def memtable_seek(entries, ikey):
    """The index of the first entry of the sorted memtable [(internal key,
    value)] that is not before ikey (a binary search), or len(entries)."""
    lo, hi = 0, len(entries)
    while lo < hi:
        mid = (lo + hi) // 2
        if bm.compare(entries[mid][0], ikey, INTERNAL_KEY) < 0:
            lo = mid + 1
        else:
            hi = mid
    return lo


def memtable_get(entries, user_key, sequence):
    """MemTable::Get: (verdict, value or None)."""
    at = memtable_seek(entries, lookup_key(user_key, sequence))
    if at < len(entries) and entries[at][0][:-8] == bytes(user_key):
        kind = entries[at][0][-8]
        if kind == TYPE_VALUE:
            return FOUND, entries[at][1]
        if kind == TYPE_DELETION:
            return DELETED, None
    return UNDECIDED, None


# ---------------------------------------------------------------- the file pick


def find_file(largest, ikey):
    """FindFile: the least i with icmp(largest[i], ikey) >= 0, or len(largest)."""
    left, right = 0, len(largest)
    while left < right:
        mid = (left + right) // 2
        if bm.compare(largest[mid], ikey, INTERNAL_KEY) < 0:
            left = mid + 1
        else:
            right = mid
    return right


def pick(bounds, flags, ikey, visible=None):
    """The file a run offers: its position in bounds [(smallest, largest)], or
    -1.  A sorted run: FindFile, user_key >= smallest.user_key(), visible.  A
    LEVEL0 run (at most one file): smallest.user_key() <= user_key <=
    largest.user_key()."""
    user = ikey[:-8]
    if not bounds:
        return -1
    if flags & RUN_LEVEL0:
        assert len(bounds) == 1
        return 0 if bounds[0][0][:-8] <= user <= bounds[0][1][:-8] else -1
    i = find_file([g for _, g in bounds], ikey)
    if i < len(bounds) and user >= bounds[i][0][:-8] and (visible is None or visible[i]):
        return i
    return -1


# ---------------------------------------------------------------- one table


def key_may_match(key, filt, bits_per_key, bloom_bits_use=15):
    """BloomFilterPolicy(bits_per_key)::KeyMayMatch (util/bloom.cc:65-89)."""
    if len(filt) < 2:
        return False
    bits = (len(filt) - 1) * 8
    raw = bloom_bits_use if 0 < bloom_bits_use < bits_per_key else bits_per_key
    k_use = int(raw * 0.69)
    stored = filt[-1] - 256 if filt[-1] >= 128 else filt[-1]  # (a char compared with a size_t)
    k = k_use if (stored & ((1 << 64) - 1)) > k_use else stored
    if k > 30:
        return True
    h = bloom_hash(key)
    delta = ((h >> 17) | (h << 15)) & 0xFFFFFFFF
    for _ in range(k):
        pos = h % bits
        if not filt[pos // 8] & (1 << (pos % 8)):
            return False
        h = (h + delta) & 0xFFFFFFFF
    return True


def filter_block_may_match(block, block_offset, key, bits_per_key):
    """FilterBlockReader(block).KeyMayMatch(block_offset, key)."""
    n = len(block)
    if n < 5:
        return True
    base_lg = block[n - 1]
    last = struct.unpack_from("<I", block, n - 5)[0]
    if last > n - 5:
        return True
    num = (n - 5 - last) // 4
    index = block_offset >> base_lg if base_lg < 64 else 0
    if index < num:
        start, limit = struct.unpack_from("<II", block, last + 4 * index)
        if start <= limit <= last:
            return key_may_match(key, block[start:limit], bits_per_key)
        if start == limit:
            return False
    return True


def open_table(data, bits_per_key, uncompress, verify=True):
    """Table::Open as lsbm_amd.db.Version does it: a dict with the index block's
    contents and the filter block's (None without a filter policy or without a
    filter block).  A block that does not read raises ValueError."""
    meta_handle, index_handle = stm.decode_footer(data)

    def read(h, what):
        st, contents, _ = stm.read_block(data, h, uncompress, verify)
        if st != stm.READ_OK:
            raise ValueError(what)
        return contents

    table = {"data": data, "index": read(index_handle, "index block"), "filter": None, "bits_per_key": bits_per_key}
    if bits_per_key is not None:
        meta = read(meta_handle, "metaindex block")
        for k, vo, vl, _ in bm.walk(meta)[1]:
            if k == bd.FILTER_KEY:
                h = bm.decode_handle(bytes(meta[vo:vo + vl]))
                if h is not None:
                    table["filter"] = read(h, "filter block")
    return table


def table_get(table, ikey, uncompress, verify=True, prechecked=False):
    """Table::InternalGet, or with prechecked ContainKey followed by
    SkipFilterGet: (state, found key or None, value or None).  The saver is
    called iff the state is VALID."""
    idx = bm.seek(table["index"], ikey, INTERNAL_KEY, value_is_handle=True)
    state = idx["state"]
    if state in (BAD_ENTRY, BAD_CONTENTS):
        return (NOT_VALID if prechecked else state), None, None
    if state == NOT_VALID:
        return NOT_VALID, None, None
    if state == VALID and table["filter"] is not None and \
            not filter_block_may_match(table["filter"], idx["handle"][0], ikey[:-8], table["bits_per_key"]):
        return FILTERED, None, None
    if state == BAD_HANDLE:
        return BAD_HANDLE, None, None
    st, contents, _ = stm.read_block(table["data"], idx["handle"], uncompress, verify)
    if st != stm.READ_OK:
        return READ_STATE[st], None, None
    dat = bm.seek(contents, ikey, INTERNAL_KEY)
    if dat["state"] != VALID:
        return dat["state"], None, None
    vo, vl = dat["value_offset"], dat["value_length"]
    return VALID, dat["key"], bytes(contents[vo:vo + vl])


def save_value(state, found_key, value, user_key):
    """SaveValue and the switch after the table read: (verdict, value)."""
    if state in (NOT_VALID, FILTERED):
        return UNDECIDED, None
    if state != VALID:
        return ERROR + state, None
    if len(found_key) < 8 or found_key[-8] > TYPE_VALUE:  # ParseInternalKey
        return CORRUPT, None
    if found_key[:-8] != bytes(user_key):
        return UNDECIDED, None
    return (FOUND, value) if found_key[-8] == TYPE_VALUE else (DELETED, None)


# ---------------------------------------------------------------- a version


def for_levels(level0_deletion, level0_insertion, levels):
    """The probe list of Version::Get with empty buffers: [(files, flags)] over
    files given as (number, ...) tuples; Level 0's deletion part newest first."""
    runs = [([f], RUN_LEVEL0) for f in sorted(level0_deletion, key=lambda f: -f[0])]
    runs.append((list(level0_insertion), 0))
    for deletion, insertion in levels:
        runs.append((list(deletion), RUN_PRECHECKED))
        runs.append((list(insertion), RUN_PRECHECKED))
    return runs


def version_get(memtables, tables, bounds, runs, user_key, sequence, uncompress, verify=True, visible=None):
    """DB::Get: (verdict, value or None, where).  memtables: sorted [(internal
    key, value)] lists, probed in order; tables: open_table results; bounds:
    [(smallest, largest)] per table; runs: [(table indices, flags)]; where: the
    memtable's index, len(memtables) + the run's index, or -1."""
    for i, mem in enumerate(memtables):
        verdict, value = memtable_get(mem, user_key, sequence)
        if verdict != UNDECIDED:
            return verdict, value, i
    ikey = lookup_key(user_key, sequence)
    for r, (files, flags) in enumerate(runs):
        at = pick([bounds[f] for f in files], flags, ikey, None if visible is None else [visible[f] for f in files])
        if at < 0:
            continue
        state, found, value = table_get(tables[files[at]], ikey, uncompress, verify, bool(flags & RUN_PRECHECKED))
        verdict, value = save_value(state, found, value, user_key)
        if verdict != UNDECIDED:
            return verdict, value, len(memtables) + r
    return UNDECIDED, None, -1
