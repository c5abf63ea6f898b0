"""Plain-Python restatement of how lsbm turns log records into a Level-0 table:
WriteBatch::Iterate (common/write_batch.cc:42-80) with GetVarint32Ptr
(util/coding.cc:112-129), MemTableInserter / MemTable::Add
(common/write_batch.cc:112-134, common/memtable.cc:83-107), the order a release
build's SkipList::Insert gives (common/skiplist.h:334-367), RecoverLogFile's
max_sequence (lsbm/db_impl.cc:456-461) and BuildTable (lsbm/builder.cc:36-48)
-- the model the GPU memtable flush (include/lsbm_memtable.h) is compared with.
tests/test_memtable.py pins it to the reference's own results
(tests/golden/memtable_fixture.json, memtable_tables.bin) and its order to an
insertion-by-insertion emulation of the skiplist rule.

Statuses are those of include/lsbm_memtable.h.
"""
import struct

from golden import buildmodel as bd
from golden import snappytablemodel as stm
from golden.blockmodel import INTERNAL_KEY

OK, TOO_SMALL, BAD_PUT, BAD_DELETE, UNKNOWN_TAG, WRONG_COUNT, BAD_INPUT, NO_ROOM = range(8)
MESSAGE = {OK: "OK", BAD_PUT: "Corruption: bad WriteBatch Put", BAD_DELETE: "Corruption: bad WriteBatch Delete",
           UNKNOWN_TAG: "Corruption: unknown WriteBatch tag", WRONG_COUNT: "Corruption: WriteBatch has wrong count"}
TYPE_DELETION, TYPE_VALUE = 0, 1
HEADER = 12
U64 = (1 << 64) - 1


def get_varint32(buf, pos, end):
    """GetVarint32Ptr: (value, next position) or None."""
    result, shift = 0, 0
    while shift <= 28 and pos < end:
        byte = buf[pos]
        pos += 1
        if byte & 128:
            result |= (byte & 127) << shift
        else:
            return (result | (byte << shift)) & 0xFFFFFFFF, pos
        shift += 7
    return None


def get_slice(buf, pos, end):
    """GetLengthPrefixedSlice: (offset, length, next position) or None."""
    got = get_varint32(buf, pos, end)
    if got is None or got[0] > end - got[1]:
        return None
    return got[1], got[0], got[1] + got[0]


def walk(buf, off=0, length=None):
    """WriteBatch::Iterate over buf[off, off + length): (status, [(type, key
    offset, key length, value offset, value length)] of the handler calls made
    before the end or the first error)."""
    length = len(buf) - off if length is None else length
    if off < 0 or length < 0 or off + length > len(buf) or length >= 1 << 32:
        return BAD_INPUT, []
    if length < HEADER:
        return TOO_SMALL, []
    count = struct.unpack_from("<I", buf, off + 8)[0]
    pos, end, calls = off + HEADER, off + length, []
    while pos < end:
        tag = buf[pos]
        pos += 1
        if tag > TYPE_VALUE:
            return UNKNOWN_TAG, calls
        key = get_slice(buf, pos, end)
        if key is None:
            return (BAD_PUT if tag == TYPE_VALUE else BAD_DELETE), calls
        pos = key[2]
        value = (pos, 0, pos)
        if tag == TYPE_VALUE:
            value = get_slice(buf, pos, end)
            if value is None:
                return BAD_PUT, calls
            pos = value[2]
        calls.append((tag, key[0], key[1], value[0], value[1]))
    return (OK if (len(calls) & 0xFFFFFFFF) == count else WRONG_COUNT), calls


def header(buf, off=0):
    """(sequence, count as the reference's int)."""
    seq, count = struct.unpack_from("<Qi", buf, off)
    return seq, count


def insert_into(buf, off=0, length=None):
    """WriteBatchInternal::InsertInto: (status, [(internal key, value, value
    offset)] in arrival order)."""
    st, calls = walk(buf, off, length)
    out = []
    if calls:
        seq = header(buf, off)[0]
        for i, (tag, ko, kl, vo, vl) in enumerate(calls):
            packed = ((((seq + i) & U64) << 8) | tag) & U64
            out.append((bytes(buf[ko:ko + kl]) + struct.pack("<Q", packed), bytes(buf[vo:vo + vl]), vo))
    return st, out


def max_sequence(buf, records):
    """RecoverLogFile's max_sequence when errors are ignored: over every record
    of at least 12 bytes, Sequence + Count - 1 in unsigned 64-bit arithmetic."""
    best = 0
    for off, length in records:
        if 0 <= off and HEADER <= length < 1 << 32 and off + length <= len(buf):
            seq, count = header(buf, off)
            best = max(best, (seq + count - 1) & U64)
    return best


def order(keys):
    """The memtable's iteration order of internal keys given in arrival order:
    [arrival index].  User key ascending, tag descending, and among equal
    internal keys the later arrival first."""
    return sorted(range(len(keys)), key=lambda i: (keys[i][:-8], -struct.unpack("<Q", keys[i][-8:])[0], -i))


def compare(a, b):
    """InternalKeyComparator::Compare."""
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return -1 if ua < ub else 1
    ta, tb = struct.unpack("<Q", a[-8:])[0], struct.unpack("<Q", b[-8:])[0]
    return -1 if ta > tb else (1 if ta < tb else 0)


def skiplist_order(keys):
    """SkipList::Insert one key at a time as a release build does it:
    FindGreaterOrEqual(key) is the first node that is not less than the key
    (an equal one included) and the new node goes in before it.  [arrival
    index] in list order."""
    nodes = []
    for i, k in enumerate(keys):
        at = 0
        while at < len(nodes) and compare(keys[nodes[at]], k) < 0:
            at += 1
        nodes.insert(at, i)
    return nodes


def entries(buf, records):
    """([(internal key, value)] in iteration order, [status per record],
    max_sequence) of one memtable over the records [(offset, length)]."""
    arrived, statuses = [], []
    for off, length in records:
        st, got = insert_into(buf, off, length)
        statuses.append(st)
        arrived += got
    keys = [k for k, _, _ in arrived]
    return [(arrived[i][0], arrived[i][1]) for i in order(keys)], statuses, max_sequence(buf, records)


def bloom_hash(data, seed=0xBC9F1D34):
    """Hash (util/hash.cc:18-49) as the reference computes it: the one to three
    tail bytes are added as `char`, signed on x86, so a tail byte >= 0x80 is
    sign-extended.  buildmodel.bloom_hash adds them unsigned, which is the same
    number only for tail bytes below 0x80; the fixture's 137-byte user keys end
    in 0x80 / 0xfe / 0xff."""
    m, M = 0xC6A4A793, 0xFFFFFFFF
    h = (seed ^ (len(data) * m)) & M
    n4 = len(data) & ~3
    for i in range(0, n4, 4):
        h = (h + struct.unpack_from("<I", data, i)[0]) & M
        h = (h * m) & M
        h ^= h >> 16
    rest = data[n4:]
    if rest:
        for i in range(len(rest) - 1, -1, -1):
            h = (h + ((rest[i] - 256 if rest[i] >= 128 else rest[i]) << (8 * i))) & M
        h = (h * m) & M
        h ^= h >> 24
    return h


def table_file(sorted_entries, block_size=4096, restart_interval=16, bits_per_key=None, compress=None):
    """BuildTable over the iteration: the file bytes, or None without entries.
    `compress` as in snappytablemodel.table_file (None: kNoCompression).  The
    table is buildmodel's with the hash above in the place of its own."""
    if not sorted_entries:
        return None
    theirs, bd.bloom_hash = bd.bloom_hash, bloom_hash
    try:
        if compress is None:
            return bd.table_file(sorted_entries, INTERNAL_KEY, block_size, restart_interval, bits_per_key)[0]
        return stm.table_file(sorted_entries, INTERNAL_KEY, block_size, restart_interval, bits_per_key, compress)[0]
    finally:
        bd.bloom_hash = theirs


# ---------------------------------------------------------------- log framing

LOG_BLOCK, LOG_HEADER = 32768, 7


def log_records(log):
    """log::Reader::ReadRecord over a cleanly framed log file: [record bytes]."""
    out, pos, parts = [], 0, None
    while pos < len(log):
        left = LOG_BLOCK - pos % LOG_BLOCK
        if left < LOG_HEADER:
            pos += left
            continue
        length, t = log[pos + 4] | log[pos + 5] << 8, log[pos + 6]
        payload = bytes(log[pos + LOG_HEADER:pos + LOG_HEADER + length])
        pos += LOG_HEADER + length
        if t == 1:
            out.append(payload)
        elif t == 2:
            parts = [payload]
        else:
            parts.append(payload)
            if t == 4:
                out.append(b"".join(parts))
                parts = None
    return out
