"""Plain-Python restatement of the write side of lsbm's table/ layer: the flush
rule of TableBuilder::Add (table/table_builder.cc:108-141) over BlockBuilder's
CurrentSizeEstimate (table/block_builder.cc:51-55), FindShortestSeparator and
FindShortSuccessor of both comparators (util/comparator.cc:29-65,
common/dbformat.cc:68-99), BlockHandle::EncodeTo, the index block, the
metaindex block, the filter block (util/hash.cc, util/bloom.cc,
table/filter_block.cc), WriteRawBlock's trailer and the footer -- the model
the GPU block builder (include/lsbm_block_build.h) is compared with.
tests/test_block_build.py pins it to the reference's own results
(tests/golden/build_fixture.json).

Statuses are those of include/lsbm_block_build.h.
"""
import struct

from golden.blockmodel import BYTEWISE, INTERNAL_KEY, build_block, put_varint

OK, NO_ROOM, BAD_INPUT, TOO_LARGE = 0, 1, 2, 3
# PackSequenceAndType(kMaxSequenceNumber, kValueTypeForSeek) as a fixed64
SEEK_TAG = struct.pack("<Q", (((1 << 56) - 1) << 8) | 1)
MAGIC = 0xDB4775248B80FB57  # table/format.h kTableMagicNumber
FILTER_KEY = b"filter.leveldb.BuiltinBloomFilter"


def varint_len(v):
    return len(put_varint(v))


def shared_prefix(a, b):
    n, m = 0, min(len(a), len(b))
    while n < m and a[n] == b[n]:
        n += 1
    return n


def plan(entries, block_size, restart_interval):
    """entries: [(key, value length)].  TableBuilder::Add's flush rule:
    ([first entry of each block] + [len(entries)], [Finish() size of each block])."""
    first, sizes = [], []
    buf, restarts, counter, last, n_in = 0, 1, 0, b"", 0
    for i, (key, vlen) in enumerate(entries):
        if n_in == 0:
            first.append(i)
        shared = 0
        if counter < restart_interval:
            shared = shared_prefix(last, key)
        else:
            restarts += 1
            counter = 0
        ns = len(key) - shared
        buf += varint_len(shared) + varint_len(ns) + varint_len(vlen) + ns + vlen
        last = key
        counter += 1
        n_in += 1
        if buf + 4 * restarts + 4 >= block_size:  # CurrentSizeEstimate() >= block_size: Flush
            sizes.append(buf + 4 * restarts + 4)
            buf, restarts, counter, last, n_in = 0, 1, 0, b"", 0
    if n_in:
        sizes.append(buf + 4 * restarts + 4)
    return first + [len(entries)], sizes


def bytewise_separator(start, limit):
    d = shared_prefix(start, limit)
    if d < min(len(start), len(limit)) and start[d] < 0xFF and start[d] + 1 < limit[d]:
        return start[:d] + bytes([start[d] + 1])
    return start


def bytewise_successor(key):
    for i, b in enumerate(key):
        if b != 0xFF:
            return key[:i] + bytes([b + 1])
    return key


def separator(start, limit, cmp):
    """FindShortestSeparator(&start, limit)."""
    if cmp == BYTEWISE:
        return bytewise_separator(start, limit)
    assert len(start) >= 8 and len(limit) >= 8
    user = start[:-8]
    tmp = bytewise_separator(user, limit[:-8])
    return tmp + SEEK_TAG if len(tmp) < len(user) and user < tmp else start


def successor(key, cmp):
    """FindShortSuccessor(&key)."""
    if cmp == BYTEWISE:
        return bytewise_successor(key)
    assert len(key) >= 8
    user = key[:-8]
    tmp = bytewise_successor(user)
    return tmp + SEEK_TAG if len(tmp) < len(user) and user < tmp else key


def encode_handle(offset, size):
    return put_varint(offset) + put_varint(size)


def index_entries(keys, block_first, handles, cmp):
    """[(index key, handle encoding)] of one table: keys are all its entries'
    keys, block b = keys[block_first[b]:block_first[b+1]], handles [(offset, size)]."""
    n = len(block_first) - 1
    out = []
    for b in range(n):
        last = keys[block_first[b + 1] - 1]
        k = separator(last, keys[block_first[b + 1]], cmp) if b + 1 < n else successor(last, cmp)
        out.append((k, encode_handle(*handles[b])))
    return out


def index_block(keys, block_first, handles, cmp):
    return build_block(index_entries(keys, block_first, handles, cmp), 1)


# ---- util/crc32c.cc, util/hash.cc, util/bloom.cc, table/filter_block.cc

_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _CRC_TABLE.append(_c)


def crc32c(data, crc=0):
    crc ^= 0xFFFFFFFF
    for b in data:
        crc = _CRC_TABLE[(crc ^ b) & 0xFF] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def trailer(block, typ=0):
    """WriteRawBlock's 5 bytes (table/table_builder.cc:245-250)."""
    crc = crc32c(bytes([typ]), crc32c(block))
    masked = (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF
    return bytes([typ]) + struct.pack("<I", masked)


def bloom_hash(data, seed=0xBC9F1D34):
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
            h = (h + (rest[i] << (8 * i))) & M
        h = (h * m) & M
        h ^= h >> 24
    return h


def create_filter(keys, bits_per_key):
    """BloomFilterPolicy::CreateFilter (util/bloom.cc:28-55)."""
    k = max(1, min(30, int(bits_per_key * 0.69)))
    bits = max(64, len(keys) * bits_per_key)
    nbytes = (bits + 7) // 8
    bits = nbytes * 8
    arr = bytearray(nbytes)
    for key in keys:
        h = bloom_hash(key)
        delta = ((h >> 17) | (h << 15)) & 0xFFFFFFFF
        for _ in range(k):
            pos = h % bits
            arr[pos // 8] |= 1 << (pos % 8)
            h = (h + delta) & 0xFFFFFFFF
    return bytes(arr) + bytes([k])


def filter_block(keys, block_first, block_start, end, bits_per_key):
    """FilterBlockBuilder: StartBlock(block_start[b]), AddKey for block b's
    keys, ..., the last Flush's StartBlock(end), Finish
    (table/filter_block.cc:22-76, table/table_builder.cc:154-156)."""
    result, offsets, pending = bytearray(), [], []

    def generate():
        offsets.append(len(result))
        if pending:
            result.extend(create_filter(pending, bits_per_key))
            pending.clear()

    for b in range(len(block_first) - 1):
        while block_start[b] // 2048 > len(offsets):
            generate()
        pending.extend(keys[block_first[b]:block_first[b + 1]])
    if len(block_first) > 1:
        while end // 2048 > len(offsets):
            generate()
    if pending:
        generate()
    array_offset = len(result)
    for o in offsets:
        result += struct.pack("<I", o)
    return bytes(result) + struct.pack("<I", array_offset) + bytes([11])


def footer(meta_handle, index_handle):
    enc = encode_handle(*meta_handle) + encode_handle(*index_handle)
    return enc + bytes(40 - len(enc)) + struct.pack("<Q", MAGIC)


def table_file(entries, cmp=INTERNAL_KEY, block_size=4096, restart_interval=16, bits_per_key=None):
    """TableBuilder: Add for every (key, value), Finish, kNoCompression.
    Returns (file bytes, [(offset, size)] of the data blocks, index handle)."""
    keys = [k for k, _ in entries]
    first, sizes = plan([(k, len(v)) for k, v in entries], block_size, restart_interval)
    out, handles = bytearray(), []

    def write(block):
        h = (len(out), len(block))
        out.extend(block + trailer(block))
        return h

    for b in range(len(sizes)):
        block = build_block(entries[first[b]:first[b + 1]], restart_interval)
        assert len(block) == sizes[b]
        handles.append(write(block))
    meta = []
    if bits_per_key is not None:
        fkeys = [k[:-8] for k in keys] if cmp == INTERNAL_KEY else keys
        fh = write(filter_block(fkeys, first, [h[0] for h in handles], len(out), bits_per_key))
        meta.append((FILTER_KEY, encode_handle(*fh)))
    meta_handle = write(build_block(meta, restart_interval))
    index_handle = write(index_block(keys, first, handles, cmp))
    out.extend(footer(meta_handle, index_handle))
    return bytes(out), handles, index_handle
