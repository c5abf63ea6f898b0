"""Plain-Python model of the write path the GPU engine replaces
(include/lsbm_write.h): a transcript, line for line, of

    common/write_batch.cc:98-109      WriteBatch::Put / Delete
    util/coding.cc                    PutVarint32, PutLengthPrefixedSlice
    common/write_batch.cc:141-145     WriteBatchInternal::Append
    common/write_batch.cc:86-96       SetSequence / SetCount
    lsbm/db_impl.cc:1396-1441         DBImpl::BuildBatchGroup
    lsbm/db_impl.cc:1338-1343, 1372   DBImpl::Write's sequence arithmetic
    common/log_writer.cc:27-100       log::Writer::AddRecord / EmitPhysicalRecord

An op is (type, key, value) with type 1 for Put and 0 for Delete; a writer is
(ops, sync).  Test infrastructure only.
"""
import struct

kBlockSize, kHeaderSize = 32768, 7
kFullType, kFirstType, kMiddleType, kLastType = 1, 2, 3, 4
kHeader = 12


def put_varint32(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def put_length_prefixed_slice(s):
    return put_varint32(len(s)) + bytes(s)


class WriteBatch:
    def __init__(self):
        self.rep = bytearray(kHeader)  # Clear()

    def count(self):
        return struct.unpack_from("<I", self.rep, 8)[0]

    def set_count(self, n):
        struct.pack_into("<I", self.rep, 8, n & 0xFFFFFFFF)

    def sequence(self):
        return struct.unpack_from("<Q", self.rep, 0)[0]

    def set_sequence(self, seq):
        struct.pack_into("<Q", self.rep, 0, seq & ((1 << 64) - 1))

    def put(self, key, value):
        self.set_count(self.count() + 1)
        self.rep.append(1)  # kTypeValue
        self.rep += put_length_prefixed_slice(key)
        self.rep += put_length_prefixed_slice(value)

    def delete(self, key):
        self.set_count(self.count() + 1)
        self.rep.append(0)  # kTypeDeletion
        self.rep += put_length_prefixed_slice(key)

    def append(self, src):  # WriteBatchInternal::Append
        self.set_count(self.count() + src.count())
        self.rep += src.rep[kHeader:]

    def byte_size(self):
        return len(self.rep)


def batch_of(ops):
    b = WriteBatch()
    for t, k, v in ops:
        if t:
            b.put(k, v)
        else:
            b.delete(k)
    return b


def op_bytes(op):
    t, k, v = op
    return 1 + len(put_varint32(len(k))) + len(k) + (len(put_varint32(len(v))) + len(v) if t else 0)


def build_batch_group(sizes, syncs, first):
    """BuildBatchGroup over writers_[first:] given each batch's ByteSize: the
    index of *last_writer.  (Every batch is non-NULL.)"""
    size = sizes[first]
    max_size = 1 << 20
    if size <= (128 << 10):
        max_size = size + (128 << 10)
    last = first
    for w in range(first + 1, len(sizes)):
        if syncs[w] and not syncs[first]:
            break
        size += sizes[w]
        if size > max_size:
            break
        last = w
    return last


def groups(sizes, syncs=None):
    """group_first (n_groups + 1 entries) of the queue drained by DBImpl::Write."""
    syncs = syncs if syncs is not None else [False] * len(sizes)
    first, out = 0, []
    while first < len(sizes):
        out.append(first)
        first = build_batch_group(sizes, syncs, first) + 1
    return out + [len(sizes)]


def group_rep(batches, sequence):
    """What the leader passes to AddRecord / InsertInto: its own batch when it
    is alone, tmp_batch_ = Append(first) + Append(each follower) otherwise."""
    if len(batches) == 1:
        result = WriteBatch()
        result.rep = bytearray(batches[0].rep)
    else:
        result = WriteBatch()  # tmp_batch_, cleared
        for b in batches:
            result.append(b)
    result.set_sequence(sequence)
    return result


def write(writers, last_sequence=0, group_first=None):
    """DBImpl::Write of every queued writer: (reps, group_first, group_sync,
    sequences, counts, last_sequence).  writers: [(ops, sync)].  With
    group_first the cut is given instead of BuildBatchGroup's."""
    batches = [batch_of(ops) for ops, _ in writers]
    syncs = [bool(s) for _, s in writers]
    if group_first is None:
        group_first = groups([b.byte_size() for b in batches], syncs)
    reps, seqs, counts = [], [], []
    for g in range(len(group_first) - 1):
        updates = group_rep(batches[group_first[g]:group_first[g + 1]], last_sequence + 1)
        last_sequence += updates.count()
        reps.append(bytes(updates.rep))
        seqs.append(updates.sequence())
        counts.append(updates.count())
    return reps, group_first, [syncs[f] for f in group_first[:-1]], seqs, counts, last_sequence


def add_records(payloads, log_offset=0, crc=None):
    """log::Writer::AddRecord of every payload onto a log that holds log_offset
    bytes: (appended bytes, header offsets relative to them, fragments per
    record, end offset).  crc(bytes) -> the masked CRC of type byte + payload
    (None: the four bytes stay zero)."""
    out, heads, frags = bytearray(), [], []
    block_offset = log_offset % kBlockSize
    for p in payloads:
        p = bytes(p)
        ptr, left, begin, n = 0, len(p), True, 0
        while True:
            leftover = kBlockSize - block_offset
            if leftover < kHeaderSize:
                if leftover > 0:
                    out += bytes(leftover)
                block_offset = 0
            avail = kBlockSize - block_offset - kHeaderSize
            fragment_length = left if left < avail else avail
            end = left == fragment_length
            t = (kFullType if end else kFirstType) if begin else (kLastType if end else kMiddleType)
            payload = p[ptr:ptr + fragment_length]
            c = crc(bytes([t]) + payload) if crc else 0
            heads.append(len(out))
            out += struct.pack("<IBBB", c, fragment_length & 0xFF, fragment_length >> 8, t) + payload
            block_offset += kHeaderSize + fragment_length
            ptr += fragment_length
            left -= fragment_length
            begin = False
            n += 1
            if left <= 0:
                break
        frags.append(n)
    return bytes(out), heads, frags, log_offset + len(out)


def memtable_iteration(reps):
    """What MemTable::NewIterator() yields after InsertInto of every rep:
    [(internal key, value)], through the memtable model."""
    from golden import memtablemodel as mt
    buf, recs = b"", []
    for r in reps:
        recs.append((len(buf), len(r)))
        buf += r
    got, statuses, _ = mt.entries(buf, recs)
    assert statuses == [mt.OK] * len(recs)
    return got
