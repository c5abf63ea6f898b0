"""Memtable flush (WriteBatchInternal::InsertInto, MemTable::Add, the skiplist's
order and BuildTable of lsbm: DBImpl::RecoverLogFile / WriteLevel0Table,
lsbm/db_impl.cc:433-540) on the GPU.

Thin wrappers over include/lsbm_memtable.h and the other modules.  Device
tensors in, device tensors out; every call runs on `stream` (default:
torch's current stream; the contract is engine.py's).

    scan(image, records)               WriteBatch::Iterate of every record:
                                       entries, user-key bytes, status
    decode(image, records, ...)        the same walk written out: internal keys
                                       + key_offsets and value {offset, length}
                                       slices, and the largest sequence number
    sort(keys, key_offsets)            the memtable's iteration order as a
                                       merge.PlanResult (merge.gather gathers it)
    entries(image, records, ...)       scan + decode + sort + gather: what
                                       MemTable::NewIterator() returns
    flush(image, records, ...)         entries, then sstable.write_tables of one
                                       table: the Level-0 table file (BuildTable)
    log_records(image_host)            a log file's logical records as
                                       {offset, length} pairs, fragments
                                       assembled on the device
    recover_log(image_host, ...)       log_records, then flush
    recover(image, ...)                log.read_records, then flush: a log in
                                       device memory, torn tail and corruption
                                       reports included (RecoverLogFile)
    heights(n, rnd)                    SkipList::RandomHeight of n inserts
    cut(key_offsets, values, ...)      ApproximateMemoryUsage() after every
                                       record and where RecoverLogFile or
                                       MakeRoomForWrite ends a memtable
                                       (include/lsbm_memtable_cut.h)
    recover_all(image, ...)            recover for a log of any size: one
                                       Level-0 table per memtable
    sort_segments(keys, key_offsets, seg_first)
                                       sort over the memtables of one log, kept
                                       apart (include/lsbm_table_write.h)
    flush_many(image, records, mem_first, ...)
                                       flush of every memtable of a cut list in
                                       one chain: one scan, decode, segmented
                                       sort and gather, sstable.write_tables;
                                       recover_all goes through it

A record is image[records[2i], records[2i] + records[2i+1]): one
WriteBatch::rep_ (int64 {offset, length} pairs).  Entries are what block.decode
returns and block_build, bloom, merge and sstable.write_table read.  One call
of scan .. recover is one memtable; cut says which records go into which,
and recover_all flushes each.
"""
from collections import namedtuple

import numpy as np

from ._lib import check, lib
from .engine import _buf, _check_tensors, _ptr, _require_cuda, _stream_ptr, _torch, on_stream
from .log import kBlockSize, kFirstType, kFullType, kHeaderSize, kLastType, kMiddleType
from .merge import MERGE_OK, PlanResult
from .table import kNoCompression

# per-record status (include/lsbm_memtable.h)
WB_OK = 0
WB_TOO_SMALL = 1
WB_BAD_PUT = 2
WB_BAD_DELETE = 3
WB_UNKNOWN_TAG = 4
WB_WRONG_COUNT = 5
WB_BAD_INPUT = 6
WB_NO_ROOM = 7

# the reference's words for each (common/write_batch.cc:42-80, lsbm/db_impl.cc:440-443)
STATUS_MESSAGE = {WB_TOO_SMALL: "log record too small", WB_BAD_PUT: "bad WriteBatch Put",
                  WB_BAD_DELETE: "bad WriteBatch Delete", WB_UNKNOWN_TAG: "unknown WriteBatch tag",
                  WB_WRONG_COUNT: "WriteBatch has wrong count", WB_BAD_INPUT: "record reaches outside the image",
                  WB_NO_ROOM: "record window too small"}

DecodeResult = namedtuple("DecodeResult", "keys key_offsets values max_sequence status")
EntriesResult = namedtuple("EntriesResult", "keys key_offsets values status max_sequence")
FlushResult = namedtuple("FlushResult", "image data_handles index_handle smallest largest max_sequence status")
RecoverResult = namedtuple("RecoverResult", "flush events status")
CutResult = namedtuple("CutResult", "usage mem_first mem_usage counts state status")
RecoverAllResult = namedtuple("RecoverAllResult", "flushes mem_first events status")

# include/lsbm_memtable_cut.h
RECOVER, WRITE = 0, 1
SKIPLIST_SEED = 0xdeadbeef & 0x7fffffff
FRESH_USAGE = 4104
kMinWriteBuffer, kMaxWriteBuffer = 64 << 10, 1 << 30  # SanitizeOptions, lsbm/db_impl.cc


def _check(**ts):
    _check_tensors(ts, u8=("image", "keys"))


def _n_records(records):
    if records.numel() % 2:
        raise ValueError("records must be {offset, length} pairs")
    return records.numel() // 2


@on_stream
def scan(image, records, stream=None):
    """(counts int64[n, 2] = {entries, user-key bytes}, status int32[n])."""
    torch = _torch()
    _require_cuda(image, records)
    _check(image=image, records=records)
    n = _n_records(records)
    counts = torch.zeros((n, 2), dtype=torch.int64, device=image.device)
    status = torch.zeros(n, dtype=torch.int32, device=image.device)
    check(lib().lsbm_wb_scan_dev(_ptr(image), image.numel(), _ptr(records), n, _ptr(counts), _ptr(status),
                                 _stream_ptr(stream)), "lsbm_wb_scan_dev")
    return counts, status


def bases(counts):
    """The running sums decode takes, from a scan's counts: (entry_base,
    key_base), n + 1 each; an entry's internal key is its user key and 8 bytes."""
    torch = _torch()
    n = counts.shape[0]
    entry_base = torch.zeros(n + 1, dtype=torch.int64, device=counts.device)
    key_base = torch.zeros(n + 1, dtype=torch.int64, device=counts.device)
    if n:
        torch.cumsum(counts[:, 0], 0, out=entry_base[1:])
        torch.cumsum(counts[:, 1] + 8 * counts[:, 0], 0, out=key_base[1:])
    return entry_base, key_base


@on_stream
def decode(image, records, entry_base=None, key_base=None, keys=None, key_offsets=None, values=None, stream=None):
    """DecodeResult(keys, key_offsets, values int64[entries, 2], max_sequence
    int64[1] (the 64 bits of the unsigned number), status int32[n]).  Record
    i's entries are [entry_base[i], entry_base[i+1]).  Without entry_base /
    key_base they are the running sums of a scan's counts; without the outputs
    one device -> host read of the totals sizes them."""
    torch = _torch()
    _require_cuda(image, records, entry_base, key_base, keys, key_offsets, values)
    _check(image=image, records=records, entry_base=entry_base, key_base=key_base, keys=keys,
           key_offsets=key_offsets, values=values)
    n = _n_records(records)
    dev = image.device
    if (entry_base is None) != (key_base is None):
        raise ValueError("entry_base and key_base come together")
    if entry_base is None:
        entry_base, key_base = bases(scan(image, records, stream)[0])
    if entry_base.numel() != n + 1 or key_base.numel() != n + 1:
        raise ValueError("entry_base and key_base need n + 1 entries")
    if key_offsets is None or values is None or keys is None:
        totals = torch.stack([entry_base[-1], key_base[-1]]).cpu()
        ne, nk = int(totals[0]), int(totals[1])
        if key_offsets is None:
            key_offsets = torch.zeros(ne + 1, dtype=torch.int64, device=dev)
        if values is None:
            values = torch.zeros((max(ne, 1), 2), dtype=torch.int64, device=dev)[:ne]
        if keys is None:
            keys = torch.zeros(max(nk, 1), dtype=torch.uint8, device=dev)[:nk]
    entries_cap = min(key_offsets.numel() - 1, values.numel() // 2)
    if entries_cap < 0:
        raise ValueError("key_offsets needs at least one entry")
    max_sequence = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    check(lib().lsbm_wb_decode_dev(_ptr(image), image.numel(), _ptr(records), n, _ptr(entry_base), _ptr(key_base),
                                   _ptr(keys), keys.numel(), _ptr(key_offsets), _ptr(values), entries_cap,
                                   _ptr(max_sequence), _ptr(status), _stream_ptr(stream)), "lsbm_wb_decode_dev")
    return DecodeResult(keys, key_offsets, values, max_sequence, status)


@on_stream
def sort(keys, key_offsets, stream=None):
    """merge.PlanResult(source int64[n], out_key_offsets int64[n + 1], counts
    int64[2] = {n, key bytes}, run_status int32[1]): the memtable's iteration
    order of the internal keys -- user key ascending, tag descending, among
    equal internal keys the later entry first.  merge.gather gathers it."""
    torch = _torch()
    _require_cuda(keys, key_offsets)
    _check(keys=keys, key_offsets=key_offsets)
    n = key_offsets.numel() - 1
    if n < 0:
        raise ValueError("key_offsets needs at least one entry")
    dev = keys.device
    source = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)[:n]
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch_bytes = lib().lsbm_memtable_sort_scratch_bytes(n)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().lsbm_memtable_sort_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), n, _ptr(source), _ptr(out_off),
                                       _ptr(counts), _ptr(status), _ptr(scratch), scratch.numel() * 8,
                                       _stream_ptr(stream)), "lsbm_memtable_sort_dev")
    return PlanResult(source, out_off, counts, status)


@on_stream
def sort_segments(keys, key_offsets, seg_first, stream=None):
    """sort over the memtables of one log (lsbm_memtable_sort_segments_dev):
    segment s = entries [seg_first[s], seg_first[s + 1]) (an int64 device
    tensor that tiles the entries; empty segments are allowed).  Within a
    segment the memtable's order; the segments stay in input order.  A
    merge.PlanResult in sort's shape; a seg_first that does not tile gives
    run_status MERGE_BAD_INPUT, counts {0, 0} and leaves `source` alone."""
    torch = _torch()
    _require_cuda(keys, key_offsets, seg_first)
    _check(keys=keys, key_offsets=key_offsets, seg_first=seg_first)
    n, ns = key_offsets.numel() - 1, seg_first.numel() - 1
    if n < 0 or ns < 0:
        raise ValueError("key_offsets and seg_first need at least one entry")
    dev = keys.device
    source = _buf(n, torch.int64, dev)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch_bytes = lib().lsbm_memtable_sort_segments_scratch_bytes(n, ns)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().lsbm_memtable_sort_segments_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), n, _ptr(seg_first), ns,
                                                _ptr(source), _ptr(out_off), _ptr(counts), _ptr(status),
                                                _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_memtable_sort_segments_dev")
    return PlanResult(source, out_off, counts, status)


def max_sequence_of(t):
    """The unsigned 64-bit number in decode's max_sequence tensor."""
    return int(t.cpu()[0]) & ((1 << 64) - 1)


@on_stream
def entries(image, records, paranoid=False, stream=None):
    """What the reference's memtable holds after InsertInto of every record, in
    NewIterator()'s order: EntriesResult(keys, key_offsets, values int64[n, 2],
    status int32[records], max_sequence int).  scan, decode, sort and
    merge.gather run on one stream; the host reads the two totals that size the
    entries after the scan, and the statuses after the gather.  A record in
    error contributes the entries before its error (paranoid_checks false);
    with paranoid=True the first such record raises ValueError with the
    reference's message."""
    torch = _torch()
    from . import merge
    counts, _ = scan(image, records)
    entry_base, key_base = bases(counts)
    d = decode(image, records, entry_base, key_base)
    p = sort(d.keys, d.key_offsets)
    flat = d.values.reshape(-1)
    g = merge.gather(d.keys, d.key_offsets, flat, p)
    # the one read after the chain: how many records are in error, sort's and gather's status
    n_bad, sort_st, gather_st = torch.stack([(d.status != WB_OK).sum().to(torch.int32), p.run_status[0],
                                             g.status[0]]).cpu().tolist()
    if n_bad:  # (only then the statuses themselves)
        status = d.status.cpu().tolist()
        for r, st in enumerate(status):
            if st in (WB_BAD_INPUT, WB_NO_ROOM) or (paranoid and st != WB_OK):
                raise ValueError(f"record {r}: {STATUS_MESSAGE.get(st, st)}")
    if sort_st != MERGE_OK or gather_st != MERGE_OK:
        raise ValueError(f"internal error: sort status {sort_st}, gather status {gather_st}")
    return EntriesResult(g.keys, g.key_offsets, g.values, d.status, max_sequence_of(d.max_sequence))


@on_stream
def flush(image, records, compression=kNoCompression, block_size=4096, restart_interval=16, bits_per_key=None,
          paranoid=False, stream=None):
    """BuildTable (lsbm/builder.cc:36-48) over the memtable of `records`:
    FlushResult(image, data_handles, index_handle, smallest, largest,
    max_sequence, status).  image is the Level-0 table file (a uint8 device
    tensor) with the internal-key comparator and, with bits_per_key, the
    InternalFilterPolicy bloom; smallest / largest are the first and the last
    internal key as bytes (FileMetaData), as the table writer's TablesResult
    has them.  Without an entry no table is written: image, data_handles,
    index_handle, smallest and largest are None."""
    from . import sstable
    from .block import INTERNAL_KEY
    e = entries(image, records, paranoid)
    n = e.key_offsets.numel() - 1
    if n == 0:
        return FlushResult(None, None, None, None, None, e.max_sequence, e.status)
    values = e.values.reshape(-1).contiguous()
    res = sstable.write_tables(e.keys, e.key_offsets, values, image, [0, n], INTERNAL_KEY, block_size,
                               restart_interval, bits_per_key, compression)
    return FlushResult(res.table(0), res.table_data_handles(0), res.index_handle(0), res.smallest[0], res.largest[0],
                       e.max_sequence, e.status)


def _max_sequences(image, records, mem_of, n_mems):
    """Per memtable what decode's max_sequence holds for its records alone: the
    largest Sequence + Count - 1 (unsigned; Count an int) over the records of
    at least 12 bytes that lie inside the image; 0 without one.  int64[n_mems]
    holding the 64 bits."""
    torch = _torch()
    rec = records.view(-1, 2)
    off, ln = rec[:, 0], rec[:, 1]
    size = image.numel()
    ok = (off >= 0) & (ln >= 12) & (ln <= 0xffffffff) & (off <= size) & (ln <= size - off)
    at = torch.where(ok, off, torch.zeros_like(off))[:, None] + torch.arange(12, device=image.device)
    b = image[torch.where(ok[:, None], at, torch.zeros_like(at))].to(torch.int64) if size else \
        torch.zeros_like(at)
    seq = torch.zeros_like(off)
    for i in range(8):
        seq = seq | (b[:, i] << (8 * i))
    count = b[:, 8] | (b[:, 9] << 8) | (b[:, 10] << 16) | (b[:, 11] << 24)
    count = torch.where(count >= 1 << 31, count - (1 << 32), count)
    flip = -(1 << 63)  # unsigned order as signed order
    last = torch.where(ok, (seq + count - 1) ^ flip, torch.full_like(seq, flip))
    best = torch.full((max(n_mems, 1),), flip, dtype=torch.int64, device=image.device)[:n_mems]
    if last.numel():
        best = best.scatter_reduce(0, mem_of, last, "amax", include_self=True)
    return best ^ flip


@on_stream
def flush_many(image, records, mem_first, compression=kNoCompression, block_size=4096, restart_interval=16,
               bits_per_key=None, paranoid=False, stream=None):
    """flush for the memtables of one cut list in one chain: memtable m is
    records [mem_first[m], mem_first[m + 1]) (mem_first a list that tiles the
    records).  One scan and one decode of all records, sort_segments, one
    gather, sstable.write_tables.  Returns one FlushResult per memtable that has
    at least one entry, each field what flush gives for that memtable's records
    (the images are views of the chain's one arena, so holding one keeps the
    whole arena alive); memtables without an entry are dropped before the table
    writer runs."""
    torch = _torch()
    from . import merge, sstable
    from .block import INTERNAL_KEY
    mem_first = [int(x) for x in mem_first]
    n, n_mems = _n_records(records), len(mem_first) - 1
    if n_mems < 0 or mem_first[0] != 0 or mem_first[-1] != n or any(a > b for a, b in zip(mem_first, mem_first[1:])):
        raise ValueError("mem_first must tile the records")
    if n_mems == 0:
        return []
    dev = image.device
    counts, _ = scan(image, records)
    entry_base, key_base = bases(counts)
    d = decode(image, records, entry_base, key_base)
    d_mem_first = torch.tensor(mem_first, dtype=torch.int64, device=dev)
    seg_first = entry_base[d_mem_first].contiguous()
    p = sort_segments(d.keys, d.key_offsets, seg_first)
    g = merge.gather(d.keys, d.key_offsets, d.values.reshape(-1), p)
    mem_of = torch.searchsorted(d_mem_first[1:].contiguous(), torch.arange(n, device=dev), right=True)
    mem_of = torch.clamp(mem_of, max=n_mems - 1)
    max_seq = _max_sequences(image, records, mem_of, n_mems)
    # the one read after the chain: how many records are in error, sort's and gather's status, where the
    # memtables' entries lie and their largest sequence numbers
    host = torch.cat([torch.stack([(d.status != WB_OK).sum().to(torch.int64), p.run_status[0].to(torch.int64),
                                   g.status[0].to(torch.int64)]), seg_first, max_seq]).cpu().tolist()
    n_bad, sort_st, gather_st = host[:3]
    seg_host, seq_host = host[3:4 + n_mems], host[4 + n_mems:]
    if n_bad:  # (only then the statuses themselves)
        status = d.status.cpu().tolist()
        for r, st in enumerate(status):
            if st in (WB_BAD_INPUT, WB_NO_ROOM) or (paranoid and st != WB_OK):
                m = max(i for i in range(n_mems) if mem_first[i] <= r)
                raise ValueError(f"record {r - mem_first[m]}: {STATUS_MESSAGE.get(st, st)}")
    if sort_st != MERGE_OK or gather_st != MERGE_OK:
        raise ValueError(f"internal error: sort status {sort_st}, gather status {gather_st}")
    live = [m for m in range(n_mems) if seg_host[m + 1] > seg_host[m]]
    if not live:
        return []
    # (the entries of the memtables without one are none: the live ones tile them)
    table_first = [seg_host[m] for m in live] + [seg_host[-1]]
    res = sstable.write_tables(g.keys, g.key_offsets, g.values.reshape(-1).contiguous(), image, table_first,
                               INTERNAL_KEY, block_size, restart_interval, bits_per_key, compression)
    return [FlushResult(res.table(t), res.table_data_handles(t), res.index_handle(t), res.smallest[t],
                        res.largest[t], seq_host[m] & ((1 << 64) - 1), d.status[mem_first[m]:mem_first[m + 1]])
            for t, m in enumerate(live)]


def _framing(buf):
    """The physical records of a cleanly framed log image: [(header offset,
    payload length, type)].  Anything log::Reader would report raises."""
    def fault(what, at):
        raise ValueError(f"{what} at offset {at}: not a cleanly framed log; lsbm::log::BatchReader "
                         "(include/lsbm/log_checksum.h) reads such a log with the reference's reporter semantics")
    out, pos, n = [], 0, len(buf)
    while pos < n:
        left = kBlockSize - pos % kBlockSize
        if left < kHeaderSize:  # the block's trailer
            pos += left
            continue
        if n - pos < kHeaderSize:
            fault("truncated record header", pos)
        length, t = int(buf[pos + 4]) | int(buf[pos + 5]) << 8, int(buf[pos + 6])
        if kHeaderSize + length > left or pos + kHeaderSize + length > n:
            fault("bad record length", pos)
        if t not in (kFullType, kFirstType, kMiddleType, kLastType):
            fault(f"unknown record type {t}", pos)
        out.append((pos, length, t))
        pos += kHeaderSize + length
    return out


@on_stream
def log_records(image_host, device="cuda", stream=None):
    """(image, records): the logical records of a log file (bytes or a uint8
    numpy array) as log::Reader::ReadRecord returns them, for scan / entries /
    flush.  Every physical record's CRC is verified on the device
    (log.verify_records).  An unfragmented record is its payload in place; the
    fragments of a FIRST / MIDDLE / LAST record are put together by
    lsbm_gather_dev in a side image that follows the log's bytes in `image`.
    A framing or CRC fault raises ValueError."""
    torch = _torch()
    from . import log
    buf = np.frombuffer(bytes(image_host), dtype=np.uint8) if isinstance(image_host, (bytes, bytearray)) \
        else np.ascontiguousarray(image_host, dtype=np.uint8)
    physical = _framing(buf)
    # the logical records: (offset, length) in place, or a list of fragments
    records, parts, side = [], None, []
    for pos, length, t in physical:
        if (t in (kFullType, kFirstType)) != (parts is None):
            raise ValueError(f"fragment out of order at offset {pos}: lsbm::log::BatchReader reads such a log")
        if t == kFullType:
            records.append((pos + kHeaderSize, length))
            continue
        if t == kFirstType:
            parts = []
        parts.append((pos + kHeaderSize, length))
        if t == kLastType:
            total = sum(ln for _, ln in parts)
            records.append((len(buf) + sum(ln for _, _, ln in side), total))
            at = records[-1][0]
            for off, ln in parts:
                side.append((off, at, ln))
                at += ln
            parts = None
    if parts is not None:
        raise ValueError("the log ends inside a fragmented record: lsbm::log::BatchReader reads such a log")
    side_bytes = sum(ln for _, _, ln in side)
    image = torch.zeros(max(len(buf) + side_bytes, 1), dtype=torch.uint8, device=device)[:len(buf) + side_bytes]
    if len(buf):
        image[:len(buf)] = torch.from_numpy(buf.copy()).to(device)
    if physical:
        heads = torch.tensor([p for p, _, _ in physical], dtype=torch.int64, device=device)
        _, nbad = log.verify_records(image[:len(buf)], heads)
        if int(nbad.cpu()[0]):
            raise ValueError(f"{int(nbad.cpu()[0])} physical record(s) fail their checksum: lsbm::log::BatchReader "
                             "reads such a log")
    if side:
        seg = torch.tensor(side, dtype=torch.int64, device=device)
        src, dst, ln = (seg[:, i].contiguous() for i in range(3))
        check(lib().lsbm_gather_dev(_ptr(image), _ptr(src), _ptr(ln), len(side), _ptr(image), _ptr(dst),
                                    _stream_ptr(None)), "lsbm_gather_dev")
    rec = torch.tensor(records, dtype=torch.int64, device=device).reshape(-1).contiguous() if records else \
        torch.zeros(0, dtype=torch.int64, device=device)
    return image, rec


@on_stream
def recover_log(image_host, compression=kNoCompression, block_size=4096, restart_interval=16, bits_per_key=None,
                paranoid=False, device="cuda", stream=None):
    """RecoverLogFile for a log that fits one memtable: log_records, then flush."""
    image, records = log_records(image_host, device, stream)
    return flush(image, records, compression, block_size, restart_interval, bits_per_key, paranoid, stream)


@on_stream
def recover(image, paranoid=False, compression=kNoCompression, block_size=4096, restart_interval=16,
            bits_per_key=None, stream=None, log_bytes=None):
    """DBImpl::RecoverLogFile (lsbm/db_impl.cc:398-470) for a log that lies in
    device memory (the first log_bytes bytes of `image`) and fits one memtable:
    log.read_records, then flush.  RecoverResult(flush, events, status): flush
    is the FlushResult of the records inserted, events the reader's
    Reporter::Corruption calls (int64[m, 4], log.REASONS), status None or the
    status RecoverLogFile returns.

    paranoid=False: every report is ignored (the reporter only logs); records
    shorter than 12 bytes are dropped as "log record too small", which is
    flush's WB_TOO_SMALL.  paranoid=True: the first report sets the status and
    ends the loop, which tests it after ReadRecord returns: the records
    returned before the reporting call are inserted, the one that call returned
    is not; a record that WriteBatch::Iterate rejects raises ValueError with the
    reference's message, as flush(paranoid=True) does."""
    from . import log
    r = log.read_records(image, log_bytes)
    records, status = r.records, None
    if paranoid and r.events.shape[0]:
        before, _, reason, arg = r.events[0].cpu().tolist()
        records = records[:before]
        status = "Corruption: " + log.REASONS[reason] + (f" {arg & 0xFFFFFFFF}" if reason == 10 else "")
    f = flush(r.image, records.reshape(-1).contiguous(), compression, block_size, restart_interval, bits_per_key,
              paranoid)
    return RecoverResult(f, r.events, status)


@on_stream
def heights(n, rnd=SKIPLIST_SEED, stream=None, device="cuda"):
    """(heights uint8[n], rnd_out int64[1]): SkipList::RandomHeight of n
    consecutive inserts from generator state rnd (a new memtable's by default),
    and the state after them."""
    torch = _torch()
    out = torch.zeros(max(n, 1), dtype=torch.uint8, device=device)[:n]
    rnd_out = torch.zeros(1, dtype=torch.int64, device=device)
    nbytes = lib().lsbm_skiplist_heights_scratch_bytes(n)
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
    check(lib().lsbm_skiplist_heights_dev(rnd, n, _ptr(out), _ptr(rnd_out), _ptr(scratch), scratch.numel() * 8,
                                          _stream_ptr(stream)), "lsbm_skiplist_heights_dev")
    return out, rnd_out


def clip_write_buffer(write_buffer_size):
    """SanitizeOptions' clip of write_buffer_size to [64 KiB, 1 GiB]."""
    return min(max(int(write_buffer_size), kMinWriteBuffer), kMaxWriteBuffer)


@on_stream
def cut(key_offsets, values, entry_base, mode, write_buffer_size, key_extra=0, types=None, rec_status=None,
        state=None, mem_cap=None, usage=None, mem_first=None, mem_usage=None, counts=None, state_out=None,
        status=None, stream=None):
    """CutResult(usage int64[n_records], mem_first int64[mem_cap + 1], mem_usage
    int64[mem_cap], counts int64[2] = {memtables, the first is the state's},
    state int64[6], status int32[1]) of lsbm_memtable_cut_dev.  key_offsets and
    values are decode's (key_extra 0) or write.sizes' inputs (key_extra 8, with
    `types`); `state` is a prior call's.  write_buffer_size is taken as given
    (clip_write_buffer is SanitizeOptions').  Without mem_cap every record may
    begin a memtable."""
    torch = _torch()
    _require_cuda(key_offsets, values, entry_base, types, rec_status, state, usage, mem_first, mem_usage, counts,
                  state_out, status)
    _check_tensors(dict(key_offsets=key_offsets, values=values, entry_base=entry_base, types=types,
                        rec_status=rec_status, state=state, usage=usage, mem_first=mem_first, mem_usage=mem_usage,
                        counts=counts, state_out=state_out, status=status), u8=("types",),
                   i32=("rec_status", "status"))
    n, nr, dev = key_offsets.numel() - 1, entry_base.numel() - 1, key_offsets.device
    if n < 0 or nr < 0 or values.numel() != 2 * n or (types is not None and types.numel() != n) or \
            (rec_status is not None and rec_status.numel() != nr) or (state is not None and state.numel() != 6):
        raise ValueError("key_offsets[n + 1], values[2n], types[n], entry_base[n_records + 1], rec_status[n_records] "
                         "and state[6] are needed")
    if mem_cap is None:
        mem_cap = nr + 1 if mem_first is None else mem_first.numel() - 1
    if usage is None:
        usage = _buf(nr, torch.int64, dev)
    if mem_first is None:
        mem_first = _buf(mem_cap + 1, torch.int64, dev)
    if mem_usage is None:
        mem_usage = _buf(mem_cap, torch.int64, dev)
    if counts is None:
        counts = _buf(2, torch.int64, dev)
    if state_out is None:
        state_out = _buf(6, torch.int64, dev)
    if status is None:
        status = _buf(1, torch.int32, dev)
    if usage.numel() != nr or mem_first.numel() < mem_cap + 1 or mem_usage.numel() < mem_cap or \
            counts.numel() != 2 or state_out.numel() != 6 or status.numel() != 1:
        raise ValueError("usage[n_records], mem_first[mem_cap + 1], mem_usage[mem_cap], counts[2], state_out[6] and "
                         "status[1] are needed")
    nbytes = lib().lsbm_memtable_cut_scratch_bytes(n, nr)
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().lsbm_memtable_cut_dev(_ptr(key_offsets), n, key_extra, _ptr(values), _ptr(types), _ptr(entry_base), nr,
                                      _ptr(rec_status), mode, write_buffer_size, _ptr(state), _ptr(usage),
                                      _ptr(mem_first), _ptr(mem_usage), mem_cap, _ptr(counts), _ptr(state_out),
                                      _ptr(status), _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_memtable_cut_dev")
    return CutResult(usage, mem_first, mem_usage, counts, state_out, status)


@on_stream
def recover_all(image, write_buffer_size=4 << 20, paranoid=False, compression=kNoCompression, block_size=4096,
                restart_interval=16, bits_per_key=None, stream=None, log_bytes=None):
    """DBImpl::RecoverLogFile (lsbm/db_impl.cc:398-479) for a log of any size in
    device memory: log.read_records, scan, decode, cut in RECOVER mode, then
    flush_many: the tables of all memtables are written in one chain.
    RecoverAllResult(flushes, mem_first, events, status): flushes are the
    FlushResults in file order (a memtable without an entry writes no table and
    has none; the images are views of one arena that holds every table of the
    log, so holding one keeps the whole arena alive), mem_first the first record of every
    memtable closed by the count of the records the loop took (a list), events
    and status as recover gives them.  write_buffer_size is clipped as SanitizeOptions clips it.

    paranoid=True: the loop ends at the reader's first report or at the first
    record WriteBatch::Iterate rejects (status: the reference's message); the
    tables of the memtables that ended before it are written, the memtable in
    progress is not (RecoverLogFile returns before its WriteLevel0Table)."""
    torch = _torch()
    from . import log
    r = log.read_records(image, log_bytes)
    records, status = r.records, None
    if paranoid and r.events.shape[0]:
        before, _, reason, arg = r.events[0].cpu().tolist()
        records = records[:before]
        status = "Corruption: " + log.REASONS[reason] + (f" {arg & 0xFFFFFFFF}" if reason == 10 else "")
    records = records.reshape(-1).contiguous()
    n = _n_records(records)
    counts, scan_status = scan(r.image, records)
    if paranoid and n:
        # the first record WriteBatch::Iterate rejects ends the loop: found on the device, one read; the records
        # from it on are neither decoded nor counted
        bad = scan_status != WB_OK
        first = bad.to(torch.int64).argmax()
        any_bad, first, st = torch.stack([bad.any().to(torch.int64), first,
                                          scan_status[first].to(torch.int64)]).cpu().tolist()
        if any_bad:
            if st in (WB_BAD_INPUT, WB_NO_ROOM):
                raise ValueError(f"record {first}: {STATUS_MESSAGE.get(st, st)}")
            records, counts, n = records[:2 * first].contiguous(), counts[:first], first
            status = "Corruption: " + STATUS_MESSAGE[st]
    entry_base, key_base = bases(counts)
    d = decode(r.image, records, entry_base, key_base)
    c = cut(d.key_offsets, d.values.reshape(-1), entry_base, RECOVER, clip_write_buffer(write_buffer_size),
            rec_status=d.status)
    fatal = (d.status == WB_BAD_INPUT) | (d.status == WB_NO_ROOM)
    n_mem, cut_st, n_fatal, open_last = torch.stack([c.counts[0], c.status[0].to(torch.int64), fatal.sum(),
                                                     c.state[0]]).cpu().tolist()
    if n_fatal:
        i = int(fatal.to(torch.int64).argmax().cpu())
        raise ValueError(f"record {i}: {STATUS_MESSAGE.get(int(d.status[i].cpu()), '')}")
    if cut_st != MERGE_OK:
        raise ValueError(f"internal error: cut status {cut_st}")
    mem_first = c.mem_first[:n_mem + 1].cpu().tolist()
    # (the loop ended early: the memtable in progress is not written)
    n_done = n_mem - 1 if status is not None and n_mem and open_last else n_mem
    # (records before the first memtable, too small to open one, belong to none)
    flushes = flush_many(r.image, records[2 * mem_first[0]:2 * mem_first[n_done]].contiguous(),
                         [m - mem_first[0] for m in mem_first[:n_done + 1]], compression, block_size,
                         restart_interval, bits_per_key, False) if n_done else []
    return RecoverAllResult(flushes, mem_first, r.events, status)
