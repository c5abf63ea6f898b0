"""Batched DB::Write (DBImpl::Write / BuildBatchGroup, WriteBatch::Put / Delete,
WriteBatchInternal::Append / SetSequence, log::Writer::AddRecord of lsbm:
lsbm/db_impl.cc:1321-1441, common/write_batch.cc, common/log_writer.cc) on the GPU.

Thin wrappers over include/lsbm_write.h.  Device tensors in, device tensors
out; every call runs on `stream` (default: torch's current stream; the contract is engine.py's).

    sizes(types, key_offsets, ...)   every op's encoded size as running sums,
                                     and the running sums of the batches' ByteSize
    group(batch_bytes, sync)         BuildBatchGroup until the queue has drained:
                                     the leaders and their sync flags
    build(types, keys, ...)          the groups' WriteBatch reps back to back,
                                     {offset, length} records, {sequence, count}
    frame_plan(records, ...)         AddRecord's arithmetic: physical records per
                                     record, each record's file offset, the end
    frame(image, records, ...)       the appended log bytes with zero CRC fields,
                                     and the header offsets log.seal_records takes
    write_batches(...)               the chain, sealed: WriteResult
    frame_records(image, records)    frame_plan + frame + seal for any records
                                     (MANIFEST records too)
    write_logs(...)                  write_batches with MakeRoomForWrite's switch:
                                     a new log wherever the memtable is full

A call models `n_writers` writers already queued in `writers_` in the given
order, each with a non-NULL batch: ops are `types` (uint8: 1 Put, 0 Delete),
user keys `keys` + `key_offsets`, values as int64 {offset, length} pairs into
`value_image`, and `batch_first[n_writers + 1]` the op range of each writer's
batch.  `memtable.entries(result.reps, result.records)` reads the reps as they
are.  Every call has one status word (MERGE_OK / MERGE_NO_ROOM / MERGE_BAD_INPUT
of include/lsbm_block_build.h); on an error no other output changes.
write_batches appends every group to one log; write_logs switches logs where
MakeRoomForWrite does (memtable.cut in WRITE mode; imm_, background errors and
the Level-0 stall stay with the caller).  Out of scope: NULL batches,
logfile_->Sync() itself (group_sync says where it falls).
"""
from collections import namedtuple

from ._lib import check, lib
from .engine import _buf, _check_tensors, _ptr, _require_cuda, _stream_ptr, _torch, on_stream
from .log import kBlockSize, kHeaderSize

OK, NO_ROOM, BAD_INPUT = 0, 1, 2  # LSBM_MERGE_OK, _NO_ROOM, _BAD_INPUT
STATUS_MESSAGE = {NO_ROOM: "an output is too small", BAD_INPUT: "bad input"}
kBatchHeader = 12  # common/write_batch.cc: fixed64 sequence, fixed32 count

SizesResult = namedtuple("SizesResult", "op_sum batch_sum status")
GroupResult = namedtuple("GroupResult", "group_first group_sync n_groups status")
BuildResult = namedtuple("BuildResult", "reps records seq_counts last_sequence status")
FramePlan = namedtuple("FramePlan", "frag_first rec_start status")
FrameResult = namedtuple("FrameResult", "out headers status")
WriteResult = namedtuple("WriteResult", "log headers reps records group_first group_sync sequences counts "
                                        "last_sequence end_offset")
FramedRecords = namedtuple("FramedRecords", "log headers end_offset")
LogSegment = namedtuple("LogSegment", "log headers records first_group n_groups end_offset")
WriteLogsResult = namedtuple("WriteLogsResult", "logs first_log_continues reps records group_first group_sync "
                                                "sequences counts mem_first usage mem_state last_sequence")


def _check(**ts):
    _check_tensors(ts, u8=("types", "keys", "value_image", "sync", "group_sync", "reps", "image", "out"),
                   i32=("status",))


def _scratch(n_ops, n_writers, dev):
    torch = _torch()
    nbytes = lib().lsbm_write_scratch_bytes(n_ops, n_writers)
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def _status(dev):
    torch = _torch()
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _raise(code, what):
    if code != OK:
        raise ValueError(f"{what}: {STATUS_MESSAGE.get(code, code)}")


@on_stream
def sizes(types, key_offsets, keys_size, values, value_image_size, batch_first, op_sum=None, batch_sum=None,
          stream=None):
    """SizesResult(op_sum int64[n_ops + 1], batch_sum int64[n_writers + 1],
    status int32[1]).  batch_sum[w + 1] - batch_sum[w] is
    WriteBatchInternal::ByteSize of writer w's batch."""
    torch = _torch()
    _require_cuda(types, key_offsets, values, batch_first, op_sum, batch_sum)
    _check(types=types, key_offsets=key_offsets, values=values, batch_first=batch_first, op_sum=op_sum,
           batch_sum=batch_sum)
    n, nw, dev = key_offsets.numel() - 1, batch_first.numel() - 1, key_offsets.device
    if n < 0 or nw < 0 or types.numel() != n or values.numel() != 2 * n:
        raise ValueError("types[n], key_offsets[n + 1], values[2n] and batch_first[n_writers + 1] are needed")
    if op_sum is None:
        op_sum = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if batch_sum is None:
        batch_sum = torch.zeros(nw + 1, dtype=torch.int64, device=dev)
    if op_sum.numel() != n + 1 or batch_sum.numel() != nw + 1:
        raise ValueError("op_sum needs n + 1 and batch_sum n_writers + 1 entries")
    status, scratch = _status(dev), _scratch(n, nw, dev)
    check(lib().lsbm_write_sizes_dev(_ptr(types), _ptr(key_offsets), keys_size, _ptr(values), value_image_size, n,
                                     _ptr(batch_first), nw, _ptr(op_sum), _ptr(batch_sum), _ptr(status), _ptr(scratch),
                                     scratch.numel() * 8, _stream_ptr(stream)), "lsbm_write_sizes_dev")
    return SizesResult(op_sum, batch_sum, status)


@on_stream
def group(batch_bytes=None, sync=None, batch_sum=None, group_first=None, group_sync=None, stream=None):
    """GroupResult(group_first int64[cap + 1], group_sync uint8[cap], n_groups
    int64[1], status): group g is writers [group_first[g], group_first[g + 1]).
    Give the batches' ByteSize as batch_bytes[n_writers], or its running sums as
    batch_sum[n_writers + 1] (sizes' output).  Without the outputs the cap is
    n_writers, which always fits."""
    torch = _torch()
    _require_cuda(batch_bytes, sync, batch_sum, group_first, group_sync)
    _check(batch_bytes=batch_bytes, sync=sync, batch_sum=batch_sum, group_first=group_first, group_sync=group_sync)
    if (batch_bytes is None) == (batch_sum is None):
        raise ValueError("give batch_bytes or batch_sum")
    if batch_sum is None:
        batch_sum = torch.zeros(batch_bytes.numel() + 1, dtype=torch.int64, device=batch_bytes.device)
        if batch_bytes.numel():
            torch.cumsum(batch_bytes, 0, out=batch_sum[1:])
    nw, dev = batch_sum.numel() - 1, batch_sum.device
    if nw < 0 or (sync is not None and sync.numel() != nw):
        raise ValueError("batch_sum needs n_writers + 1 entries and sync n_writers")
    if group_first is None:
        group_first = torch.zeros(nw + 1, dtype=torch.int64, device=dev)
    if group_sync is None:
        group_sync = _buf(group_first.numel() - 1, torch.uint8, dev)
    cap = min(group_first.numel() - 1, group_sync.numel())
    if cap < 0:
        raise ValueError("group_first needs at least one entry")
    n_groups, status, scratch = torch.zeros(1, dtype=torch.int64, device=dev), _status(dev), _scratch(0, nw, dev)
    check(lib().lsbm_write_group_dev(_ptr(batch_sum), nw, _ptr(sync), _ptr(group_first), _ptr(group_sync), cap,
                                     _ptr(n_groups), _ptr(status), _ptr(scratch), scratch.numel() * 8,
                                     _stream_ptr(stream)), "lsbm_write_group_dev")
    return GroupResult(group_first, group_sync, n_groups, status)


@on_stream
def build(types, keys, key_offsets, value_image, values, batch_first, op_sum, group_first, n_groups, last_sequence=0,
          reps=None, records=None, seq_counts=None, stream=None):
    """BuildResult(reps uint8, records int64[2 n_groups], seq_counts
    int64[n_groups, 2] = {sequence, count}, last_sequence int64[1], status).
    group_first's first n_groups + 1 entries are the cut.  Without `reps` one
    device -> host read of op_sum's total sizes it."""
    torch = _torch()
    _require_cuda(types, keys, key_offsets, value_image, values, batch_first, op_sum, group_first, reps, records,
                  seq_counts)
    _check(types=types, keys=keys, key_offsets=key_offsets, value_image=value_image, values=values,
           batch_first=batch_first, op_sum=op_sum, group_first=group_first, reps=reps, records=records,
           seq_counts=seq_counts)
    n, nw, dev = key_offsets.numel() - 1, batch_first.numel() - 1, key_offsets.device
    if n < 0 or nw < 0 or types.numel() != n or values.numel() != 2 * n or op_sum.numel() != n + 1:
        raise ValueError("types[n], key_offsets[n + 1], values[2n], op_sum[n + 1] and batch_first[n_writers + 1] "
                         "are needed")
    if group_first.numel() < n_groups + 1:
        raise ValueError("group_first needs n_groups + 1 entries")
    if reps is None:
        reps = _buf(kBatchHeader * n_groups + int(op_sum[-1].cpu()), torch.uint8, dev)
    if records is None:
        records = _buf(2 * n_groups, torch.int64, dev)
    if seq_counts is None:
        seq_counts = _buf(2 * n_groups, torch.int64, dev).reshape(n_groups, 2)
    if records.numel() != 2 * n_groups or seq_counts.numel() != 2 * n_groups:
        raise ValueError("records and seq_counts need 2 n_groups entries")
    new_last, status = torch.zeros(1, dtype=torch.int64, device=dev), _status(dev)
    check(lib().lsbm_write_build_dev(_ptr(types), _ptr(keys), keys.numel(), _ptr(key_offsets), _ptr(value_image),
                                     value_image.numel(), _ptr(values), n, _ptr(batch_first), nw, _ptr(op_sum),
                                     _ptr(group_first), n_groups, last_sequence, _ptr(reps), reps.numel(),
                                     _ptr(records), _ptr(seq_counts), _ptr(new_last), _ptr(status),
                                     _stream_ptr(stream)), "lsbm_write_build_dev")
    return BuildResult(reps, records, seq_counts, new_last, status)


@on_stream
def frame_plan(records, image_size, log_offset=0, frag_first=None, rec_start=None, stream=None):
    """FramePlan(frag_first int64[n + 1], rec_start int64[n + 1], status):
    record i is physical records [frag_first[i], frag_first[i + 1]) and its
    first header is at file offset rec_start[i]; rec_start[n] is the log's new
    end."""
    torch = _torch()
    _require_cuda(records, frag_first, rec_start)
    _check(records=records, frag_first=frag_first, rec_start=rec_start)
    if records.numel() % 2:
        raise ValueError("records must be {offset, length} pairs")
    n, dev = records.numel() // 2, records.device
    if frag_first is None:
        frag_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if rec_start is None:
        rec_start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if frag_first.numel() != n + 1 or rec_start.numel() != n + 1:
        raise ValueError("frag_first and rec_start need n + 1 entries")
    status = _status(dev)
    check(lib().lsbm_log_frame_plan_dev(image_size, _ptr(records), n, log_offset, _ptr(frag_first), _ptr(rec_start),
                                        _ptr(status), _stream_ptr(stream)), "lsbm_log_frame_plan_dev")
    return FramePlan(frag_first, rec_start, status)


@on_stream
def frame(image, records, log_offset, frag_first, rec_start, out=None, headers=None, stream=None):
    """FrameResult(out uint8, headers int64, status): the bytes appended at file
    offset log_offset (out[0] is that offset) with zero CRC fields, and every
    physical record's offset in `out`.  Without the outputs one device -> host
    read of the plan's totals sizes them."""
    torch = _torch()
    _require_cuda(image, records, frag_first, rec_start, out, headers)
    _check(image=image, records=records, frag_first=frag_first, rec_start=rec_start, out=out, headers=headers)
    n, dev = records.numel() // 2, records.device
    if records.numel() % 2 or frag_first.numel() != n + 1 or rec_start.numel() != n + 1:
        raise ValueError("records[2n], frag_first[n + 1] and rec_start[n + 1] are needed")
    if out is None or headers is None:
        n_frag, end = torch.stack([frag_first[-1], rec_start[-1]]).cpu().tolist()
        if out is None:
            out = _buf(max(end - log_offset, 0), torch.uint8, dev)
        if headers is None:
            headers = _buf(max(n_frag, 0), torch.int64, dev)
    status = _status(dev)
    check(lib().lsbm_log_frame_dev(_ptr(image), image.numel(), _ptr(records), n, log_offset, _ptr(frag_first),
                                   _ptr(rec_start), _ptr(out), out.numel(), _ptr(headers), headers.numel(),
                                   _ptr(status), _stream_ptr(stream)), "lsbm_log_frame_dev")
    return FrameResult(out, headers, status)


@on_stream
def frame_records(image, records, log_offset=0, seal=True, stream=None):
    """log::Writer::AddRecord of every record image[records[2i], + records[2i+1])
    onto a log of log_offset bytes: FramedRecords(log uint8, headers int64,
    end_offset int).  log[0] is file offset log_offset; with `seal` every
    header's masked CRC is written (log.seal_records).  One host read between
    the plan and the frame (the physical record count, the end offset and the
    status), one after."""
    torch = _torch()
    from . import log as _log
    p = frame_plan(records, image.numel(), log_offset)
    n_frag, end, st = torch.stack([p.frag_first[-1], p.rec_start[-1], p.status[0].to(torch.int64)]).cpu().tolist()
    _raise(st, "frame_plan")
    out = _buf(end - log_offset, torch.uint8, image.device)
    headers = _buf(n_frag, torch.int64, image.device)
    f = frame(image, records, log_offset, p.frag_first, p.rec_start, out, headers)
    if seal and n_frag:
        _log.seal_records(out, headers)
    _raise(int(f.status.cpu()[0]), "frame")
    return FramedRecords(out, headers, end)


@on_stream
def write_batches(types, keys, key_offsets, value_image, values, batch_first, sync=None, last_sequence=0,
                  log_offset=0, stream=None):
    """DBImpl::Write of every queued writer until the queue has drained:
    sizes -> group -> build -> frame_plan -> frame -> log.seal_records.
    WriteResult(log, headers, reps, records, group_first, group_sync,
    sequences, counts, last_sequence, end_offset): `log` is what the reference
    would have appended at file offset log_offset, `headers` its physical
    records, `reps` / `records` the WriteBatch each group's leader passed to
    InsertInto (memtable.entries reads them), group g is writers
    [group_first[g], group_first[g + 1]), and last_sequence / end_offset are
    the next call's.  Host reads between the steps are only the totals that
    size the next output: the group count and the rep bytes after `group`, the
    physical record count and the end offset after `frame_plan`."""
    torch = _torch()
    from . import log as _log
    dev = key_offsets.device
    s = sizes(types, key_offsets, keys.numel(), values, value_image.numel(), batch_first)
    g = group(batch_sum=s.batch_sum, sync=sync)
    st_s, st_g, n_groups, body = torch.stack([s.status[0].to(torch.int64), g.status[0].to(torch.int64), g.n_groups[0],
                                              s.op_sum[-1]]).cpu().tolist()
    _raise(st_s, "sizes")
    _raise(st_g, "group")
    reps = _buf(kBatchHeader * n_groups + body, torch.uint8, dev)
    b = build(types, keys, key_offsets, value_image, values, batch_first, s.op_sum, g.group_first, n_groups,
              last_sequence, reps)
    p = frame_plan(b.records, reps.numel(), log_offset)
    st_b, st_p, n_frag, end = torch.stack([b.status[0].to(torch.int64), p.status[0].to(torch.int64), p.frag_first[-1],
                                           p.rec_start[-1]]).cpu().tolist()
    _raise(st_b, "build")
    _raise(st_p, "frame_plan")
    out = _buf(end - log_offset, torch.uint8, dev)
    headers = _buf(n_frag, torch.int64, dev)
    f = frame(reps, b.records, log_offset, p.frag_first, p.rec_start, out, headers)
    if n_frag:
        _log.seal_records(out, headers)
    _raise(int(f.status.cpu()[0]), "frame")
    return WriteResult(out, headers, reps, b.records, g.group_first[:n_groups + 1], g.group_sync[:n_groups],
                       b.seq_counts[:, 0], b.seq_counts[:, 1], last_sequence + (key_offsets.numel() - 1), end)


@on_stream
def write_logs(types, keys, key_offsets, value_image, values, batch_first, sync=None, last_sequence=0,
               write_buffer_size=4 << 20, mem_state=None, log_offset=0, stream=None):
    """DBImpl::Write of every queued writer with MakeRoomForWrite's switch
    (lsbm/db_impl.cc:1469-1505, with imm_ == NULL, no background error and no
    Level-0 stall): sizes -> group -> memtable.cut(WRITE) over the groups ->
    build -> frame_records per log.  Before a group whose memtable reports more
    than write_buffer_size (clipped as SanitizeOptions clips it) a new log and
    a new memtable begin.  WriteLogsResult(logs, first_log_continues, reps,
    records, group_first, group_sync, sequences, counts, mem_first, usage,
    mem_state, last_sequence): logs are LogSegments in order, each the bytes
    appended to one log file, its physical records, its groups' {offset,
    length} records into `reps`, and its end offset; the first continues the
    current log at log_offset when first_log_continues, every other one is a
    new file from offset 0.  mem_state (int64[6], None for a new memtable) is
    the memtable's accounting; pass the returned one to the next call."""
    torch = _torch()
    from . import memtable as _mt
    dev = key_offsets.device
    s = sizes(types, key_offsets, keys.numel(), values, value_image.numel(), batch_first)
    g = group(batch_sum=s.batch_sum, sync=sync)
    st_s, st_g, n_groups, body = torch.stack([s.status[0].to(torch.int64), g.status[0].to(torch.int64), g.n_groups[0],
                                              s.op_sum[-1]]).cpu().tolist()
    _raise(st_s, "sizes")
    _raise(st_g, "group")
    group_first = g.group_first[:n_groups + 1].contiguous()
    entry_base = batch_first[group_first].contiguous()  # the ops of each group
    c = _mt.cut(key_offsets, values, entry_base, _mt.WRITE, _mt.clip_write_buffer(write_buffer_size), key_extra=8,
                types=types, state=mem_state)
    reps = _buf(kBatchHeader * n_groups + body, torch.uint8, dev)
    b = build(types, keys, key_offsets, value_image, values, batch_first, s.op_sum, g.group_first, n_groups,
              last_sequence, reps)
    had_mem = torch.zeros(1, dtype=torch.int64, device=dev) if mem_state is None else mem_state[:1]
    st_b, st_c, n_mem, continues, had = torch.stack([b.status[0].to(torch.int64), c.status[0].to(torch.int64),
                                                     c.counts[0], c.counts[1], had_mem[0]]).cpu().tolist()
    _raise(st_b, "build")
    _raise(st_c, "cut")
    mem_first = c.mem_first[:n_mem + 1].cpu().tolist()
    first_continues = bool(continues) or not had  # (without a memtable the caller's log is the new, empty one)
    logs = []
    for m in range(n_mem):
        lo, hi = mem_first[m], mem_first[m + 1]
        recs = b.records[2 * lo:2 * hi].contiguous()
        f = frame_records(reps, recs, log_offset if m == 0 and first_continues else 0)
        logs.append(LogSegment(f.log, f.headers, recs, lo, hi - lo, f.end_offset))
    return WriteLogsResult(logs, first_continues, reps, b.records, group_first, g.group_sync[:n_groups],
                           b.seq_counts[:, 0], b.seq_counts[:, 1], mem_first, c.usage, c.state,
                           last_sequence + (key_offsets.numel() - 1))


__all__ = ["sizes", "group", "build", "frame_plan", "frame", "frame_records", "write_batches", "write_logs", "WriteResult",
           "WriteLogsResult", "LogSegment",
           "OK", "NO_ROOM", "BAD_INPUT", "kBlockSize", "kHeaderSize", "kBatchHeader"]
