"""WAL / MANIFEST record CRCs (common/log_*.cc of lsbm), batched on the GPU.

A log image is 32 KiB blocks of physical records, each a 7-byte header
[masked crc LE32][length LE16][type u8] plus `length` payload bytes
(common/log_format.h).  The reference seals one record at a time in
log::Writer::EmitPhysicalRecord (common/log_writer.cc:75-100) and checks one
at a time in log::Reader::ReadPhysicalRecord (common/log_reader.cc:228-242);
here every header of a device-resident image is sealed / verified in one
launch.  The C++ host layer that frames records and replays the reader is
include/lsbm/log_checksum.h.

The reader itself (include/lsbm_log_read.h): walk, plan
and emit are the three steps over a log image in device memory, read_records
chains them with verify_records into log::Reader's loop -- every record, every
LastRecordOffset() and every Reporter::Corruption call in the reference's order
-- and event_text renders the result as the reference's test shim prints it.
"""
from collections import namedtuple

import numpy as np

from ._lib import check, lib
from .engine import _ptr, _require_cuda, _stream_ptr, _torch, on_stream

kBlockSize = 32768  # common/log_format.h:27
kHeaderSize = 7     # common/log_format.h:30
kZeroType, kFullType, kFirstType, kMiddleType, kLastType = range(5)


def layout_records(payloads):
    """Frame records as log::Writer::AddRecord does (common/log_writer.cc:27-73),
    CRC fields left zero.  Returns (image uint8, header offsets int64)."""
    out, heads, bo = bytearray(), [], 0
    for p in payloads:
        p = bytes(p)
        pos, first = 0, True
        while True:
            if kBlockSize - bo < kHeaderSize:
                out += bytes(kBlockSize - bo)
                bo = 0
            frag = min(len(p) - pos, kBlockSize - bo - kHeaderSize)
            last = pos + frag == len(p)
            t = (kFullType if last else kFirstType) if first else (kLastType if last else kMiddleType)
            heads.append(len(out))
            out += bytes(4) + bytes([frag & 0xFF, frag >> 8, t]) + p[pos:pos + frag]
            bo += kHeaderSize + frag
            pos += frag
            first = False
            if pos == len(p):
                break
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), np.array(heads, dtype=np.int64)


@on_stream
def seal_records(image, headers, stream=None):
    """lsbm_log_seal_dev: write every header's masked CRC in place.
    Returns (masked uint32-as-int32[n], nbad int32[1]) device tensors."""
    torch = _torch()
    _require_cuda(image, headers)
    n = headers.numel()
    masked = torch.empty(n, dtype=torch.int32, device=image.device)
    nbad = torch.zeros(1, dtype=torch.int32, device=image.device)
    check(lib().lsbm_log_seal_dev(_ptr(image), image.numel(), _ptr(headers), n, _ptr(masked),
                                  _ptr(nbad), _stream_ptr(stream)), "lsbm_log_seal_dev")
    return masked, nbad


@on_stream
def verify_records(image, headers, stream=None):
    """lsbm_log_verify_dev: returns (ok uint8[n], nbad int32[1]) device tensors."""
    torch = _torch()
    _require_cuda(image, headers)
    n = headers.numel()
    ok = torch.empty(n, dtype=torch.uint8, device=image.device)
    nbad = torch.zeros(1, dtype=torch.int32, device=image.device)
    check(lib().lsbm_log_verify_dev(_ptr(image), image.numel(), _ptr(headers), n, _ptr(ok),
                                    _ptr(nbad), _stream_ptr(stream)), "lsbm_log_verify_dev")
    return ok, nbad


# ---------------------------------------------------------------- log::Reader (include/lsbm_log_read.h)
READ_OK, READ_NO_ROOM, READ_BAD_INPUT = 0, 1, 2
# how a block's walk ended (block_end[:, 0])
END_RAN_OUT, END_TRAILER, END_BAD_LENGTH, END_ZERO_HEADER, END_TRUNCATED = range(5)
# Reporter::Corruption's words for each reason of events[:, 2] (common/log_reader.cc)
REASONS = {1: "bad record length", 2: "checksum mismatch", 3: "truncated record at end of file",
           4: "partial record without end(1)", 5: "partial record without end(2)",
           6: "partial record without end(3)", 7: "missing start of fragmented record(1)",
           8: "missing start of fragmented record(2)", 9: "error in middle of record", 10: "unknown record type"}

WalkResult = namedtuple("WalkResult", "block_first block_end headers n_headers status")
PlanResult = namedtuple("PlanResult", "totals status scratch n_blocks n_headers")
EmitResult = namedtuple("EmitResult", "records last_record_offset events status")
ReadResult = namedtuple("ReadResult", "image records last_record_offset events")


def read_blocks(log_bytes, initial_offset=0):
    """The blocks a read covers: from SkipToInitialBlock's block to the end."""
    return int(lib().lsbm_log_read_blocks(log_bytes, initial_offset))


def _scratch(nbytes, device):
    return _torch().empty(max((nbytes + 7) // 8, 1), dtype=_torch().int64, device=device)


@on_stream
def walk(image, log_at, log_bytes, initial_offset=0, headers_cap=None, stream=None):
    """lsbm_log_read_walk_dev: WalkResult(block_first int64[n_blocks + 1],
    block_end int64[n_blocks, 2], headers int64[headers_cap] or None, n_headers
    int64[1], status int32[1]).  headers_cap=None only counts: n_headers then
    sizes the second call."""
    torch = _torch()
    _require_cuda(image)
    dev = image.device
    nb = read_blocks(log_bytes, initial_offset)
    block_first = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    block_end = torch.zeros((max(nb, 1), 2), dtype=torch.int64, device=dev)[:nb]
    headers = None if headers_cap is None else torch.zeros(max(headers_cap, 1), dtype=torch.int64, device=dev)
    n_headers = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(8 * (3 * nb + 1), dev)
    check(lib().lsbm_log_read_walk_dev(_ptr(image), image.numel(), log_at, log_bytes, initial_offset, _ptr(block_first),
                                       _ptr(block_end), nb, None if headers is None else _ptr(headers),
                                       0 if headers is None else headers_cap, _ptr(n_headers), _ptr(status),
                                       _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_log_read_walk_dev")
    return WalkResult(block_first, block_end, None if headers is None else headers[:headers_cap], n_headers, status)


@on_stream
def plan(image, log_at, log_bytes, initial_offset, block_first, block_end, headers, ok, stream=None):
    """lsbm_log_read_plan_dev: PlanResult(totals int64[4] = {records, events,
    side bytes, stop offset}, status int32[1], scratch, n_blocks, n_headers);
    emit takes the PlanResult."""
    torch = _torch()
    _require_cuda(image, block_first, block_end, headers, ok)
    dev = image.device
    nb, nh = block_first.numel() - 1, headers.numel()
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(lib().lsbm_log_read_plan_scratch_bytes(nh, nb), dev)
    check(lib().lsbm_log_read_plan_dev(_ptr(image), image.numel(), log_at, log_bytes, initial_offset, _ptr(block_first),
                                       _ptr(block_end), nb, _ptr(headers), nh, _ptr(ok), _ptr(totals), _ptr(status),
                                       _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_log_read_plan_dev")
    return PlanResult(totals, status, scratch, nb, nh)


@on_stream
def emit(image, log_at, log_bytes, initial_offset, p, side_at, side_cap, records_cap, events_cap, stream=None):
    """lsbm_log_read_emit_dev: EmitResult(records int64[records_cap, 2],
    last_record_offset int64[records_cap], events int64[events_cap, 4], status
    int32[1]); fragmented records are assembled in image[side_at, side_at +
    side_cap)."""
    torch = _torch()
    _require_cuda(image)
    dev = image.device
    records = torch.zeros((max(records_cap, 1), 2), dtype=torch.int64, device=dev)[:records_cap]
    lro = torch.zeros(max(records_cap, 1), dtype=torch.int64, device=dev)[:records_cap]
    events = torch.zeros((max(events_cap, 1), 4), dtype=torch.int64, device=dev)[:events_cap]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().lsbm_log_read_emit_dev(_ptr(image), image.numel(), log_at, log_bytes, initial_offset, p.n_blocks,
                                       p.n_headers, side_at, side_cap, _ptr(records), records_cap, _ptr(lro),
                                       _ptr(events), events_cap, _ptr(status), _ptr(p.scratch), p.scratch.numel() * 8,
                                       _stream_ptr(stream)), "lsbm_log_read_emit_dev")
    return EmitResult(records, lro, events, status)


@on_stream
def read_records(image, log_bytes=None, initial_offset=0, stream=None):
    """log::Reader(file, reporter, true, initial_offset) over the log in the
    first log_bytes bytes of a uint8 device tensor, until ReadRecord returns
    false: ReadResult(image, records int64[n, 2], last_record_offset int64[n],
    events int64[m, 4]).  records are {offset, length} in the returned image:
    an unfragmented record in place, a fragmented one in the side area that
    follows the log's bytes (the input tensor itself when no record is
    fragmented).  events are Reporter::Corruption's calls: {records returned
    before the call, bytes, reason, arg} (REASONS; event_text renders them).
    Walk, lsbm_log_verify_dev, plan and emit run on one stream; the host reads
    the header count after the counting walk and the four totals after the
    plan."""
    torch = _torch()
    _require_cuda(image)
    n = image.numel() if log_bytes is None else int(log_bytes)
    if n > image.numel():
        raise ValueError("log_bytes reaches past the image")
    dev = image.device
    nh = int(walk(image, 0, n, initial_offset).n_headers.cpu()[0])
    w = walk(image, 0, n, initial_offset, headers_cap=nh)
    if nh:
        ok, _ = verify_records(image[:n], w.headers)
    else:
        ok = torch.zeros(1, dtype=torch.uint8, device=dev)[:0]
    p = plan(image, 0, n, initial_offset, w.block_first, w.block_end, w.headers, ok)
    n_rec, n_ev, side, _, st_w, st_p = torch.cat([p.totals, w.status.to(torch.int64), p.status.to(torch.int64)]).cpu().tolist()
    if st_w != READ_OK or st_p != READ_OK:
        raise ValueError(f"internal error: walk status {st_w}, plan status {st_p}")
    out = image[:n]
    if side:  # the side image follows the log's bytes
        out = torch.empty(n + side, dtype=torch.uint8, device=dev)
        out[:n] = image[:n]
    e = emit(out, 0, n, initial_offset, p, n, side, n_rec, n_ev)
    st_e = int(e.status.cpu()[0])
    if st_e != READ_OK:
        raise ValueError(f"internal error: emit status {st_e}")
    return ReadResult(out, e.records, e.last_record_offset, e.events)


def _host(t):
    return np.asarray(t.cpu() if hasattr(t, "cpu") else t)


def event_text(result, image_host=None, value=None):
    """Reporter::Corruption's calls of a ReadResult as `D <bytes> Corruption:
    <reason>` lines.  With image_host (the result's image on the host) and
    value (a crc32c function), the full text of the reference's reader
    (oracle/ref_log_shim.cc): an `R <length> <crc32c> <LastRecordOffset>` line
    per record, the reports placed between them."""
    records, lro, events = _host(result.records).reshape(-1, 2), _host(result.last_record_offset), \
        _host(result.events).reshape(-1, 4)
    lines, e = [], 0
    for i in range(len(records) + 1):
        while e < len(events) and events[e][0] == i:
            _, nbytes, reason, arg = (int(x) for x in events[e])
            what = REASONS[reason] + (f" {arg & 0xFFFFFFFF}" if reason == 10 else "")
            lines.append(f"D {nbytes} Corruption: {what}")
            e += 1
        if i < len(records) and image_host is not None:
            off, ln = int(records[i][0]), int(records[i][1])
            lines.append(f"R {ln} {value(bytes(image_host[off:off + ln])):08x} {int(lro[i])}")
    return "".join(line + "\n" for line in lines)
