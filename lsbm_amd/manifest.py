"""MANIFEST snapshots (lsbm/version_edit.cc, lsbm/version_set.cc), batched on the GPU.

The descriptor of a database directory is a log of VersionEdit records; lsbm's
BasicVersionSet::LogAndApply rewrites it as one WriteSnapshot record on every
call, so the work is the encode and the parse of one very long record
(include/lsbm_manifest.h).

  decode_edits   VersionEdit::DecodeFrom of n records at once: a verdict and
                 the fields per record, the new and deleted files flat
  encode_edits   VersionEdit::EncodeTo of n edits at once from the same shapes
  snapshot       one WriteSnapshot record from a device-resident file table;
                 manifest_image frames it, current_file names it
  recover        BasicVersionSet::Recover's loop over a MANIFEST image:
                 log.read_records, decode_edits and a fold in plain torch
"""
from collections import namedtuple

from ._lib import check, lib
from .engine import _buf, _check_tensors, _ptr, _require_cuda, _stream_ptr, _torch, on_stream

OK, NO_ROOM, BAD_INPUT = 0, 1, 2  # LSBM_MERGE_OK, _NO_ROOM, _BAD_INPUT
STATUS_MESSAGE = {NO_ROOM: "an output is too small", BAD_INPUT: "bad input"}
kNumLevels, kNumTypes = 4, 4  # include/leveldb/params.h:55; deleted_files_[4], new_files_[4]
BYTEWISE = b"leveldb.BytewiseComparator"

# the words of an edit's fields (LSBM_EDIT_* of include/lsbm_manifest.h)
HAS, READ_HAS, LOG, PREV_LOG, NEXT_FILE, LAST_SEQ, WRITE_CURSOR, READ = 0, 1, 2, 3, 4, 5, 6, 7
CMP_OFF, CMP_LEN, FIELD_WORDS = 11, 12, 13
HAS_COMPARATOR, HAS_LOG, HAS_PREV_LOG, HAS_NEXT_FILE, HAS_LAST_SEQ, HAS_WRITE_CURSOR = 1, 2, 4, 8, 16, 32
NEW_WORDS, DEL_WORDS = 5, 4  # {record, type, level, number[, file_size]}

# DecodeFrom's messages by verdict (lsbm/version_edit.cc:137-251); 12 and 13 are the library's
MESSAGES = {1: "comparator name", 2: "log number", 3: "previous log number", 4: "next file number",
            5: "last sequence number", 6: "deleted file", 7: "new-file entry", 8: "write cursor", 9: "read cursor",
            10: "unknown tag", 11: "invalid tag", 12: "file type out of range", 13: "read cursor index out of range"}

DecodePlan = namedtuple("DecodePlan", "verdict fields new_first del_first totals status scratch span_cap")
DecodeItems = namedtuple("DecodeItems", "new_items key_offsets keys del_items status")
Edits = namedtuple("Edits", "verdict fields new_first new_items key_offsets keys del_first del_items")
EncodePlan = namedtuple("EncodePlan", "records totals status scratch")
Encoded = namedtuple("Encoded", "image records")
FileTable = namedtuple("FileTable", "numbers sizes levels types keys key_offsets")
Recovered = namedtuple("Recovered", "status ok log_number prev_log_number next_file_number manifest_file_number "
                                    "last_sequence write_cursor read_cursors files edits live",
                       defaults=(None, None))


def edit_status_string(code):
    """Status::ToString() of DecodeFrom's result for a verdict."""
    return "OK" if code == 0 else "Corruption: VersionEdit: " + MESSAGES[int(code)]


def current_file(number):
    """The bytes of CURRENT for descriptor `number` (SetCurrentFile, common/filename.cc)."""
    return b"MANIFEST-%06d\n" % number


def _scratch(nbytes, dev):
    return _torch().empty(max((nbytes + 7) // 8, 1), dtype=_torch().int64, device=dev)


def _raise(code, what):
    if code != OK:
        raise ValueError(f"{what}: {STATUS_MESSAGE.get(code, code)}")


def _check(**ts):
    _check_tensors(ts, u8=("image", "keys", "names", "out"), i32=("status", "verdict"))


# ---------------------------------------------------------------- decode

@on_stream
def decode_plan(image, records, span_cap, longest_cap, stream=None):
    """lsbm_edit_decode_plan_dev: DecodePlan(verdict int32[n], fields int64[n,
    13], new_first int64[n + 1], del_first int64[n + 1], totals int64[3] =
    {n_new, n_deleted, key bytes}, status int32[1], scratch, span_cap).
    span_cap bounds the records' lengths summed, longest_cap the longest."""
    torch = _torch()
    _require_cuda(image, records)
    _check(image=image, records=records)
    if records.numel() % 2:
        raise ValueError("records must be {offset, length} pairs")
    n, dev = records.numel() // 2, image.device
    verdict = _buf(n, torch.int32, dev)
    fields = torch.zeros((max(n, 1), FIELD_WORDS), dtype=torch.int64, device=dev)[:n]
    new_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    del_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    totals = torch.zeros(3, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(lib().lsbm_edit_decode_scratch_bytes(n, span_cap), dev)
    check(lib().lsbm_edit_decode_plan_dev(_ptr(image), image.numel(), _ptr(records), n, span_cap, longest_cap,
                                          _ptr(verdict), _ptr(fields), _ptr(new_first), _ptr(del_first), _ptr(totals),
                                          _ptr(status), _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_edit_decode_plan_dev")
    return DecodePlan(verdict, fields, new_first, del_first, totals, status, scratch, span_cap)


@on_stream
def decode_emit(image, records, plan, new_cap, del_cap, keys_cap, stream=None):
    """lsbm_edit_decode_emit_dev: DecodeItems(new_items int64[new_cap, 5],
    key_offsets int64[2 new_cap + 1], keys uint8[keys_cap], del_items
    int64[del_cap, 4], status int32[1])."""
    torch = _torch()
    _require_cuda(image, records)
    _check(image=image, records=records)
    n, dev = records.numel() // 2, image.device
    new_items = torch.zeros((max(new_cap, 1), NEW_WORDS), dtype=torch.int64, device=dev)[:new_cap]
    del_items = torch.zeros((max(del_cap, 1), DEL_WORDS), dtype=torch.int64, device=dev)[:del_cap]
    key_offsets = torch.zeros(2 * new_cap + 1, dtype=torch.int64, device=dev)
    keys = _buf(keys_cap, torch.uint8, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().lsbm_edit_decode_emit_dev(_ptr(image), image.numel(), _ptr(records), n, plan.span_cap, _ptr(new_items),
                                          new_cap, _ptr(key_offsets), _ptr(keys), keys_cap, _ptr(del_items), del_cap,
                                          _ptr(status), _ptr(plan.scratch), plan.scratch.numel() * 8,
                                          _stream_ptr(stream)), "lsbm_edit_decode_emit_dev")
    return DecodeItems(new_items, key_offsets, keys, del_items, status)


@on_stream
def decode_edits(image, records, stream=None):
    """VersionEdit::DecodeFrom of every record image[records[i, 0], +
    records[i, 1]) -- what log.read_records returns -- at once:
    Edits(verdict int32[n], fields int64[n, 13], new_first int64[n + 1],
    new_items int64[n_new, 5] = {record, type, level, number, file_size},
    key_offsets int64[2 n_new + 1], keys uint8 (key 2j is file j's smallest,
    2j + 1 its largest), del_first int64[n + 1], del_items int64[n_del, 4]).
    A record whose verdict is not 0 (edit_status_string) has no items and no
    fields.  One host read sizes the plan (the lengths' sum and maximum), one
    sizes the items."""
    torch = _torch()
    _require_cuda(image, records)
    records = records.reshape(-1, 2).contiguous()
    n = records.shape[0]
    span, longest = (torch.stack([records[:, 1].sum(), records[:, 1].max()]).cpu().tolist()) if n else (0, 0)
    if span < 0 or longest < 0:
        raise ValueError("negative record length")
    p = decode_plan(image, records, span, longest)
    n_new, n_del, key_bytes, st = torch.cat([p.totals, p.status.to(torch.int64)]).cpu().tolist()
    _raise(st, "decode_plan")
    e = decode_emit(image, records, p, n_new, n_del, key_bytes)
    _raise(int(e.status.cpu()[0]), "decode_emit")
    return Edits(p.verdict, p.fields, p.new_first, e.new_items, e.key_offsets, e.keys, p.del_first, e.del_items)


# ---------------------------------------------------------------- encode

def _encode_args(fields, names, del_first, del_items, new_first, new_items, keys, key_offsets):
    _require_cuda(fields, names, del_first, del_items, new_first, new_items, keys, key_offsets)
    _check(fields=fields, names=names, del_first=del_first, del_items=del_items, new_first=new_first,
           new_items=new_items, keys=keys, key_offsets=key_offsets)
    n = fields.numel() // FIELD_WORDS
    n_del, n_new = del_items.numel() // DEL_WORDS, new_items.numel() // NEW_WORDS
    if fields.numel() % FIELD_WORDS or del_items.numel() % DEL_WORDS or new_items.numel() % NEW_WORDS:
        raise ValueError("fields[n, 13], del_items[n_del, 4] and new_items[n_new, 5] are needed")
    if del_first.numel() != n + 1 or new_first.numel() != n + 1 or key_offsets.numel() != 2 * n_new + 1:
        raise ValueError("del_first[n + 1], new_first[n + 1] and key_offsets[2 n_new + 1] are needed")
    return (_ptr(fields), _ptr(names), names.numel(), n, _ptr(del_first), _ptr(del_items), n_del, _ptr(new_first),
            _ptr(new_items), n_new, _ptr(keys), _ptr(key_offsets), keys.numel()), n, n_del, n_new


@on_stream
def encode_plan(fields, names, del_first, del_items, new_first, new_items, keys, key_offsets, out_at=0, stream=None):
    """lsbm_edit_encode_plan_dev: EncodePlan(records int64[n, 2] = {out_at +
    offset, length}, totals int64[1] = {bytes}, status int32[1], scratch)."""
    torch = _torch()
    args, n, n_del, n_new = _encode_args(fields, names, del_first, del_items, new_first, new_items, keys, key_offsets)
    dev = fields.device
    records = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev)[:n]
    totals = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(lib().lsbm_edit_encode_scratch_bytes(n, n_del, n_new), dev)
    check(lib().lsbm_edit_encode_plan_dev(*args, out_at, _ptr(records), _ptr(totals), _ptr(status), _ptr(scratch),
                                          scratch.numel() * 8, _stream_ptr(stream)), "lsbm_edit_encode_plan_dev")
    return EncodePlan(records, totals, status, scratch)


@on_stream
def encode_emit(fields, names, del_first, del_items, new_first, new_items, keys, key_offsets, plan, out, out_at=0,
                out_cap=None, stream=None):
    """lsbm_edit_encode_emit_dev into out[out_at, out_at + out_cap): status int32[1]."""
    torch = _torch()
    args, _, _, _ = _encode_args(fields, names, del_first, del_items, new_first, new_items, keys, key_offsets)
    _require_cuda(out)
    _check(out=out)
    status = torch.zeros(1, dtype=torch.int32, device=out.device)
    cap = out.numel() - out_at if out_cap is None else out_cap
    check(lib().lsbm_edit_encode_emit_dev(*args, _ptr(out), out.numel(), out_at, cap, _ptr(status), _ptr(plan.scratch),
                                          plan.scratch.numel() * 8, _stream_ptr(stream)), "lsbm_edit_encode_emit_dev")
    return status


def _unsigned_order(x):
    return x ^ (-0x8000000000000000)  # int64 order of the result is uint64 order of x


def sort_deleted(del_items, n):
    """The deleted files as the reference keeps them -- a std::set<pair<level,
    number>> per type and edit: sorted by (record, type, level, number as
    uint64), duplicates dropped.  Returns (del_first int64[n + 1], del_items)."""
    torch = _torch()
    d = del_items.reshape(-1, DEL_WORDS)
    for col, key in ((3, _unsigned_order), (2, None), (1, None), (0, None)):
        k = d[:, col] if key is None else key(d[:, col])
        d = d[torch.sort(k, stable=True).indices]
    if d.shape[0] > 1:
        keep = torch.ones(d.shape[0], dtype=torch.bool, device=d.device)
        keep[1:] = (d[1:] != d[:-1]).any(dim=1)
        d = d[keep]
    first = torch.zeros(n + 1, dtype=torch.int64, device=d.device)
    if d.shape[0]:
        first[1:] = torch.cumsum(torch.bincount(d[:, 0].clamp(0, max(n - 1, 0)), minlength=n)[:n], 0)
    return first, d.contiguous()


@on_stream
def encode_edits(fields, names=None, del_items=None, new_first=None, new_items=None, keys=None, key_offsets=None,
                 stream=None):
    """VersionEdit::EncodeTo of n edits at once: Encoded(image uint8, records
    int64[n, 2]); write.frame_records(image, records) frames them into a
    MANIFEST log.  fields int64[n, 13] as decode_edits gives them, the
    comparator's {offset, length} in `names`; every edit is written with its
    write cursor and four read cursors, as the reference writes them.
    del_items int64[n_del, 4] in any order (sorted and de-duplicated here, as
    the reference's std::set does); new_items int64[n_new, 5] grouped by edit
    (new_first int64[n + 1]) and non-descending in type inside an edit, their
    keys as decode_edits gives them."""
    torch = _torch()
    _require_cuda(fields)
    dev = fields.device
    fields = fields.reshape(-1, FIELD_WORDS).contiguous()
    n = fields.shape[0]
    names = _buf(0, torch.uint8, dev) if names is None else names
    if del_items is None:
        del_items = torch.zeros((1, DEL_WORDS), dtype=torch.int64, device=dev)[:0]
    if new_items is None:
        new_items = torch.zeros((1, NEW_WORDS), dtype=torch.int64, device=dev)[:0]
        new_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        key_offsets = torch.zeros(1, dtype=torch.int64, device=dev)
    keys = _buf(0, torch.uint8, dev) if keys is None else keys
    del_first, del_items = sort_deleted(del_items, n)
    a = (fields, names, del_first, del_items, new_first.contiguous(), new_items.contiguous(), keys, key_offsets)
    p = encode_plan(*a)
    total, st = torch.cat([p.totals, p.status.to(torch.int64)]).cpu().tolist()
    _raise(st, "encode_plan")
    out = _buf(total, torch.uint8, dev)
    _raise(int(encode_emit(*a, p, out).cpu()[0]), "encode_emit")
    return Encoded(out, p.records)


# ---------------------------------------------------------------- snapshot

def _gather_keys(keys, key_offsets, order):
    """Keys 2p, 2p + 1 for p in order, back to back: (keys, key_offsets)."""
    torch = _torch()
    dev = keys.device
    idx = torch.stack([2 * order, 2 * order + 1], dim=1).reshape(-1)
    start, length = key_offsets[:-1][idx], (key_offsets[1:] - key_offsets[:-1])[idx]
    offs = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(length, 0)
    total = int(offs[-1].cpu()) if idx.numel() else 0
    which = torch.repeat_interleave(torch.arange(idx.numel(), device=dev), length)
    src = start[which] + (torch.arange(total, device=dev) - offs[:-1][which])
    out = _buf(total, torch.uint8, dev)
    if total:
        out.copy_(keys[src])
    return out, offs


@on_stream
def snapshot(files, comparator=BYTEWISE, log_number=0, prev_log_number=0, next_file=0, last_sequence=0, write_cursor=0,
             read_cursors=(0, 0, 0, 0), stream=None):
    """VersionSet::WriteSnapshot's record (lsbm/version_set.cc:2217-2246) from a
    device-resident FileTable(numbers, sizes, levels, types int64[n], keys
    uint8, key_offsets int64[2n + 1]): the comparator, the four numbers, every
    file of every (level, type) part in the table's order, the write cursor
    and the four read cursors.  Encoded(image uint8, records int64[1, 2])."""
    torch = _torch()
    _require_cuda(files.numbers)
    dev = files.numbers.device
    n = files.numbers.numel()
    # EncodeTo writes type by type; WriteSnapshot adds level by level: (type, level), then the table's order
    order = torch.sort(files.types * kNumLevels + files.levels, stable=True).indices
    items = torch.stack([torch.zeros(n, dtype=torch.int64, device=dev), files.types[order], files.levels[order],
                         files.numbers[order], files.sizes[order]], dim=1).contiguous()
    keys, offs = _gather_keys(files.keys, files.key_offsets, order)
    u64 = lambda v: v - (1 << 64) if v >= 1 << 63 else v
    f = [0] * FIELD_WORDS
    f[HAS] = HAS_COMPARATOR | HAS_LOG | HAS_PREV_LOG | HAS_NEXT_FILE | HAS_LAST_SEQ | HAS_WRITE_CURSOR
    f[READ_HAS] = 15
    f[LOG], f[PREV_LOG], f[NEXT_FILE], f[LAST_SEQ], f[WRITE_CURSOR] = (u64(v) for v in (
        log_number, prev_log_number, next_file, last_sequence, write_cursor))
    f[READ:READ + 4] = [u64(v) for v in read_cursors]
    f[CMP_LEN] = len(comparator)
    fields = torch.tensor([f], dtype=torch.int64, device=dev)
    names = torch.tensor(list(comparator), dtype=torch.uint8, device=dev) if comparator else None
    new_first = torch.tensor([0, n], dtype=torch.int64, device=dev)
    return encode_edits(fields, names, None, new_first, items, keys, offs)


def manifest_image(files, log_offset=0, **numbers):
    """snapshot(files, **numbers) framed by log::Writer::AddRecord: the bytes
    of a MANIFEST file (write.FramedRecords)."""
    from . import write as _write
    s = snapshot(files, **numbers)
    return _write.frame_records(s.image, s.records, log_offset)


# ---------------------------------------------------------------- recover

def live_files(edits, n_records):
    """Builder::Apply over records [0, n_records) on an empty base, then
    MaybeAddFile's test (lsbm/version_set.cc:1660-1683, :1795): an added entry
    is live iff the last record that adds its (type, level, number) is not
    before the last record that deletes it.  Returns a bool mask over
    edits.new_items (entries of later records are False)."""
    torch = _torch()
    new, dele = edits.new_items, edits.del_items
    new_in = new[:, 0] < n_records
    dele = dele[dele[:, 0] < n_records]
    keys = torch.cat([new[:, 1:4], dele[:, 1:4]])
    if not keys.shape[0]:
        return new_in
    _, inv = torch.unique(keys, dim=0, return_inverse=True)
    n_keys = int(inv.max().cpu()) + 1
    last_add = torch.full((n_keys,), -1, dtype=torch.int64, device=new.device)
    last_del = torch.full((n_keys,), -1, dtype=torch.int64, device=new.device)
    inv_new, inv_del = inv[:new.shape[0]], inv[new.shape[0]:]
    last_add.scatter_reduce_(0, inv_new[new_in], new[:, 0][new_in], reduce="amax")
    last_del.scatter_reduce_(0, inv_del, dele[:, 0], reduce="amax")
    return new_in & (last_add[inv_new] >= last_del[inv_new])


def _failed(status):
    return Recovered(status, False, 0, 0, 0, 0, 0, 0, (0, 0, 0, 0), {})


@on_stream
def recover(image, comparator=BYTEWISE, log_bytes=None, host_files=True, stream=None):
    """The loop of BasicVersionSet::Recover (lsbm/version_set.cc:1987-2116) over
    a MANIFEST image in device memory: Recovered(status -- Status::ToString()
    -- ok, log_number, prev_log_number, next_file_number, manifest_file_number,
    last_sequence, write_cursor, read_cursors, files).  files maps (level,
    type) to the live entries in added order, each (number, file_size,
    smallest, largest); Builder::SaveTo's split into sorted tables is not
    applied.  With host_files=False files is None and the result carries the
    decoded `edits` and the bool mask `live` over edits.new_items on the
    device instead.  Records are processed up to the reader's first
    Reporter::Corruption call, whose status then is the result."""
    torch = _torch()
    from . import log as _log
    _require_cuda(image)
    r = _log.read_records(image, log_bytes)
    events = r.events.cpu().tolist()
    n = r.records.shape[0]
    k = min(n, events[0][0]) if events else n
    e = decode_edits(r.image, r.records)
    verdict = e.verdict[:k].cpu().tolist()
    fields = [[v & 0xFFFFFFFFFFFFFFFF for v in row] for row in e.fields[:k].cpu().tolist()]
    for i in range(k):
        if verdict[i]:
            return _failed(edit_status_string(verdict[i]))
        if fields[i][HAS] & HAS_COMPARATOR:
            off, ln = fields[i][CMP_OFF], fields[i][CMP_LEN]
            name = r.image[off:off + ln].cpu().numpy().tobytes()
            if name != comparator:
                return _failed("Invalid argument: " + name.decode("latin-1") + " does not match existing comparator : "
                               + comparator.decode("latin-1"))
    if events:
        _, _, reason, arg = events[0]
        return _failed("Corruption: " + _log.REASONS[reason] + (f" {arg & 0xFFFFFFFF}" if reason == 10 else ""))

    def last(bit, word, mask=HAS):
        for row in reversed(fields):
            if row[mask] & bit:
                return row[word]
        return None
    log_number, prev, next_file, last_seq = (last(b, w) for b, w in (
        (HAS_LOG, LOG), (HAS_PREV_LOG, PREV_LOG), (HAS_NEXT_FILE, NEXT_FILE), (HAS_LAST_SEQ, LAST_SEQ)))
    for have, what in ((next_file, "no meta-nextfile entry in descriptor"),
                       (log_number, "no meta-lognumber entry in descriptor"),
                       (last_seq, "no last-sequence-number entry in descriptor")):
        if have is None:
            return _failed("Corruption: " + what)
    live = live_files(e, k)
    files = None
    if host_files:
        items = e.new_items[live].cpu().tolist()
        idx = torch.nonzero(live).reshape(-1).cpu().tolist()
        offs, keys = e.key_offsets.cpu().tolist(), e.keys.cpu().numpy().tobytes()
        files = {}
        for j, (_, t, level, number, size) in zip(idx, items):
            files.setdefault((level, t), []).append((number & 0xFFFFFFFFFFFFFFFF, size & 0xFFFFFFFFFFFFFFFF,
                                                     keys[offs[2 * j]:offs[2 * j + 1]],
                                                     keys[offs[2 * j + 1]:offs[2 * j + 2]]))
    return Recovered("OK", True, log_number, prev or 0, (next_file + 1) & 0xFFFFFFFFFFFFFFFF, next_file, last_seq,
                     last(HAS_WRITE_CURSOR, WRITE_CURSOR) or 0,
                     tuple(last(1 << i, READ + i, READ_HAS) or 0 for i in range(4)), files, e, live)
