"""Batched DB::Get (lsbm's DBImpl::Get -> MemTable::Get -> Version::Get) on the
GPU: the value of key k at snapshot s over memtables and a set of tables.

Thin wrappers over include/lsbm_get.h and the chain between them.  Device
tensors in, device tensors out; every call runs on `stream` (default:
torch's current stream; the contract is engine.py's).

    lookup_keys(user_keys, key_offsets, snapshot)   LookupKey: user key ||
                                       fixed64(seq << 8 | kTypeValue)
    memtable_get(mem, user_keys, key_offsets, snapshot)
                                       MemTable::Get over a sorted memtable
    find_file(bounds, ..., keys, key_offsets)
                                       FindFile and the smallest-key test per
                                       (query, run); Level 0's overlap rule
    save_value(state, key_len, found, ...)
                                       SaveValue and the switch after it
    slices_gather(image, slices, where, ...)
                                       the found values, copied out
    Version(files, runs)               table files opened as Table::Open keeps
                                       them: index and filter blocks in a device
                                       meta buffer, the images in one arena
    Version.for_levels(...)            the probe order of Version::Get
    Version.get(user_keys, key_offsets, snapshot, memtables, verify)
                                       the whole chain
    Version.view(snapshot, memtables, runs, verify)
                                       DBImpl::NewIterator: the scan.SnapshotView
                                       over the memtables and the runs' tables
    status_string(code, user_key)      the reference's Status::ToString()

Keys are a uint8 buffer plus int64 offsets (key i = keys[off[i], off[i+1])).
A sorted memtable is a MemTable(keys, key_offsets, values, image): what
memtable.entries returns, and the image its value slices point into.
"""
from collections import namedtuple

import numpy as np

from ._lib import check, lib
from .block import (GET_FILTERED, INTERNAL_KEY, SEEK_BAD_CONTENTS, SEEK_BAD_ENTRY, SEEK_BAD_HANDLE, SEEK_NOT_VALID,
                    SEEK_VALID, STATE_MESSAGE)
from .block_build import FILTER_KEY, kFooterEncodedLength, kTableMagicNumber
from .engine import _buf, _check_tensors, _ptr, _require_cuda, _stream_ptr, _torch, on_stream
from .merge import MERGE_BAD_INPUT, MERGE_OK  # noqa: F401 (the status word of every call here)
from .sstable import GET_BAD_COMPRESSED
from .table import kBlockTrailerSize

# per-query verdict / final status (include/lsbm_get.h)
UNDECIDED = 0   # after every source: NotFound
FOUND = 1
DELETED = 2
CORRUPT = 3
ERROR = 16      # + a table read's state

# run flags
RUN_LEVEL0 = 0x1
RUN_PRECHECKED = 0x2

MemTable = namedtuple("MemTable", "keys key_offsets values image")
TableFile = namedtuple("TableFile", "data number bits_per_key smallest largest", defaults=(None, None, None))
Run = namedtuple("Run", "files flags", defaults=(0,))
DbGetResult = namedtuple("DbGetResult", "status values value_offsets where")


def status_string(code, user_key=b""):
    """Status::ToString() of a final status: "OK", "NotFound: ", "Corruption:
    corrupted key for : <key>", or the block message of a table read."""
    code = int(code)
    if code == FOUND:
        return "OK"
    if code in (UNDECIDED, DELETED):
        return "NotFound: "
    if code == CORRUPT:
        # (Status joins its two messages with ": ")
        return "Corruption: corrupted key for : " + bytes(user_key).decode("latin-1")
    state = code - ERROR
    if state == GET_BAD_COMPRESSED:
        return "Corruption: corrupted compressed block contents"
    if state in STATE_MESSAGE:
        return "Corruption: " + STATE_MESSAGE[state]
    raise ValueError(f"unknown status {code}")


def _check(**ts):
    _check_tensors(ts, u8=("keys", "user_keys", "image", "found", "bounds", "visible", "out"),
                   i32=("state", "verdict", "where", "run_flags"))


def _status_ok(status, what):
    if int(status.cpu()[0]) != MERGE_OK:
        raise ValueError(f"{what}: bad input (offsets that decrease or pass their buffer, or a key that is too short)")


# ---------------------------------------------------------------- the kernels


@on_stream
def lookup_keys(user_keys, key_offsets, snapshot, stream=None):
    """(keys uint8, key_offsets int64[n + 1], status int32[1]): LookupKey of
    every user key at `snapshot` (an int, or an int64 device tensor of one
    sequence number per query).  key_offsets[q] = the user offset + 8q."""
    torch = _torch()
    snaps = snapshot if hasattr(snapshot, "dtype") else None
    _require_cuda(user_keys, key_offsets, snaps)
    _check(user_keys=user_keys, key_offsets=key_offsets, snapshots=snaps)
    n = key_offsets.numel() - 1
    if n < 0:
        raise ValueError("key_offsets needs at least one entry")
    if snaps is not None and snaps.numel() != n:
        raise ValueError("one snapshot per query")
    dev = key_offsets.device
    cap = user_keys.numel() + 8 * n
    keys = _buf(cap, torch.uint8, dev)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().lsbm_lookup_keys_dev(_ptr(user_keys), user_keys.numel(), _ptr(key_offsets), n,
                                     0 if snaps is not None else int(snapshot), _ptr(snaps), _ptr(keys), cap,
                                     _ptr(out_off), _ptr(status), _stream_ptr(stream)), "lsbm_lookup_keys_dev")
    return keys, out_off, status


def new_verdicts(n, dev):
    """(verdict int32[n] = UNDECIDED, value int64[n, 2] = 0, where int32[n] = -1)."""
    torch = _torch()
    return (_buf(n, torch.int32, dev), _buf(2 * n, torch.int64, dev).view(n, 2), _buf(n, torch.int32, dev, -1))


@on_stream
def memtable_probe(mem, keys, key_offsets, source_id, verdict, value, where, stream=None):
    """lsbm_memtable_get_dev: MemTable::Get of every undecided lookup key over
    the sorted memtable `mem`, into verdict / value / where.  Returns status
    int32[1]."""
    torch = _torch()
    _require_cuda(mem.keys, mem.key_offsets, mem.values, keys, key_offsets, verdict, value, where)
    _check(keys=keys, key_offsets=key_offsets, verdict=verdict, value=value, where=where,
           mem_key_offsets=mem.key_offsets, mem_values=mem.values)
    _check(keys=mem.keys)
    n = key_offsets.numel() - 1
    ne = mem.key_offsets.numel() - 1
    if mem.values.numel() != 2 * ne:
        raise ValueError("mem.values must be one {offset, length} pair per entry")
    status = torch.zeros(1, dtype=torch.int32, device=keys.device)
    check(lib().lsbm_memtable_get_dev(_ptr(mem.keys), mem.keys.numel(), _ptr(mem.key_offsets), _ptr(mem.values), ne,
                                      _ptr(keys), keys.numel(), _ptr(key_offsets), n, int(source_id), _ptr(verdict),
                                      _ptr(value), _ptr(where), _ptr(status), _stream_ptr(stream)),
          "lsbm_memtable_get_dev")
    return status


@on_stream
def find_file(bounds, bound_offsets, run_first, run_flags, visible, keys, key_offsets, stream=None):
    """lsbm_find_file_dev: (file int32[n, n_runs], status int32[1]).  File f's
    smallest and largest internal keys are keys 2f and 2f + 1 of bounds /
    bound_offsets; run r holds files [run_first[r], run_first[r + 1])."""
    torch = _torch()
    _require_cuda(bounds, bound_offsets, run_first, run_flags, visible, keys, key_offsets)
    _check(bounds=bounds, bound_offsets=bound_offsets, run_first=run_first, run_flags=run_flags, visible=visible,
           keys=keys, key_offsets=key_offsets)
    n = key_offsets.numel() - 1
    n_runs = run_first.numel() - 1
    n_files = visible.numel()
    if bound_offsets.numel() != 2 * n_files + 1 or run_flags.numel() != n_runs:
        raise ValueError("bound_offsets needs 2 n_files + 1 entries, run_flags one per run")
    dev = keys.device
    file = _buf(n * n_runs, torch.int32, dev, -1).view(n, n_runs)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().lsbm_find_file_dev(_ptr(bounds), bounds.numel(), _ptr(bound_offsets), n_files, _ptr(run_first),
                                   _ptr(run_flags), _ptr(visible), n_runs, _ptr(keys), keys.numel(),
                                   _ptr(key_offsets), n, _ptr(file), _ptr(status), _stream_ptr(stream)),
          "lsbm_find_file_dev")
    return file, status


@on_stream
def save_value(state, key_len, found, found_offsets, value_in, keys, key_offsets, source_id, verdict, value, where,
               stream=None):
    """lsbm_save_value_dev over one round's table reads, into verdict / value /
    where.  Returns status int32[1]."""
    torch = _torch()
    _require_cuda(state, key_len, found, found_offsets, value_in, keys, key_offsets, verdict, value, where)
    _check(state=state, key_len=key_len, found=found, found_offsets=found_offsets, value_in=value_in, keys=keys,
           key_offsets=key_offsets, verdict=verdict, value=value, where=where)
    n = key_offsets.numel() - 1
    if state.numel() != n or key_len.numel() != n or value_in.numel() != 2 * n or found_offsets.numel() != n + 1:
        raise ValueError("state, key_len, value_in and found_offsets need one entry per query")
    status = torch.zeros(1, dtype=torch.int32, device=keys.device)
    check(lib().lsbm_save_value_dev(_ptr(state), _ptr(key_len), _ptr(found), found.numel(), _ptr(found_offsets),
                                    _ptr(value_in), _ptr(keys), keys.numel(), _ptr(key_offsets), n, int(source_id),
                                    _ptr(verdict), _ptr(value), _ptr(where), _ptr(status), _stream_ptr(stream)),
          "lsbm_save_value_dev")
    return status


@on_stream
def slices_gather(image, slices, where, where_lo, where_hi, out, out_offsets, stream=None):
    """lsbm_slices_gather_dev: image[slices[q]] -> out[out_offsets[q]:] for the
    queries with where_lo <= where[q] < where_hi.  Returns status int32[1]."""
    torch = _torch()
    _require_cuda(image, slices, where, out, out_offsets)
    _check(image=image, slices=slices, where=where, out=out, out_offsets=out_offsets)
    n = where.numel()
    if slices.numel() != 2 * n or out_offsets.numel() != n + 1:
        raise ValueError("slices needs one pair per query, out_offsets n + 1 entries")
    status = torch.zeros(1, dtype=torch.int32, device=where.device)
    check(lib().lsbm_slices_gather_dev(_ptr(image), image.numel(), _ptr(slices), _ptr(where), int(where_lo),
                                       int(where_hi), _ptr(out), out.numel(), _ptr(out_offsets), n, _ptr(status),
                                       _stream_ptr(stream)), "lsbm_slices_gather_dev")
    return status


def _collect(verdict, value, where, images):
    """The final DbGetResult: one read of the values' total, one gather per
    contents buffer.  images: [(where_lo, where_hi, image)]."""
    torch = _torch()
    n = verdict.numel()
    dev = verdict.device
    lengths = torch.where(verdict == FOUND, value[:, 1], torch.zeros_like(value[:, 1]))
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(lengths, 0, out=offsets[1:])
    total = int(offsets[-1].cpu())
    out = _buf(total, torch.uint8, dev)
    # (a source that decided without finding a value has the slice {0, 0})
    slices = torch.where((verdict == FOUND)[:, None], value, torch.zeros_like(value)).reshape(-1).contiguous()
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    for lo, hi, image in images:
        bad |= slices_gather(image if image.numel() else _buf(0, torch.uint8, dev), slices, where, lo, hi, out, offsets)
    _status_ok(bad, "slices_gather")
    return DbGetResult(verdict, out, offsets, where)


@on_stream
def memtable_get(mem, user_keys, key_offsets, snapshot, stream=None):
    """MemTable::Get(LookupKey(k, snapshot)) for a batch of user keys over one
    sorted memtable: DbGetResult(status, values, value_offsets, where) with
    status FOUND / DELETED / UNDECIDED (the reference returns false) and where
    0 for the decided queries."""
    keys, offs, st = lookup_keys(user_keys, key_offsets, snapshot)
    verdict, value, where = new_verdicts(offs.numel() - 1, offs.device)
    st2 = memtable_probe(mem, keys, offs, 0, verdict, value, where)
    _status_ok(st | st2, "memtable_get")
    return _collect(verdict, value, where, [(0, 1, mem.image)])


# ---------------------------------------------------------------- a version


def _varint64(buf, p, limit):
    v, shift = 0, 0
    while shift <= 63 and p < limit:
        b = buf[p]
        p += 1
        v |= (b & 127) << shift
        if b < 128:
            return v, p
        shift += 7
    raise ValueError("bad varint")


def _decode_footer(data, what):
    """Footer::DecodeFrom (table/format.cc:43-64): (metaindex handle, index handle)."""
    if len(data) < kFooterEncodedLength:
        raise ValueError(f"{what}: file is too short to be an sstable")
    foot = bytes(data[len(data) - kFooterEncodedLength:])
    if int.from_bytes(foot[40:], "little") != kTableMagicNumber:
        raise ValueError(f"{what}: not an sstable (bad magic number)")
    try:
        a, p = _varint64(foot, 0, 40)
        b, p = _varint64(foot, p, 40)
        c, p = _varint64(foot, p, 40)
        d, p = _varint64(foot, p, 40)
    except ValueError:
        raise ValueError(f"{what}: bad block handle") from None
    return (a, b), (c, d)


def _walk(buf):
    """The entries of a block's contents up to its end or its first bad entry:
    [(key, value)] (Block::Iter's forward walk, on the host: files are opened
    once)."""
    n = len(buf)
    if n < 4:
        return []
    restarts = n - 4 * (1 + int.from_bytes(buf[n - 4:], "little"))
    out, p, key = [], 0, b""
    try:
        while 0 <= p < restarts:
            sh, p = _varint64(buf, p, restarts)
            ns, p = _varint64(buf, p, restarts)
            vl, p = _varint64(buf, p, restarts)
            if sh > len(key) or p + ns + vl > restarts:
                break
            key = key[:sh] + bytes(buf[p:p + ns])
            out.append((key, bytes(buf[p + ns:p + ns + vl])))
            p += ns + vl
    except ValueError:
        pass
    return out


def _handle_of(value):
    a, p = _varint64(value, 0, len(value))
    b, _ = _varint64(value, p, len(value))
    return a, b


class Version:
    """Table files opened for Get, and the order in which Get probes them.

    files: [TableFile(data, number, bits_per_key=None, smallest=None,
    largest=None)] (or plain tuples): the file's bytes; its number;
    bits_per_key of the BloomFilterPolicy under InternalFilterPolicy the
    store runs with, or None for no filter policy (a filter block in the file
    is then not consulted, as in Table::ReadMeta); the FileMetaData's smallest
    and largest internal keys, read from the file's first and last entry when
    not given.
    runs: [Run(files, flags=0)] (or plain tuples), the probe list in order:
    file indices in key order, and RUN_LEVEL0 / RUN_PRECHECKED.

    Construction parses each footer and each metaindex block on the host, puts
    the images side by side in one device arena, and sends every index block
    and filter block through sstable.read_blocks once, into the meta buffer
    (Table::Open keeps the same two).  A file whose footer, metaindex, index or
    filter block does not read raises ValueError (in the reference it is
    FindTable's error on every Get that reaches the file).  `visible[f]` (uint8
    device tensor, all 1) is FileMetaData::visible."""

    def __init__(self, files, runs, device="cuda", verify=True):
        torch = _torch()
        from . import sstable
        self.device = dev = torch.device(device)
        self.files = [f if isinstance(f, TableFile) else TableFile(*f) for f in files]
        self.runs = [r if isinstance(r, Run) else Run(*r) for r in runs]
        nf = len(self.files)
        for r in self.runs:
            if any(not 0 <= f < nf for f in r.files):
                raise ValueError("a run names a file that is not there")
            if r.flags & RUN_LEVEL0 and len(r.files) > 1:
                raise ValueError("a LEVEL0 run holds one file")
        datas = [np.frombuffer(bytes(f.data), dtype=np.uint8) for f in self.files]
        base = np.zeros(nf + 1, dtype=np.int64)
        np.cumsum([len(d) for d in datas], out=base[1:])
        self.arena = _buf(int(base[-1]), torch.uint8, dev)
        if base[-1]:
            self.arena.copy_(torch.from_numpy(np.concatenate(datas).copy()))
        self.file_base = torch.from_numpy(base[:-1].copy()).to(dev) if nf else _buf(0, torch.int64, dev)
        self.file_size = torch.from_numpy(np.diff(base)).to(dev) if nf else _buf(0, torch.int64, dev)

        def read(handles, what):
            """read_blocks of [(file, (offset, size))]: each block's contents as bytes
            on the host plus (contents, out_handles) on the device."""
            for f, (off, size) in handles:
                if off + size + kBlockTrailerSize > len(datas[f]):
                    raise ValueError(f"file {self.files[f].number}: {what}: truncated block read")
            flat = [v for f, (off, size) in handles for v in (int(base[f]) + off, size)]
            h = torch.tensor(flat, dtype=torch.int64, device=dev) if flat else _buf(0, torch.int64, dev)
            contents, oh, st = sstable.read_blocks(self.arena, h, verify)
            for (f, _), s in zip(handles, st.cpu().tolist()):
                if s != sstable.READ_OK:
                    raise ValueError(f"file {self.files[f].number}: {what}: {sstable.READ_MESSAGE[s]}")
            host = contents.cpu().numpy().tobytes()
            pairs = oh.view(-1, 2).cpu().tolist()
            return [host[o:o + s] for o, s in pairs], contents, oh

        footers = [_decode_footer(d, f"file {f.number}") for d, f in zip(datas, self.files)]
        self._index_at = [footers[i][1] for i in range(nf)]  # each index block's handle in its file (view)
        # the metaindex blocks: where the filter block is (Table::ReadMeta)
        metas, _, _ = read([(i, footers[i][0]) for i in range(nf)], "metaindex block")
        filter_handle = [None] * nf
        for i, meta in enumerate(metas):
            if self.files[i].bits_per_key is None:
                continue
            for k, v in _walk(meta):
                if k == FILTER_KEY:
                    try:
                        filter_handle[i] = _handle_of(v)
                    except ValueError:
                        pass  # (ReadMeta ignores a handle that does not decode: no filter)
        # the index blocks and the filter blocks: the meta buffer
        wanted = [(i, footers[i][1]) for i in range(nf)]
        wanted += [(i, h) for i, h in enumerate(filter_handle) if h is not None]
        blocks, self.meta, oh = read(wanted, "index or filter block")
        if self.meta.numel() == 0:
            self.meta = torch.zeros(1, dtype=torch.uint8, device=dev)
        oh = oh.view(-1, 2)
        self.index_handle = oh[:nf].contiguous() if nf else _buf(0, torch.int64, dev).view(0, 2)
        fh = torch.zeros((max(nf, 1), 2), dtype=torch.int64, device=dev)[:nf]
        with_filter = [i for i, h in enumerate(filter_handle) if h is not None]
        if with_filter:
            fh[torch.tensor(with_filter, dtype=torch.int64, device=dev)] = oh[nf:]
        self.filter_handle = fh
        bits = [f.bits_per_key if filter_handle[i] is not None else -1 for i, f in enumerate(self.files)]
        self.file_bits = torch.tensor(bits, dtype=torch.int64, device=dev) if nf else _buf(0, torch.int64, dev)
        self._bits = bits
        # smallest and largest, from the first and the last data block where the caller has none
        need = [i for i, f in enumerate(self.files) if f.smallest is None or f.largest is None]
        ends = {}
        if need:
            asks = []
            for i in need:
                entries = _walk(blocks[i])
                if not entries:
                    raise ValueError(f"file {self.files[i].number}: no smallest / largest key given and the index "
                                     "block has no entry")
                try:
                    asks += [(i, _handle_of(entries[0][1])), (i, _handle_of(entries[-1][1]))]
                except ValueError:
                    raise ValueError(f"file {self.files[i].number}: bad block handle") from None
            got, _, _ = read(asks, "data block")
            for j, i in enumerate(need):
                first, last = _walk(got[2 * j]), _walk(got[2 * j + 1])
                if not first or not last:
                    raise ValueError(f"file {self.files[i].number}: a data block has no entry")
                ends[i] = (first[0][0], last[-1][0])
        bounds = []
        for i, f in enumerate(self.files):
            s = bytes(f.smallest) if f.smallest is not None else ends[i][0]
            g = bytes(f.largest) if f.largest is not None else ends[i][1]
            if len(s) < 8 or len(g) < 8:
                raise ValueError(f"file {f.number}: smallest / largest is no internal key")
            bounds += [s, g]
        self.smallest, self.largest = bounds[0::2], bounds[1::2]
        # the files in run order (a file may sit in more than one run), for lsbm_find_file_dev
        order = [f for r in self.runs for f in r.files]
        self.run_file = torch.tensor(order, dtype=torch.int64, device=dev) if order else _buf(0, torch.int64, dev)
        ordered = [b for f in order for b in (bounds[2 * f], bounds[2 * f + 1])]
        boff = np.zeros(len(ordered) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in ordered], out=boff[1:])
        self.bounds = _buf(int(boff[-1]), torch.uint8, dev)
        if boff[-1]:
            self.bounds.copy_(torch.from_numpy(np.frombuffer(b"".join(ordered), dtype=np.uint8).copy()))
        self.bound_offsets = torch.from_numpy(boff).to(dev)
        first = np.zeros(len(self.runs) + 1, dtype=np.int64)
        np.cumsum([len(r.files) for r in self.runs], out=first[1:])
        self.run_first = torch.from_numpy(first).to(dev)
        self.run_flags = torch.tensor([r.flags for r in self.runs], dtype=torch.int32, device=dev) if self.runs \
            else _buf(0, torch.int32, dev)
        self.visible = _buf(nf, torch.uint8, dev, 1)

    @classmethod
    def for_levels(cls, level0_deletion, level0_insertion, levels, device="cuda", verify=True):
        """The probe order of Version::Get (lsbm/version_set.cc:349-) for a tree
        whose compaction and warm-up buffers are empty
        (compaction_buffer_use_length all 0).  level0_deletion: [TableFile],
        probed newest first (the larger number first), one LEVEL0 run each;
        level0_insertion: [TableFile] in key order, one run; levels: [(deletion
        part, insertion part)] for level 1 and up, each part [TableFile] in key
        order and probed PRECHECKED (ContainKey, then SkipFilterGet)."""
        files, runs = [], []

        def add(part, flags):
            idx = list(range(len(files), len(files) + len(part)))
            files.extend(part)
            return Run(idx, flags)

        norm = [f if isinstance(f, TableFile) else TableFile(*f) for f in level0_deletion]
        for f in sorted(norm, key=lambda f: -f.number):
            runs.append(add([f], RUN_LEVEL0))
        runs.append(add(list(level0_insertion), 0))
        for deletion, insertion in levels:
            runs.append(add(list(deletion), RUN_PRECHECKED))
            runs.append(add(list(insertion), RUN_PRECHECKED))
        return cls(files, runs, device, verify)

    def _visible_in_run_order(self):
        return self.visible[self.run_file].contiguous() if self.run_file.numel() else self.visible[:0]

    @on_stream
    def get(self, user_keys, key_offsets, snapshot, memtables=(), verify=True, stream=None):
        """DB::Get for a batch of user keys at `snapshot` (an int, or an int64
        device tensor, one per query) over `memtables` (MemTable, in the order
        given: mem, then imm) and this version's runs.  Returns
        DbGetResult(status int32[q], values uint8, value_offsets int64[q + 1],
        where int32[q]): status FOUND with the value at values[value_offsets[q]
        : value_offsets[q + 1]], DELETED or UNDECIDED (NotFound), CORRUPT, or
        ERROR + the state of the table read that failed; where is the source
        that decided (memtable i: i; run r: len(memtables) + r; -1: none).
        The host reads one number per run (the found keys longer than their
        lookup key), besides what sstable.read_blocks and torch.unique read."""
        torch = _torch()
        from . import block, bloom, sstable
        dev = self.arena.device
        keys, offs, st = lookup_keys(user_keys, key_offsets, snapshot)
        n = offs.numel() - 1
        verdict, value, where = new_verdicts(n, dev)
        images, bad = [], st.clone()
        if n == 0:
            return _collect(verdict, value, where, images)
        for i, mem in enumerate(memtables):
            bad |= memtable_probe(mem, keys, offs, i, verdict, value, where)
            images.append((i, i + 1, mem.image))
        if not self.runs:
            _status_ok(bad, "Version.get")
            return _collect(verdict, value, where, images)
        file, st = find_file(self.bounds, self.bound_offsets, self.run_first, self.run_flags,
                             self._visible_in_run_order(), keys, offs)
        bad |= st
        _status_ok(bad, "Version.get")  # (the rounds below read through these offsets)
        klen = offs[1:] - offs[:-1]
        zero2 = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        for r, run in enumerate(self.runs):
            if not run.files:
                continue
            source = len(memtables) + r
            slot = file[:, r].to(torch.int64)
            live = (verdict == UNDECIDED) & (slot >= 0)
            f = self.run_file[torch.where(live, slot, torch.zeros_like(slot))]
            # 1. iiter->Seek(k) with BlockHandle::DecodeFrom; a masked query seeks an empty handle
            ih = torch.where(live[:, None], self.index_handle[f], zero2).reshape(-1).contiguous()
            idx = block.seek(self.meta, ih, keys, offs, cmp=INTERNAL_KEY, value_is_handle=True)
            state = torch.where(live, idx.state, torch.full_like(idx.state, SEEK_NOT_VALID))
            if run.flags & RUN_PRECHECKED:  # ContainKey: an index Seek that ends in an error is a miss
                miss = (state == SEEK_BAD_ENTRY) | (state == SEEK_BAD_CONTENTS)
                state = torch.where(miss, torch.full_like(state, SEEK_NOT_VALID), state)
            found = state == SEEK_VALID
            handle = torch.where(found[:, None], idx.handle, zero2)
            # 2. filter->KeyMayMatch(handle.offset(), k), once, PRECHECKED or not
            for bits in sorted({self._bits[i] for i in run.files if self._bits[i] >= 0}):
                probe = found & (self.file_bits[f] == bits)
                fh = torch.where(probe[:, None], self.filter_handle[f], zero2).reshape(-1).contiguous()
                may, _ = bloom.filter_block_may_match(self.meta, fh, handle[:, 0].contiguous(), keys, offs, int(bits),
                                                      strip=8)
                state = torch.where(probe & (may == 0), torch.full_like(state, GET_FILTERED), state)
            live = state == SEEK_VALID
            # 3. the handle inside its file, then moved by the file's place in the arena
            room = self.file_size[f] - kBlockTrailerSize - handle[:, 0]
            inside = (handle[:, 0] >= 0) & (handle[:, 1] >= 0) & (handle[:, 0] <= self.file_size[f]) & \
                (handle[:, 1] <= room)
            state = torch.where(live & ~inside, torch.full_like(state, SEEK_BAD_HANDLE), state)
            live = live & inside
            moved = torch.stack([handle[:, 0] + self.file_base[f], handle[:, 1]], 1)
            # 4. ReadBlock of the distinct data blocks (a query that ended above asks for no block)
            asked = torch.where(live[:, None], moved, torch.full_like(moved, -1))
            blocks, which = torch.unique(asked, dim=0, return_inverse=True)
            contents, out_handles, bstatus = sstable.read_blocks(self.arena, blocks.reshape(-1).contiguous(), verify)
            bstate = sstable._get_state_of(bstatus.to(torch.int64))[which].to(torch.int32)
            state = torch.where(live, bstate, state)
            live = state == SEEK_VALID
            # 5. block_iter->Seek(k), the found key into a window of the lookup key's length
            dh = torch.where(live[:, None], out_handles.view(-1, 2)[which], zero2).reshape(-1).contiguous()
            seek_image = contents if contents.numel() else torch.zeros(1, dtype=torch.uint8, device=dev)
            window = torch.empty(max(keys.numel(), 1), dtype=torch.uint8, device=dev)
            dat = block.seek(seek_image, dh, keys, offs, cmp=INTERNAL_KEY, found=window, found_offsets=offs)
            state = torch.where(live, dat.state, state).contiguous()
            # a found key longer than the lookup key cannot match but can be corrupt, and its tag is
            # past the window: only then the same Seek again, into windows of the true lengths
            longer = (state == SEEK_VALID) & (dat.key_len > klen)
            found_offsets = offs
            if n and int(longer.sum().cpu()):
                sizes = torch.where(longer, dat.key_len, klen)
                found_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                torch.cumsum(sizes, 0, out=found_offsets[1:])
                window = torch.empty(int(found_offsets[-1].cpu()), dtype=torch.uint8, device=dev)
                dat = block.seek(seek_image, dh, keys, offs, cmp=INTERNAL_KEY, found=window,
                                 found_offsets=found_offsets)
            # 6. SaveValue and the switch
            bad |= save_value(state, dat.key_len, window, found_offsets, dat.value.reshape(-1).contiguous(), keys, offs,
                              source, verdict, value, where)
            images.append((source, source + 1, contents))
        _status_ok(bad, "Version.get")
        return _collect(verdict, value, where, images)

    @on_stream
    def view(self, snapshot, memtables=(), runs=None, verify=True, stream=None):
        """DBImpl::NewIterator at `snapshot` (lsbm/db_impl.cc:1290-): the
        scan.SnapshotView over `memtables` (MemTable, in the order given: mem,
        then imm) and the runs `runs` (indices into self.runs; None: all of
        them in order), whose scan() answers range queries.

        NewInternalIterator (:1139-1157) is one MergingIterator over the
        memtables and Version::AddIterators' children; here every data block of
        the chosen runs' files goes through sstable.read_blocks (as
        sstable.compact steps 1-2), a run's files' blocks are concatenated in
        file order into one sorted run (what NewConcatenatingIterator yields),
        the memtables go first as runs of their own, the value images are
        concatenated with the slices rebased, and merge.merge (no drop) is the
        MergingIterator; scan.view then applies DBIter's rule.  A table read
        that fails raises ValueError with the reference's message (iter_->
        status()), as does a run whose files overlap (UNSORTED).

        Version::AddIterators (lsbm/version_set.cc:190-210) adds Level 0's
        deletion part and, for levels 1 and up, both parts -- it leaves out
        Level 0's insertion part, which Version::Get (:349-) probes.  With
        runs=None a Version.for_levels tree therefore scans one run more than
        the reference's iterator sees; for_levels callers who want
        AddIterators' children pass scan_runs()."""
        torch = _torch()
        from . import block, merge, scan, sstable
        dev = self.arena.device
        chosen = list(range(len(self.runs))) if runs is None else [int(r) for r in runs]
        if any(not 0 <= r < len(self.runs) for r in chosen):
            raise ValueError("a run that is not there")
        if len(memtables) + len(chosen) > merge.MAX_RUNS:
            raise ValueError(f"at most {merge.MAX_RUNS} memtables and runs")
        # 1. the data block handles of every chosen run, file after file, moved into the arena
        base = self.file_base.cpu().tolist()
        handles, blocks_before = [], [0]
        for r in chosen:
            for f in self.runs[r].files:
                at = (base[f] + self._index_at[f][0], self._index_at[f][1])
                try:
                    h = sstable.index_data_handles(self.arena, at, verify).reshape(-1, 2).copy()
                except ValueError as e:
                    raise ValueError(f"file {self.files[f].number}: {e}") from None
                h[:, 0] += base[f]
                handles.append(h)
            blocks_before.append(sum(len(h) for h in handles))
        # 2. ReadBlock of every data block; the entries, one run per chosen run
        parts_keys, parts_off, parts_val, images, firsts = [], [], [], [], [0]
        key_base_at, image_base, n_before = 0, 0, 0
        for mem in memtables:
            _require_cuda(mem.keys, mem.key_offsets, mem.values, mem.image)
            vals = mem.values.reshape(-1, 2)
            parts_keys.append(mem.keys.reshape(-1))
            parts_off.append(mem.key_offsets[:-1] + key_base_at)
            parts_val.append(torch.stack([vals[:, 0] + image_base, vals[:, 1]], 1))
            images.append(mem.image.reshape(-1))
            key_base_at += mem.keys.numel()
            image_base += mem.image.numel()
            n_before += mem.key_offsets.numel() - 1
            firsts.append(n_before)
        run_first = torch.tensor(firsts, dtype=torch.int64, device=dev)
        if handles and sum(len(h) for h in handles):
            flat = torch.from_numpy(np.concatenate(handles).reshape(-1)).to(dev)
            contents, out_handles, st = sstable.read_blocks(self.arena, flat, verify)
            bad = [(b, int(s)) for b, s in enumerate(st.cpu().tolist()) if s != sstable.READ_OK]
            if bad:
                raise ValueError(f"data block {bad[0][0]}: {sstable.READ_MESSAGE[bad[0][1]]}")
            counts, st = block.scan(contents, out_handles)
            sstable._raise_on(st, "scan")
            nb = counts.shape[0]
            entry_base = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
            key_base = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts[:, 0], 0, out=entry_base[1:])
            torch.cumsum(counts[:, 1], 0, out=key_base[1:])
            keys, key_offsets, values, _, st = block.decode(contents, out_handles, entry_base, key_base)
            sstable._raise_on(st, "decode")
            values = values.reshape(-1, 2)
            parts_keys.append(keys)
            parts_off.append(key_offsets[:-1] + key_base_at)
            parts_val.append(torch.stack([values[:, 0] + image_base, values[:, 1]], 1))
            images.append(contents)
            key_base_at += keys.numel()
            table_first = entry_base[torch.tensor(blocks_before[1:], dtype=torch.int64, device=dev)] + n_before
            run_first = torch.cat([run_first, table_first])
        else:
            run_first = torch.cat([run_first, torch.full((len(chosen),), n_before, dtype=torch.int64, device=dev)])
        end = torch.tensor([key_base_at], dtype=torch.int64, device=dev)
        all_keys = torch.cat(parts_keys) if parts_keys else _buf(0, torch.uint8, dev)
        all_off = torch.cat(parts_off + [end]).contiguous()
        all_val = torch.cat(parts_val).contiguous() if parts_val else _buf(0, torch.int64, dev).view(0, 2)
        image = torch.cat(images) if images else _buf(0, torch.uint8, dev)
        if all_keys.numel() == 0:
            all_keys = _buf(0, torch.uint8, dev)
        if image.numel() == 0:
            image = _buf(0, torch.uint8, dev)
        # 3. the MergingIterator, then DBIter's rule at the snapshot
        m = merge.merge(all_keys.contiguous(), all_off, all_val, run_first.contiguous(), INTERNAL_KEY)
        bad = [(r, int(s)) for r, s in enumerate(m.run_status.cpu().tolist()) if s != MERGE_OK]
        if bad:
            r, st = bad[0]
            what = f"memtable {r}" if r < len(memtables) else f"run {chosen[r - len(memtables)]}"
            raise ValueError(f"{what}: {merge.STATUS_MESSAGE.get(st, st)}")
        return scan.view(m.keys, m.key_offsets, m.values.reshape(-1).contiguous(), image, snapshot)

    def scan_runs(self):
        """The runs Version::AddIterators walks, for a Version.for_levels tree:
        every run but Level 0's insertion part (the one run without a flag)."""
        return [r for r, run in enumerate(self.runs) if run.flags & (RUN_LEVEL0 | RUN_PRECHECKED)]
