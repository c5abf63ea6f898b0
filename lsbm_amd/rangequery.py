"""LSbM's RangeQuery on the GPU: DBImpl::RangeQuery (lsbm/db_impl.cc:1268-1288)
over the sorted-table lists of a buffered tree -- Version::RangeQuery
(lsbm/version_set.cc:1043-1214) picks the files, TableCache::GetRange /
Table::InternalGetRange (table/table.cc:340-368) counts the entries of each.

    layout_range_slots(tables, use_length, buffered_merge)
                                       the sorted tables Version::RangeQuery can
                                       reach, in the order in which it can reach
                                       them (not Version::Get's: layout_slots)
    range_plan / range_emit            include/lsbm_range.h: the files each query
                                       reads, in the reference's read order
    range_count                        the Seek and the count up to the end key,
                                       one wave per (query, file) pair
    RangeQuery(version)                a BufferedVersion's opened files, the
                                       slots, the range index, and query()

The range index is the internal keys of every entry of every opened file, decoded
once with block.decode into one device arena (keys, 64-bit key_offsets,
file_first_entry, a state per file).  It is built on the first query and kept;
it costs the bytes of the tree's keys plus 8 bytes an entry.

Memtables are not consulted (DBImpl::RangeQuery does not).  Out of scope: a data
block that does not read or decode (ValueError when the index is built; the
reference's TwoLevelIterator skips it), the block cache and fill_cache,
RefineCompactionBuffer.

None of these callables takes a stream: they enqueue on torch's current stream;
select one with torch.cuda.stream(s).
"""
from collections import namedtuple

import numpy as np

from ._lib import check, lib
from .buffered import (COMPACTION_BUFFER, DELETION_PART, INSERTION_PART, WARMINGUP_BUFFER, _lists, kNumLevels)
from .db import lookup_keys
from .engine import _buf, _ptr, _require_cuda, _stream_ptr, _torch
from .table import kBlockTrailerSize

# slot kinds, slot flags and pair flags (include/lsbm_range.h)
RSLOT_ALL, RSLOT_L0INS, RSLOT_WB, RSLOT_DEL, RSLOT_CB, RSLOT_INS = range(6)
RANGE_COVERS, RANGE_SOLE = 1, 2
RANGE_LAST, RANGE_NO_ENTRIES = 1, 2
RANGE_OK, RANGE_NO_ROOM, RANGE_BAD_INPUT = 0, 1, 2
N_CURSORS = kNumLevels + 1  # read_cursor_key_[0..3], then read_upto_key_

# files: the table's entries; refs: per file (type, table, position) in its level's lists
RangeSlot = namedtuple("RangeSlot", "level kind flags files refs")
RangeResult = namedtuple("RangeResult", "found checked total pair_first pair_file pair_count pair_flags status")
RangeIndex = namedtuple("RangeIndex", "keys key_offsets file_first_entry file_state")


def layout_range_slots(tables, use_length=(0, 0, 0, 0), buffered_merge=False):
    """The slots of Version::RangeQuery, as [RangeSlot(level, kind, flags, files,
    refs)].

    Level 0: ALL, the head deletion table in files_ order (:1060-1066: every
    file is tested, no FindFile, no newest-first sort), then L0INS, the head
    insertion table.  Level L = 1..3: WB, the warm-up list from levels_[L][3]
    itself round to its start, at most use_length[L-1] + 1 tables (:1099-1123),
    only with buffered_merge, L > 1 and use_length[L-1] > 0; DEL; CB, from cb =
    levels_[L][2]->next round to cb, at most use_length[L] tables (:1151-1177;
    a walk that skips cb reaches fewer); INS.

    COVERS marks the table whose ->next is the walk head's ->prev (:1110,
    :1167), by its place in the whole circular list, whatever the use lengths
    cut; SOLE a compaction-buffer table that is its list's only one (cb->next
    is cb: the walk that skips the head starts at it again)."""
    use = [int(u) for u in use_length]
    if len(use) != kNumLevels:
        raise ValueError(f"use_length needs {kNumLevels} entries")
    slots = []

    def table(level, slot_kind, flags, kind, t, lists):
        slots.append(RangeSlot(level, slot_kind, flags, lists[t], [(kind, t, i) for i in range(len(lists[t]))]))

    table(0, RSLOT_ALL, 0, DELETION_PART, 0, _lists(tables, 0, DELETION_PART))
    table(0, RSLOT_L0INS, 0, INSERTION_PART, 0, _lists(tables, 0, INSERTION_PART))
    for level in range(1, kNumLevels):
        cbl, wbl = _lists(tables, level, COMPACTION_BUFFER), _lists(tables, level, WARMINGUP_BUFFER)
        if buffered_merge and level > 1 and use[level - 1] > 0:
            for j in range(min(len(wbl), use[level - 1] + 1)):
                table(level, RSLOT_WB, RANGE_COVERS if j == (0 - 2) % len(wbl) else 0, WARMINGUP_BUFFER, j, wbl)
        table(level, RSLOT_DEL, 0, DELETION_PART, 0, _lists(tables, level, DELETION_PART))
        cb = 1 % len(cbl)
        for j in range(min(len(cbl), use[level])):
            t = (cb + j) % len(cbl)
            flags = (RANGE_COVERS if t == (cb - 2) % len(cbl) else 0) | (RANGE_SOLE if len(cbl) == 1 else 0)
            table(level, RSLOT_CB, flags, COMPACTION_BUFFER, t, cbl)
        table(level, RSLOT_INS, 0, INSERTION_PART, 0, _lists(tables, level, INSERTION_PART))
    return slots


# ---------------------------------------------------------------- the three calls


def _need(t, dtype, what, n=None):
    if t.dtype != dtype or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f"{what} must be a contiguous {dtype} tensor" + (f" of {n}" if n is not None else ""))


def _key_args(start_keys, start_offsets, end_keys, end_offsets):
    torch = _torch()
    _require_cuda(start_keys, start_offsets, end_keys, end_offsets)
    _need(start_keys, torch.uint8, "start_keys")
    _need(end_keys, torch.uint8, "end_keys")
    _need(start_offsets, torch.int64, "start_offsets")
    n = start_offsets.numel() - 1
    if n < 0:
        raise ValueError("start_offsets needs at least one entry")
    _need(end_offsets, torch.int64, "end_offsets", n + 1)
    return n, (_ptr(start_keys), start_keys.numel(), _ptr(start_offsets), _ptr(end_keys), end_keys.numel(),
               _ptr(end_offsets), n)


def _plan_inputs(slot_info, run_first, bounds, bound_offsets, use_length, wb_enabled, cursor_keys, cursor_offsets,
                 start_keys, start_offsets, end_keys, end_offsets):
    torch = _torch()
    _require_cuda(slot_info, run_first, bounds, bound_offsets, use_length, wb_enabled, cursor_keys, cursor_offsets)
    n_slots = slot_info.numel()
    _need(slot_info, torch.int32, "slot_info")
    _need(run_first, torch.int64, "run_first", n_slots + 1)
    _need(bounds, torch.uint8, "bounds")
    _need(bound_offsets, torch.int64, "bound_offsets")
    if bound_offsets.numel() % 2 != 1:
        raise ValueError("bound_offsets needs two keys per run entry and one offset more")
    _need(use_length, torch.int32, "use_length", kNumLevels)
    _need(wb_enabled, torch.int32, "wb_enabled", kNumLevels)
    _need(cursor_keys, torch.uint8, "cursor_keys")
    _need(cursor_offsets, torch.int64, "cursor_offsets", N_CURSORS + 1)
    n, key_args = _key_args(start_keys, start_offsets, end_keys, end_offsets)
    return n, (_ptr(slot_info), n_slots, _ptr(run_first), bound_offsets.numel() // 2, _ptr(bounds), bounds.numel(),
               _ptr(bound_offsets), _ptr(use_length), _ptr(wb_enabled), _ptr(cursor_keys), cursor_keys.numel(),
               _ptr(cursor_offsets)) + key_args


def range_plan(slot_info, run_first, bounds, bound_offsets, use_length, wb_enabled, cursor_keys, cursor_offsets,
               start_keys, start_offsets, end_keys, end_offsets, count=None):
    """lsbm_range_plan_dev: (count int32[n], status int32[1]).  slot_info
    int32[n_slots] = kind | level << 8 | flags << 16; slot s holds the run
    entries [run_first[s], run_first[s + 1]); run entry r's smallest and
    largest internal keys are keys 2r and 2r + 1 of bounds / bound_offsets;
    use_length, wb_enabled int32[4]; cursor key i = cursor_keys[cursor_offsets[i]
    : cursor_offsets[i + 1]], i = 4 being read_upto_key; the start and end
    lookup keys."""
    torch = _torch()
    n, inputs = _plan_inputs(slot_info, run_first, bounds, bound_offsets, use_length, wb_enabled, cursor_keys,
                             cursor_offsets, start_keys, start_offsets, end_keys, end_offsets)
    count = _buf(n, torch.int32, start_offsets.device) if count is None else count
    _need(count, torch.int32, "count", n)
    status = torch.zeros(1, dtype=torch.int32, device=start_offsets.device)
    check(lib().lsbm_range_plan_dev(*inputs, _ptr(count), _ptr(status), _stream_ptr(None)), "lsbm_range_plan_dev")
    return count, status


def range_emit(slot_info, run_first, bounds, bound_offsets, use_length, wb_enabled, cursor_keys, cursor_offsets,
               start_keys, start_offsets, end_keys, end_offsets, pair_first, pair_run, pair_flags, checked,
               pair_cap=None):
    """lsbm_range_emit_dev into pair_run, pair_flags int32[>= pair_cap] at
    pair_first int64[n + 1], and checked int32[n].  Returns status int32[1]."""
    torch = _torch()
    n, inputs = _plan_inputs(slot_info, run_first, bounds, bound_offsets, use_length, wb_enabled, cursor_keys,
                             cursor_offsets, start_keys, start_offsets, end_keys, end_offsets)
    _require_cuda(pair_first, pair_run, pair_flags, checked)
    _need(pair_first, torch.int64, "pair_first", n + 1)
    _need(pair_run, torch.int32, "pair_run")
    _need(pair_flags, torch.int32, "pair_flags")
    _need(checked, torch.int32, "checked", n)
    cap = min(pair_run.numel(), pair_flags.numel()) if pair_cap is None else int(pair_cap)
    if cap > pair_run.numel() or cap > pair_flags.numel():
        raise ValueError("pair_cap passes pair_run or pair_flags")
    status = torch.zeros(1, dtype=torch.int32, device=start_offsets.device)
    check(lib().lsbm_range_emit_dev(*inputs, _ptr(pair_first), _ptr(pair_run), _ptr(pair_flags), cap, _ptr(checked),
                                    _ptr(status), _stream_ptr(None)), "lsbm_range_emit_dev")
    return status


def range_count(index, start_keys, start_offsets, end_keys, end_offsets, pair_first, pair_file, pair_flags,
                pair_count=None, pair_error=None, found=None, total=None):
    """lsbm_range_count_dev over a RangeIndex (keys uint8, key_offsets int64[
    entries + 1], file_first_entry int64[files + 1], file_state int32[files]):
    (pair_count int32[pairs], pair_error int32[pairs], found int32[n], total
    int64[n], status int32[1]).  pair_file int32[pairs] names each pair's file
    by its place in the index."""
    torch = _torch()
    n, key_args = _key_args(start_keys, start_offsets, end_keys, end_offsets)
    keys, key_offsets, file_first, file_state = index
    _require_cuda(keys, key_offsets, file_first, file_state, pair_first, pair_file, pair_flags)
    _need(keys, torch.uint8, "index keys")
    _need(key_offsets, torch.int64, "index key_offsets")
    _need(file_first, torch.int64, "file_first_entry")
    if key_offsets.numel() < 1 or file_first.numel() < 1:
        raise ValueError("key_offsets and file_first_entry need at least one entry")
    n_files = file_first.numel() - 1
    _need(file_state, torch.int32, "file_state", n_files)
    _need(pair_first, torch.int64, "pair_first", n + 1)
    _need(pair_file, torch.int32, "pair_file")
    n_pairs = pair_file.numel()
    _need(pair_flags, torch.int32, "pair_flags", n_pairs)
    dev = start_offsets.device
    pair_count = _buf(n_pairs, torch.int32, dev) if pair_count is None else pair_count
    pair_error = _buf(n_pairs, torch.int32, dev) if pair_error is None else pair_error
    found = _buf(n, torch.int32, dev) if found is None else found
    total = _buf(n, torch.int64, dev) if total is None else total
    _need(pair_count, torch.int32, "pair_count", n_pairs)
    _need(pair_error, torch.int32, "pair_error", n_pairs)
    _need(found, torch.int32, "found", n)
    _need(total, torch.int64, "total", n)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().lsbm_range_count_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), key_offsets.numel() - 1,
                                     _ptr(file_first), _ptr(file_state), n_files, *key_args, _ptr(pair_first),
                                     _ptr(pair_file), _ptr(pair_flags), n_pairs, _ptr(pair_count), _ptr(pair_error),
                                     _ptr(found), _ptr(total), _ptr(status), _stream_ptr(None)),
          "lsbm_range_count_dev")
    return pair_count, pair_error, found, total, status


# ---------------------------------------------------------------- a version's range query


def _varint64(buf, p, limit):
    v, shift = 0, 0
    while p < limit and shift <= 63:
        b = buf[p]
        p += 1
        v |= (b & 127) << shift
        if b < 128:
            return v, p
        shift += 7
    raise ValueError("bad block handle")


class RangeQuery:
    """DBImpl::RangeQuery over a BufferedVersion's tree.

    version: the BufferedVersion whose opened files, lists and arena are used.
    read_upto_key: runtime::read_upto_key_, a user key (the default, empty,
    never opens the compaction buffer's gate).  configure() follows the
    version's use lengths, buffered_merge and read cursor keys unless told
    otherwise, and lays the range slots out again.

    `slots` is layout_range_slots' list; `numbers` (int64 device tensor) the
    file number of every opened file, so numbers[pair_file] names a result's
    files; `index` the RangeIndex, built on the first query()."""

    def __init__(self, version, read_upto_key=b"", verify=True):
        self.version = version
        self.device = version.device
        self.verify = verify
        self.read_upto_key = bytes(read_upto_key)
        self._index = None
        torch = _torch()
        numbers = [f.number for f in version.version.files]
        self.numbers = torch.tensor(numbers, dtype=torch.int64, device=self.device) if numbers else \
            _buf(0, torch.int64, self.device)
        self.configure()

    def configure(self, use_length=None, buffered_merge=None, read_cursor_keys=None, read_upto_key=None):
        """Set compaction_buffer_use_length, buffered_merge, the read cursor keys
        (None: the version's) and read_upto_key (None: as it is), and lay out
        the slots again; the opened files and the range index stay."""
        torch = _torch()
        bv, dev = self.version, self.device
        self.use_length = tuple(int(u) for u in (bv.use_length if use_length is None else use_length))
        self.buffered_merge = bool(bv.buffered_merge if buffered_merge is None else buffered_merge)
        self.read_cursor_keys = tuple(bytes(k) for k in (bv.read_cursor_keys if read_cursor_keys is None
                                                         else read_cursor_keys))
        if len(self.read_cursor_keys) != kNumLevels:
            raise ValueError(f"read_cursor_keys needs {kNumLevels} entries")
        if read_upto_key is not None:
            self.read_upto_key = bytes(read_upto_key)
        self.slots = layout_range_slots(bv.tables, self.use_length, self.buffered_merge)
        run_file, bounds, first = [], [], [0]
        for s in self.slots:
            for e in s.files:
                run_file.append(bv._index_of[e[0]])
                bounds += [bytes(e[2]), bytes(e[3])]
            first.append(len(run_file))
        self.run_file = torch.tensor(run_file, dtype=torch.int32, device=dev) if run_file else \
            _buf(0, torch.int32, dev)
        self.run_first = torch.tensor(first, dtype=torch.int64, device=dev)
        self.bounds, self.bound_offsets = _blob(bounds, dev)
        self.slot_info = torch.tensor([s.kind | (s.level << 8) | (s.flags << 16) for s in self.slots],
                                      dtype=torch.int32, device=dev)
        use = self.use_length
        wb = [int(self.buffered_merge and level > 1 and use[level - 1] > 0) for level in range(kNumLevels)]
        self._use = torch.tensor(use, dtype=torch.int32, device=dev)
        self._wb = torch.tensor(wb, dtype=torch.int32, device=dev)
        self._cursor_keys, self._cursor_offsets = _blob(list(self.read_cursor_keys) + [self.read_upto_key], dev)
        return self

    def _plan_args(self):
        return (self.slot_info, self.run_first, self.bounds, self.bound_offsets, self._use, self._wb,
                self._cursor_keys, self._cursor_offsets)

    @property
    def index(self):
        """The RangeIndex of the opened files: every data block decoded once.
        A file whose index block does not parse has no entries and state 1 (its
        pairs count 0 with RANGE_NO_ENTRIES); a data block that does not read
        or decode raises ValueError."""
        if self._index is None:
            self._index = self._build_index()
        return self._index

    def _build_index(self):
        torch = _torch()
        from . import block, sstable
        v, dev = self.version.version, self.device
        nf = len(v.files)
        state = np.zeros(nf, dtype=np.int32)
        first = np.zeros(nf + 1, dtype=np.int64)
        keys, key_offsets = _buf(0, torch.uint8, dev), torch.zeros(1, dtype=torch.int64, device=dev)
        if nf:
            _, st = block.scan(v.meta, v.index_handle.reshape(-1).contiguous())
            state[:] = [int(s != block.BLOCK_OK) for s in st.cpu().tolist()]
        good = [f for f in range(nf) if not state[f]]
        if good:
            at = torch.tensor(good, dtype=torch.int64, device=dev)
            _, _, values, entry_base, _ = block.decode(v.meta, v.index_handle[at].reshape(-1).contiguous())
            meta = v.meta.cpu().numpy().tobytes()
            values, entry_base = values.cpu().tolist(), entry_base.cpu().tolist()
            base, size = v.file_base.cpu().tolist(), v.file_size.cpu().tolist()
            handles, blocks_of = [], []
            for j, f in enumerate(good):
                for off, n in values[entry_base[j]:entry_base[j + 1]]:
                    try:
                        o, p = _varint64(meta, off, off + n)
                        s, _ = _varint64(meta, p, off + n)
                    except ValueError:
                        raise ValueError(f"file {v.files[f].number}: bad block handle") from None
                    if o + s + kBlockTrailerSize > size[f]:
                        raise ValueError(f"file {v.files[f].number}: data block: truncated block read")
                    handles += [base[f] + o, s]
                blocks_of.append(entry_base[j + 1] - entry_base[j])
            if handles:
                h = torch.tensor(handles, dtype=torch.int64, device=dev)
                contents, out_handles, rst = sstable.read_blocks(v.arena, h, self.verify)
                keys, key_offsets, _, block_first, dst = block.decode(contents, out_handles)
                rst, dst = rst.cpu().tolist(), dst.cpu().tolist()
                which = [f for j, f in enumerate(good) for _ in range(blocks_of[j])]
                for b, f in enumerate(which):
                    if rst[b] != sstable.READ_OK:
                        raise ValueError(f"file {v.files[f].number}: data block: {sstable.READ_MESSAGE[rst[b]]}")
                    if dst[b] != block.BLOCK_OK:
                        raise ValueError(f"file {v.files[f].number}: data block: "
                                         f"{block.STATUS_MESSAGE.get(dst[b], dst[b])}")
                block_first = block_first.cpu().tolist()
                entries, b = {}, 0
                for j, f in enumerate(good):
                    entries[f] = block_first[b + blocks_of[j]] - block_first[b]
                    b += blocks_of[j]
                np.cumsum([entries.get(f, 0) for f in range(nf)], out=first[1:])
                # (the good files' blocks were decoded in file order: their entries lie in file order too)
        return RangeIndex(keys.contiguous(), key_offsets.contiguous(), torch.from_numpy(first).to(dev),
                          torch.from_numpy(state).to(dev) if nf else _buf(0, torch.int32, dev))

    def query(self, start_keys, start_offsets, end_keys, end_offsets, snapshot):
        """DBImpl::RangeQuery for a batch: query q is the user keys
        start_keys[start_offsets[q] : start_offsets[q + 1]] and the like of
        end_keys, at `snapshot` (an int, or one int64 per query on the device).
        Returns RangeResult: found int32[n], Version::RangeQuery's return value
        (per level group the count of the last file read); checked int32[n],
        the files read; total int64[n], the sum of all the counts (our own
        figure); pair_first int64[n + 1]; per pair, in the reference's read
        order, pair_file int32 (a place in `numbers`), pair_count int32 and
        pair_flags int32 (RANGE_LAST, RANGE_NO_ENTRIES, the slot's level << 8);
        status int32[1].  Bad input (a start key under 8 bytes, offsets that
        decrease) raises ValueError.  The host reads two small tensors: the
        pairs' total with the first calls' status words, and the last calls'."""
        torch = _torch()
        dev = self.device
        skeys, soff, st_a = lookup_keys(start_keys, start_offsets, snapshot)
        ekeys, eoff, st_b = lookup_keys(end_keys, end_offsets, snapshot)
        n = soff.numel() - 1
        if eoff.numel() - 1 != n:
            raise ValueError("one end key per start key")
        count, st_c = range_plan(*self._plan_args(), skeys, soff, ekeys, eoff)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            torch.cumsum(count, 0, out=first[1:])
        total_pairs, *bad = torch.stack([first[-1], st_a[0].to(torch.int64), st_b[0].to(torch.int64),
                                         st_c[0].to(torch.int64)]).cpu().tolist()
        if any(bad):
            raise ValueError("RangeQuery.query: bad input (offsets that decrease or pass their buffer, or a start "
                             "or end user key under 8 bytes)")
        pair_run = _buf(total_pairs, torch.int32, dev)
        pair_flags = _buf(total_pairs, torch.int32, dev)
        checked = _buf(n, torch.int32, dev)
        st_d = range_emit(*self._plan_args(), skeys, soff, ekeys, eoff, first, pair_run, pair_flags, checked,
                          total_pairs)
        pair_file = self.run_file[pair_run.to(torch.int64)] if total_pairs else _buf(0, torch.int32, dev)
        pair_count, pair_error, found, total, st_e = range_count(self.index, skeys, soff, ekeys, eoff, first,
                                                                 pair_file.contiguous(), pair_flags)
        status = torch.maximum(st_d, st_e)
        if int(status.cpu()[0]) != RANGE_OK:
            raise ValueError(f"RangeQuery.query: status {int(status.cpu()[0])}")
        return RangeResult(found, checked, total, first, pair_file, pair_count,
                           pair_flags | (pair_error * RANGE_NO_ENTRIES), status)


def _blob(keys, dev):
    """(bytes uint8, offsets int64[len + 1]) of a list of byte strings, on the device."""
    torch = _torch()
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    blob = _buf(int(off[-1]), torch.uint8, dev)
    if off[-1]:
        blob.copy_(torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()))
    return blob, torch.from_numpy(off).to(dev)
