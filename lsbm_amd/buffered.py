"""LSbM's buffered Get on the GPU: Version::Get (lsbm/version_set.cc:349-623)
over the sorted-table lists of the compaction and warm-up buffers.

    sorted_tables(new_items, live, keys, key_offsets, compaction_buffer_length)
                                       Builder::SaveTo on an empty base, as
                                       Recover calls it: the circular lists of
                                       sorted tables per (level, type)
    layout_slots(tables, use_length, buffered_merge)
                                       the sorted tables Version::Get can reach,
                                       in the order in which it can reach them
    probe_plan / probe_emit            include/lsbm_probe.h: which slots each
                                       query reads, by rank
    BufferedVersion(tables, files, ...)
                                       the opened files (a db.Version), the
                                       slots, and get(): memtables, candidates,
                                       the plan, then one table read per rank
    BufferedVersion.from_manifest(image, files, ...)
                                       manifest.recover, sorted_tables, the
                                       constructor

The sorted-table structure is {(level, type): [table, ...]} with types 0 the
deletion part, 1 the insertion part, 2 the compaction buffer and 3 the warm-up
buffer; tables[0] is levels_[level][type] and the others follow in ->next
order; a table is a list of file entries (number, file_size, smallest,
largest), and may be empty.  The lists are small metadata and are built by a
host loop over the added entries.

Out of scope: RefineCompactionBuffer (which sets `visible`; here it is an
input), AddIterators over the buffers, SaveTo on a non-empty base,
LogAndApply, Finalize, PickCompaction, the key and block caches,
runtime::setReadCursor.  Version::RangeQuery is lsbm_amd/rangequery.py.
"""
from collections import namedtuple

import numpy as np

from ._lib import check, lib
from .block import (INTERNAL_KEY, SEEK_BAD_CONTENTS, SEEK_BAD_ENTRY, SEEK_BAD_HANDLE, SEEK_NOT_VALID, SEEK_VALID)
from .db import (RUN_LEVEL0, UNDECIDED, DbGetResult, TableFile, Version, _collect, _status_ok, find_file, lookup_keys,
                 memtable_probe, new_verdicts, save_value)
from .engine import _buf, _ptr, _require_cuda, _stream_ptr, _torch, on_stream
from .manifest import BYTEWISE
from .table import kBlockTrailerSize

kNumLevels = 4
DELETION_PART, INSERTION_PART, COMPACTION_BUFFER, WARMINGUP_BUFFER = 0, 1, 2, 3

# slot kinds and candidate codes (include/lsbm_probe.h)
SLOT_LEVEL0, SLOT_WB, SLOT_DEL, SLOT_HEAD, SLOT_REST, SLOT_INS = range(6)
CAND_NONE, CAND_MISS, CAND_MAY, CAND_ERR = range(4)
PROBE_OK, PROBE_NO_ROOM, PROBE_BAD_INPUT = 0, 1, 2

# files: the table's entries; flags: the run's, for find_file; refs: per file (type, table, position) in its level's lists
Slot = namedtuple("Slot", "level kind files flags refs")


# ---------------------------------------------------------------- the lists


def _icmp(a, b):
    """InternalKeyComparator::Compare over the bytewise user comparator."""
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return -1 if ua < ub else 1
    ta, tb = int.from_bytes(a[-8:], "little"), int.from_bytes(b[-8:], "little")
    return -1 if ta > tb else (1 if ta < tb else 0)


def new_sorted_table(tables, level, kind, compaction_buffer_length):
    """Version::NewSortedTable (:312-346) on one list: a new empty head, and for
    the compaction buffer the eviction, whose do-while keeps length + 1 tables."""
    tables.insert(0, [])
    if kind == COMPACTION_BUFFER:
        listlength, cur = 0, 0
        while True:
            listlength += 1
            cur = (cur + 1) % len(tables)
            if not (cur != 0 and listlength <= compaction_buffer_length[level]):
                break
        if cur != 0:  # detach all after
            del tables[cur:]


def sorted_tables(new_items, live, keys, key_offsets, compaction_buffer_length=(0, 20, 20, 3), comparator=BYTEWISE):
    """Builder::SaveTo (lsbm/version_set.cc:1686-1770) on an empty base, as
    BasicVersionSet::Recover calls it (:2102-2107).  new_items: the added
    entries in added order, rows (record, type, level, number, file_size) as
    manifest.recover(..., host_files=False).edits.new_items holds them; live:
    MaybeAddFile's test per entry; entry i's smallest and largest internal keys
    are keys 2i and 2i + 1 of keys / key_offsets.  Tensors or host sequences.
    The dead entries matter: preLargest (:1747) is set before MaybeAddFile's
    test.  Returns {(level, type): [table, ...]} for every level and type."""
    if bytes(comparator) != BYTEWISE:
        raise ValueError("only the bytewise comparator orders sorted tables")
    host = lambda t: t.cpu().tolist() if hasattr(t, "cpu") else list(t)
    items, alive, offs = host(new_items), host(live), host(key_offsets)
    blob = keys.cpu().numpy().tobytes() if hasattr(keys, "cpu") else bytes(keys)
    if len(alive) != len(items) or len(offs) != 2 * len(items) + 1:
        raise ValueError("one live flag and two keys per added entry")
    added = {}
    for i, (_, kind, level, number, size) in enumerate(items):
        if not (0 <= level < kNumLevels and 0 <= kind < 4):
            raise ValueError("an entry's level or type is out of range")
        entry = (number & 0xFFFFFFFFFFFFFFFF, size & 0xFFFFFFFFFFFFFFFF, blob[offs[2 * i]:offs[2 * i + 1]],
                 blob[offs[2 * i + 1]:offs[2 * i + 2]])
        if len(entry[2]) < 8 or len(entry[3]) < 8:
            raise ValueError("smallest / largest is no internal key")
        added.setdefault((level, kind), []).append((entry, bool(alive[i])))
    out = {}
    for level in range(kNumLevels):
        for kind in range(4):
            tables = [[]]  # Version's constructor: one empty table, the head
            pre_largest = None
            for i, (entry, is_live) in enumerate(added.get((level, kind), [])):
                # :1743 a smallest key below the previous entry's largest opens a new head
                if level > 0 and i > 0 and _icmp(entry[2], pre_largest) < 0:
                    new_sorted_table(tables, level, kind, compaction_buffer_length)
                pre_largest = entry[3]
                if is_live:  # MaybeAddFile
                    tables[0].append(entry)
            # :1765 the head of the compaction buffer always empty
            if kind in (COMPACTION_BUFFER, WARMINGUP_BUFFER) and tables[0]:
                new_sorted_table(tables, level, kind, compaction_buffer_length)
            out[(level, kind)] = tables
    return out


def _lists(tables, level, kind):
    got = tables.get((level, kind))
    return [list(t) for t in got] if got else [[]]


def layout_slots(tables, use_length=(0, 0, 0, 0), buffered_merge=False):
    """The slots: every sorted table Version::Get can reach, in the fixed order
    in which it can reach it, as [Slot(level, kind, files, flags)].

    Level 0: each file of the head deletion table as one LEVEL0 run, the larger
    number first (:364-374), then the head insertion table.  Level L = 1..3:
    WB, the warm-up list from levels_[L][3]->next round to its start, at most
    use_length[L-1] + 1 tables (:443-463), only with buffered_merge, L > 1 and
    use_length[L-1] > 0; DEL, the head deletion table; HEAD, cb =
    levels_[L][2]->next, only with use_length[L] > 0 and files in it (:526);
    REST, from cb->next round to cb with the counter that starts at 2
    (:568-585); INS, the head insertion table."""
    use = [int(u) for u in use_length]
    if len(use) != kNumLevels:
        raise ValueError(f"use_length needs {kNumLevels} entries")
    slots = []

    def table(level, slot_kind, kind, t, lists):
        slots.append(Slot(level, slot_kind, lists[t], 0, [(kind, t, i) for i in range(len(lists[t]))]))

    dele = _lists(tables, 0, DELETION_PART)
    for i, f in sorted(enumerate(dele[0]), key=lambda p: -p[1][0]):
        slots.append(Slot(0, SLOT_LEVEL0, [f], RUN_LEVEL0, [(DELETION_PART, 0, i)]))
    table(0, SLOT_LEVEL0, INSERTION_PART, 0, _lists(tables, 0, INSERTION_PART))
    for level in range(1, kNumLevels):
        cbl, wbl = _lists(tables, level, COMPACTION_BUFFER), _lists(tables, level, WARMINGUP_BUFFER)
        if buffered_merge and level > 1 and use[level - 1] > 0:
            head = cur = 1 % len(wbl)
            checked = 0
            while True:
                if checked > use[level - 1]:
                    break
                checked += 1
                table(level, SLOT_WB, WARMINGUP_BUFFER, cur, wbl)
                cur = (cur + 1) % len(wbl)
                if cur == head:
                    break
        table(level, SLOT_DEL, DELETION_PART, 0, _lists(tables, level, DELETION_PART))
        cb = 1 % len(cbl)
        if use[level] > 0 and cbl[cb]:
            table(level, SLOT_HEAD, COMPACTION_BUFFER, cb, cbl)
        cur = (cb + 1) % len(cbl)
        checked = 2
        while True:
            if checked > use[level]:
                break
            checked += 1
            table(level, SLOT_REST, COMPACTION_BUFFER, cur, cbl)
            cur = (cur + 1) % len(cbl)
            if cur == cb:
                break
        table(level, SLOT_INS, INSERTION_PART, 0, _lists(tables, level, INSERTION_PART))
    return slots


# ---------------------------------------------------------------- the plan


def _probe_inputs(cand, slot_info, use_length, wb_enabled, cursor_keys, cursor_offsets, keys, key_offsets):
    torch = _torch()
    _require_cuda(cand, slot_info, use_length, wb_enabled, cursor_keys, cursor_offsets, keys, key_offsets)
    for t, dt, what in ((cand, torch.uint8, "cand"), (slot_info, torch.int32, "slot_info"),
                        (use_length, torch.int32, "use_length"), (wb_enabled, torch.int32, "wb_enabled"),
                        (cursor_keys, torch.uint8, "cursor_keys"), (cursor_offsets, torch.int64, "cursor_offsets"),
                        (keys, torch.uint8, "keys"), (key_offsets, torch.int64, "key_offsets")):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {dt} tensor")
    n, n_slots = key_offsets.numel() - 1, slot_info.numel()
    if n < 0 or cand.numel() != n * n_slots:
        raise ValueError("cand needs one byte per (slot, query), slot-major")
    if use_length.numel() != kNumLevels or wb_enabled.numel() != kNumLevels or cursor_offsets.numel() != kNumLevels + 1:
        raise ValueError(f"use_length and wb_enabled need {kNumLevels} entries, cursor_offsets one more")
    return n, (_ptr(cand), n_slots, _ptr(slot_info), _ptr(use_length), _ptr(wb_enabled), _ptr(cursor_keys),
               cursor_keys.numel(), _ptr(cursor_offsets), _ptr(keys), keys.numel(), _ptr(key_offsets), n)


@on_stream
def probe_plan(cand, slot_info, use_length, wb_enabled, cursor_keys, cursor_offsets, keys, key_offsets, count=None,
               stream=None):
    """lsbm_probe_plan_dev: (count int32[n], status int32[1]).  cand uint8[n_slots,
    n] (slot-major); slot_info int32[n_slots] = kind | level << 8; use_length,
    wb_enabled int32[4]; cursor key L = cursor_keys[cursor_offsets[L] :
    cursor_offsets[L + 1]]; keys / key_offsets the lookup keys."""
    torch = _torch()
    n, inputs = _probe_inputs(cand, slot_info, use_length, wb_enabled, cursor_keys, cursor_offsets, keys, key_offsets)
    count = _buf(n, torch.int32, keys.device) if count is None else count
    status = torch.zeros(1, dtype=torch.int32, device=keys.device)
    check(lib().lsbm_probe_plan_dev(*inputs, _ptr(count), _ptr(status), _stream_ptr(stream)), "lsbm_probe_plan_dev")
    return count, status


@on_stream
def probe_emit(cand, slot_info, use_length, wb_enabled, cursor_keys, cursor_offsets, keys, key_offsets, probe_first,
               probe_slot, probe_cap=None, stream=None):
    """lsbm_probe_emit_dev into probe_slot int32[>= probe_cap] at probe_first
    int64[n + 1].  Returns status int32[1]."""
    torch = _torch()
    n, inputs = _probe_inputs(cand, slot_info, use_length, wb_enabled, cursor_keys, cursor_offsets, keys, key_offsets)
    _require_cuda(probe_first, probe_slot)
    if probe_first.dtype != torch.int64 or probe_first.numel() != n + 1 or probe_slot.dtype != torch.int32:
        raise ValueError("probe_first is int64[n + 1], probe_slot int32")
    cap = probe_slot.numel() if probe_cap is None else int(probe_cap)
    if cap > probe_slot.numel():
        raise ValueError("probe_cap passes probe_slot")
    status = torch.zeros(1, dtype=torch.int32, device=keys.device)
    check(lib().lsbm_probe_emit_dev(*inputs, _ptr(probe_first), _ptr(probe_slot), cap, _ptr(status),
                                    _stream_ptr(stream)), "lsbm_probe_emit_dev")
    return status


# ---------------------------------------------------------------- a version


def _file_bytes(f):
    if isinstance(f, TableFile):
        return f
    if isinstance(f, tuple):
        return TableFile(*f)
    if hasattr(f, "cpu"):  # a view of an arena (flush_many, write_tables)
        return TableFile(f.cpu().numpy().tobytes(), None)
    return TableFile(bytes(f), None)


class BufferedVersion:
    """A version with compaction and warm-up buffers, opened for Get.

    tables: the sorted-table structure (sorted_tables' result; missing (level,
    type) keys are empty lists).  files: {number: TableFile, bytes or a uint8
    tensor} -- the bytes of every file the structure names; two entries with
    one number are the same file; a number without bytes raises ValueError.
    bits_per_key: the filter policy of files given as plain bytes (a TableFile
    carries its own).

    use_length: runtime::compaction_buffer_use_length[4]; buffered_merge:
    config::buffered_merge; read_cursor_keys: runtime::read_cursor_key_[4], user
    keys; visible: FileMetaData::visible per file entry, in the order of
    `entries` (level, type, table, file), a uint8 sequence or {number: flag},
    default all 1 -- `visible` is the device tensor and may be rewritten in
    place between calls.

    Composes a db.Version for the opened files (`version`: the arena, the meta
    buffer); `slots` is layout_slots' list, slot s being source
    len(memtables) + s of get().  configure() changes the three parameters
    and lays the slots out again without opening the files again."""

    def __init__(self, tables, files, use_length=(0, 0, 0, 0), buffered_merge=False,
                 read_cursor_keys=(b"", b"", b"", b""), visible=None, bits_per_key=None, device="cuda", verify=True):
        torch = _torch()
        self.device = dev = torch.device(device)
        self.tables = {k: [[tuple(e) for e in t] for t in v] for k, v in tables.items()}
        # the file entries, in the structure's order
        self.entries, self._entry_at = [], {}
        for level in range(kNumLevels):
            for kind in range(4):
                for t, table in enumerate(self.tables.get((level, kind), [])):
                    for i, e in enumerate(table):
                        self._entry_at[(level, kind, t, i)] = len(self.entries)
                        self.entries.append(e)
        if isinstance(visible, dict):
            visible = [int(bool(visible.get(e[0], 1))) for e in self.entries]
        vis = np.ones(len(self.entries), dtype=np.uint8) if visible is None else \
            np.asarray(visible.cpu() if hasattr(visible, "cpu") else visible, dtype=np.uint8)
        if vis.shape != (len(self.entries),):
            raise ValueError("visible needs one flag per file entry")
        self.visible = torch.from_numpy(vis.copy()).to(dev) if len(vis) else _buf(0, torch.uint8, dev)
        # the opened files: one per number the structure names
        numbers = []
        for e in self.entries:
            if e[0] not in numbers:
                numbers.append(e[0])
        opened = []
        for number in numbers:
            if number not in files:
                raise ValueError(f"file {number}: no bytes given")
            f = _file_bytes(files[number])
            first = next(e for e in self.entries if e[0] == number)
            opened.append(TableFile(f.data, number, f.bits_per_key if f.bits_per_key is not None else bits_per_key,
                                    first[2], first[3]))
        self.version = Version(opened, [], dev, verify)
        self._index_of = {number: i for i, number in enumerate(numbers)}
        self.configure(use_length, buffered_merge, read_cursor_keys)

    def configure(self, use_length=None, buffered_merge=None, read_cursor_keys=None):
        """Set compaction_buffer_use_length, buffered_merge and the read cursor
        keys (None: as they are) and lay out the slots again; the opened files
        stay."""
        torch = _torch()
        dev = self.device
        if use_length is not None:
            self.use_length = tuple(int(u) for u in use_length)
        if buffered_merge is not None:
            self.buffered_merge = bool(buffered_merge)
        if read_cursor_keys is not None:
            self.read_cursor_keys = tuple(bytes(k) for k in read_cursor_keys)
        if len(self.read_cursor_keys) != kNumLevels:
            raise ValueError(f"read_cursor_keys needs {kNumLevels} entries")
        self.slots = layout_slots(self.tables, self.use_length, self.buffered_merge)
        # the slots as runs of lsbm_find_file_dev: bounds per entry, in slot order
        run_file, run_entry, run_masked, bounds, first = [], [], [], [], [0]
        for s in self.slots:
            for e, (kind, t, i) in zip(s.files, s.refs):
                run_file.append(self._index_of[e[0]])
                run_entry.append(self._entry_at[(s.level, kind, t, i)])
                run_masked.append(1 if s.kind in (SLOT_WB, SLOT_REST) else 0)
                bounds += [bytes(e[2]), bytes(e[3])]
            first.append(len(run_file))
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev) if v else _buf(0, torch.int64, dev)
        self.run_file, self.run_entry = t64(run_file), t64(run_entry)
        self.run_masked = torch.tensor(run_masked, dtype=torch.bool, device=dev) if run_masked else \
            torch.zeros(0, dtype=torch.bool, device=dev)
        boff = np.zeros(len(bounds) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bounds], out=boff[1:])
        self.bounds = _buf(int(boff[-1]), torch.uint8, dev)
        if boff[-1]:
            self.bounds.copy_(torch.from_numpy(np.frombuffer(b"".join(bounds), dtype=np.uint8).copy()))
        self.bound_offsets = torch.from_numpy(boff).to(dev)
        self.run_first = t64(first)
        self.run_flags = torch.tensor([s.flags for s in self.slots], dtype=torch.int32, device=dev)
        self.slot_info = torch.tensor([s.kind | (s.level << 8) for s in self.slots], dtype=torch.int32, device=dev)
        self._slot_files = [[self._index_of[e[0]] for e in s.files] for s in self.slots]
        return self

    @classmethod
    def from_manifest(cls, image, files, compaction_buffer_length=(0, 20, 20, 3), comparator=BYTEWISE, **params):
        """manifest.recover(image, host_files=False), sorted_tables, then the
        constructor.  A MANIFEST that does not recover raises ValueError with
        Recover's status."""
        from . import manifest
        r = manifest.recover(image, comparator, host_files=False)
        if not r.ok:
            raise ValueError(r.status)
        e, live = r[-2], r[-1]
        tables = sorted_tables(e.new_items[:, :5], live, e.keys, e.key_offsets, compaction_buffer_length, comparator)
        return cls(tables, files, **params)

    # -- the steps of get()

    def _params(self):
        torch = _torch()
        dev = self.device
        use = self.use_length
        wb = [int(self.buffered_merge and level > 1 and use[level - 1] > 0) for level in range(kNumLevels)]
        blob = b"".join(self.read_cursor_keys)
        coff = np.zeros(kNumLevels + 1, dtype=np.int64)
        np.cumsum([len(k) for k in self.read_cursor_keys], out=coff[1:])
        ckeys = _buf(len(blob), torch.uint8, dev)
        if blob:
            ckeys.copy_(torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()))
        return (torch.tensor(use, dtype=torch.int32, device=dev), torch.tensor(wb, dtype=torch.int32, device=dev),
                ckeys, torch.from_numpy(coff).to(dev))

    def candidates(self, keys, offs):
        """Steps 1 and 2 of Version.get's chain for every (query, slot): (file
        int32[n, S], cand uint8[S, n], state int32[S, n], handle int64[S, n, 2],
        status).  No device-to-host read.  That is 25 bytes of device memory per
        (query, slot) pair, kept until the rounds end (about 200 MB for 65,536
        queries over 130 slots): a caller with more queries than memory for
        them splits the batch."""
        torch = _torch()
        from . import block, bloom
        v, dev = self.version, self.device
        n, n_slots = offs.numel() - 1, len(self.slots)
        # FileMetaData::visible is read for WB and REST tables only
        vis = torch.where(self.run_masked, self.visible[self.run_entry], torch.ones_like(self.run_masked,
                                                                                         dtype=torch.uint8)) \
            if self.run_file.numel() else _buf(0, torch.uint8, dev)
        file, st = find_file(self.bounds, self.bound_offsets, self.run_first, self.run_flags, vis.contiguous(), keys,
                             offs)
        cand = torch.zeros((n_slots, n), dtype=torch.uint8, device=dev)
        state_all = torch.full((n_slots, n), SEEK_NOT_VALID, dtype=torch.int32, device=dev)
        handle_all = torch.zeros((n_slots, n, 2), dtype=torch.int64, device=dev)
        zero2 = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        # (a bad status leaves every file word -1: nothing is sought below)
        for s, slot_files in enumerate(self._slot_files):
            if not slot_files:
                continue
            at = file[:, s].to(torch.int64)
            offered = at >= 0
            f = self.run_file[torch.where(offered, at, torch.zeros_like(at))]
            # 1. iiter->Seek(k) with BlockHandle::DecodeFrom; a query without a file seeks an empty handle
            ih = torch.where(offered[:, None], v.index_handle[f], zero2).reshape(-1).contiguous()
            idx = block.seek(v.meta, ih, keys, offs, cmp=INTERNAL_KEY, value_is_handle=True)
            state = torch.where(offered, idx.state, torch.full_like(idx.state, SEEK_NOT_VALID))
            found = state == SEEK_VALID
            handle = torch.where(found[:, None], idx.handle, zero2)
            # 2. filter->KeyMayMatch(handle.offset(), k)
            filtered = torch.zeros_like(found)
            for bits in sorted({v._bits[i] for i in slot_files if v._bits[i] >= 0}):
                probe = found & (v.file_bits[f] == bits)
                fh = torch.where(probe[:, None], v.filter_handle[f], zero2).reshape(-1).contiguous()
                may, _ = bloom.filter_block_may_match(v.meta, fh, handle[:, 0].contiguous(), keys, offs, int(bits),
                                                      strip=8)
                filtered |= probe & (may == 0)
            # a handle that does not decode leaves the iterator valid: the read then fails (BlockReader)
            code = torch.full_like(state, CAND_MISS)
            code = torch.where((found & ~filtered) | (state == SEEK_BAD_HANDLE), torch.full_like(code, CAND_MAY), code)
            code = torch.where((state == SEEK_BAD_ENTRY) | (state == SEEK_BAD_CONTENTS),
                               torch.full_like(code, CAND_ERR), code)
            code = torch.where(offered, code, torch.full_like(code, CAND_NONE))
            cand[s] = code.to(torch.uint8)
            state_all[s] = state
            handle_all[s] = handle
        return file, cand, state_all, handle_all, st

    def plan(self, cand, keys, offs):
        """(count int32[n], probe_first int64[n + 1], status): lsbm_probe_plan_dev
        and the prefix sum."""
        torch = _torch()
        use, wb, ckeys, coff = self._params()
        count, st = probe_plan(cand.reshape(-1), self.slot_info, use, wb, ckeys, coff, keys, offs)
        first = torch.zeros(offs.numel(), dtype=torch.int64, device=self.device)
        torch.cumsum(count, 0, out=first[1:])
        return count, first, st, (use, wb, ckeys, coff)

    @on_stream
    def get(self, user_keys, key_offsets, snapshot, memtables=(), verify=True, stream=None):
        """Version::Get for a batch of user keys at `snapshot`, after `memtables`:
        db.Version.get's signature and result, DbGetResult(status, values,
        value_offsets, where) with where = memtable i: i; slot s: len(memtables)
        + s; -1: none.

        Candidates for every (query, slot), the probe plan, then rounds: round
        j reads, for every query still undecided with more than j probes, the
        data block of its j-th probe (steps 3 to 6 of db.Version.get's chain).
        The host reads the probes' total and largest count once and one number
        or two per round, besides what sstable.read_blocks and torch.unique
        read; nothing per slot or per sorted table."""
        torch = _torch()
        from . import block, sstable
        v, dev = self.version, self.device
        keys, offs, st = lookup_keys(user_keys, key_offsets, snapshot)
        n = offs.numel() - 1
        verdict, value, where = new_verdicts(n, dev)
        images, bad = [], st.clone()
        n_mem = len(memtables)
        if n == 0:
            return _collect(verdict, value, where, images)
        for i, mem in enumerate(memtables):
            bad |= memtable_probe(mem, keys, offs, i, verdict, value, where)
            images.append((i, i + 1, mem.image))
        if not self.run_file.numel():
            _status_ok(bad, "BufferedVersion.get")
            return _collect(verdict, value, where, images)
        file, cand, state_all, handle_all, st = self.candidates(keys, offs)
        bad |= st
        count, first, st, params = self.plan(cand, keys, offs)
        bad |= torch.where(st != PROBE_OK, torch.full_like(st, PROBE_BAD_INPUT), st)
        total, rounds, status = torch.stack([first[-1], count.max().to(torch.int64), bad[0].to(torch.int64)]).cpu().tolist()
        if status:
            _status_ok(bad, "BufferedVersion.get")
        probe_slot = _buf(max(total, 1), torch.int32, dev)  # (zeros: slot 0 where an emit that fails stores nothing)
        bad |= probe_emit(cand.reshape(-1), self.slot_info, *params, keys, offs, first, probe_slot, total)
        klen = offs[1:] - offs[:-1]
        zero2 = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        qi = torch.arange(n, device=dev)
        decided_slot = torch.zeros(n, dtype=torch.int64, device=dev)
        for j in range(rounds):
            source = n_mem + j
            live = (verdict == UNDECIDED) & (count > j)
            if not int(live.sum().cpu()):
                break
            slot = probe_slot[torch.where(live, first[:-1] + j, torch.zeros_like(first[:-1]))].to(torch.int64)
            # (inside [0, S) whatever probe_slot holds: the gathers below never leave their tensors)
            slot = torch.where(live, slot, torch.zeros_like(slot)).clamp_(0, len(self.slots) - 1)
            at = file[qi, slot].to(torch.int64)
            live = live & (at >= 0)
            f = self.run_file[torch.where(live, at, torch.zeros_like(at))]
            state = torch.where(live, state_all[slot, qi], torch.full_like(state_all[0], SEEK_NOT_VALID))
            live = state == SEEK_VALID
            handle = torch.where(live[:, None], handle_all[slot, qi], zero2)
            # 3. the handle inside its file, then moved by the file's place in the arena
            room = v.file_size[f] - kBlockTrailerSize - handle[:, 0]
            inside = (handle[:, 0] >= 0) & (handle[:, 1] >= 0) & (handle[:, 0] <= v.file_size[f]) & \
                (handle[:, 1] <= room)
            state = torch.where(live & ~inside, torch.full_like(state, SEEK_BAD_HANDLE), state)
            live = live & inside
            moved = torch.stack([handle[:, 0] + v.file_base[f], handle[:, 1]], 1)
            # 4. ReadBlock of the distinct data blocks
            asked = torch.where(live[:, None], moved, torch.full_like(moved, -1))
            blocks, which = torch.unique(asked, dim=0, return_inverse=True)
            contents, out_handles, bstatus = sstable.read_blocks(v.arena, blocks.reshape(-1).contiguous(), verify)
            bstate = sstable._get_state_of(bstatus.to(torch.int64))[which].to(torch.int32)
            state = torch.where(live, bstate, state)
            live = state == SEEK_VALID
            # 5. block_iter->Seek(k), the found key into a window of the lookup key's length
            dh = torch.where(live[:, None], out_handles.view(-1, 2)[which], zero2).reshape(-1).contiguous()
            seek_image = contents if contents.numel() else torch.zeros(1, dtype=torch.uint8, device=dev)
            window = torch.empty(max(keys.numel(), 1), dtype=torch.uint8, device=dev)
            dat = block.seek(seek_image, dh, keys, offs, cmp=INTERNAL_KEY, found=window, found_offsets=offs)
            state = torch.where(live, dat.state, state).contiguous()
            longer = (state == SEEK_VALID) & (dat.key_len > klen)
            found_offsets = offs
            if int(longer.sum().cpu()):
                sizes = torch.where(longer, dat.key_len, klen)
                found_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                torch.cumsum(sizes, 0, out=found_offsets[1:])
                window = torch.empty(int(found_offsets[-1].cpu()), dtype=torch.uint8, device=dev)
                dat = block.seek(seek_image, dh, keys, offs, cmp=INTERNAL_KEY, found=window,
                                 found_offsets=found_offsets)
            # 6. SaveValue and the switch; the round is the source, the slot goes into where below
            bad |= save_value(state, dat.key_len, window, found_offsets, dat.value.reshape(-1).contiguous(), keys, offs,
                              source, verdict, value, where)
            decided_slot = torch.where(where == source, slot, decided_slot)
            images.append((source, source + 1, contents))
        _status_ok(bad, "BufferedVersion.get")
        r = _collect(verdict, value, where, images)
        in_slot = where >= n_mem
        return DbGetResult(r.status, r.values, r.value_offsets,
                           torch.where(in_slot, (n_mem + decided_slot).to(torch.int32), where))
