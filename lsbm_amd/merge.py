"""Compaction merge (MergingIterator of lsbm's table/merger.cc, the drop rule
and the output-file cut of DoCompactionWork, lsbm/db_impl.cc) on the GPU.

Thin wrappers over include/lsbm_merge.h.  Device tensors in, device tensors
out; every call enqueues on `stream` (default: torch's current stream).

    plan(keys, key_offsets, run_first, ...)
                                      which input entry becomes which output
                                      entry: the stable merge by (key, run,
                                      position) and, with drop, the drop rule
    gather(keys, key_offsets, values, plan, ...)
                                      the output entries in the input's shape;
                                      value bytes are not moved
    merge(keys, key_offsets, values, run_first, ...)
                                      plan + gather, sized to the output
    cut_tables(block_first, block_bytes, max_file_size)
                                      where DoCompactionWork closes its output
                                      files (host arithmetic over a plan)
    compact(images, data_handles, max_file_size, ...)
                                      input table images -> output table files:
                                      scan, decode, merge, plan, cut, table_build

Entries are what block.decode returns and block_build reads: a uint8 key buffer
plus int64 offsets and int64 {offset, length} value slices.  Run r owns entries
[run_first[r], run_first[r+1]).
"""
from collections import namedtuple

import numpy as np

from ._lib import check, lib
from .block import BYTEWISE, INTERNAL_KEY
from .engine import _check_tensors, _ptr, _raise_on, _require_cuda, _stream_ptr, _torch

# per-run status (include/lsbm_merge.h)
MERGE_OK = 0
MERGE_NO_ROOM = 1     # gather: the caps are smaller than the output
MERGE_BAD_INPUT = 2
MERGE_UNSORTED = 3
MAX_RUNS = 64
MERGE_DROP = 0x1
MERGE_BOTTOM_LEVEL = 0x2
kMaxSequenceNumber = (1 << 56) - 1  # common/dbformat.h

STATUS_MESSAGE = {MERGE_NO_ROOM: "merge output window too small", MERGE_BAD_INPUT: "bad merge input",
                  MERGE_UNSORTED: "run is not sorted"}

PlanResult = namedtuple("PlanResult", "source out_key_offsets counts run_status")
GatherResult = namedtuple("GatherResult", "keys key_offsets values status")
MergeResult = namedtuple("MergeResult", "keys key_offsets values source run_status")
OutputTable = namedtuple("OutputTable", "image data_handles index_handle")


def _check(**ts):
    _check_tensors(ts, u8=("keys", "out_keys"))


def _flags(cmp, drop, smallest_snapshot, bottom_level):
    if cmp not in (BYTEWISE, INTERNAL_KEY):
        raise ValueError("unknown comparator")
    if not drop:
        return 0, 0
    if cmp != INTERNAL_KEY:
        raise ValueError("the drop rule needs internal keys")
    if smallest_snapshot is None:
        raise ValueError("drop needs smallest_snapshot")
    if not 0 <= int(smallest_snapshot) <= kMaxSequenceNumber:
        raise ValueError("smallest_snapshot is a 56-bit sequence number")
    return MERGE_DROP | (MERGE_BOTTOM_LEVEL if bottom_level else 0), int(smallest_snapshot)


def plan(keys, key_offsets, run_first, cmp=INTERNAL_KEY, drop=False, smallest_snapshot=None, bottom_level=False,
         stream=None):
    """PlanResult(source int64[n], out_key_offsets int64[n + 1], counts int64[2]
    = {n_out, output key bytes}, run_status int32[n_runs]); source and
    out_key_offsets are used up to n_out."""
    torch = _torch()
    _require_cuda(keys, key_offsets, run_first)
    _check(keys=keys, key_offsets=key_offsets, run_first=run_first)
    flags, snapshot = _flags(cmp, drop, smallest_snapshot, bottom_level)
    n = key_offsets.numel() - 1
    n_runs = run_first.numel() - 1
    if n < 0 or n_runs < 0:
        raise ValueError("key_offsets and run_first need at least one entry")
    dev = keys.device
    source = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)[:n]
    out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    run_status = torch.zeros(max(n_runs, 1), dtype=torch.int32, device=dev)[:n_runs]
    scratch_bytes = lib().lsbm_merge_scratch_bytes(n, n_runs)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().lsbm_merge_plan_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), n, _ptr(run_first), n_runs,
                                    int(cmp), flags, snapshot, _ptr(source), _ptr(out_off), _ptr(counts),
                                    _ptr(run_status), _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_merge_plan_dev")
    return PlanResult(source, out_off, counts, run_status)


def gather(keys, key_offsets, values, plan_result, out_keys=None, out_key_offsets=None, out_values=None,
           stream=None):
    """GatherResult(keys, key_offsets, values int64[cap, 2], status int32[1]).
    Without out_* the outputs are input-sized, which always suffices; the
    output's true extent is plan_result.counts."""
    torch = _torch()
    _require_cuda(keys, key_offsets, values, out_keys, out_key_offsets, out_values)
    _check(keys=keys, key_offsets=key_offsets, values=values, out_keys=out_keys, out_key_offsets=out_key_offsets,
           out_values=out_values)
    n = key_offsets.numel() - 1
    if n < 0 or values.numel() != 2 * n:
        raise ValueError("values must be one {offset, length} pair per entry")
    dev = keys.device
    if out_keys is None:
        out_keys = torch.zeros(max(keys.numel(), 1), dtype=torch.uint8, device=dev)[:keys.numel()]
    if out_key_offsets is None:
        out_key_offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if out_values is None:
        out_values = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev)[:n]
    cap = min(out_key_offsets.numel() - 1, out_values.numel() // 2)
    if cap < 0:
        raise ValueError("out_key_offsets needs at least one entry")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = plan_result
    check(lib().lsbm_merge_gather_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), _ptr(values), n, _ptr(p.source),
                                      _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(out_keys), out_keys.numel(),
                                      _ptr(out_key_offsets), _ptr(out_values), cap, _ptr(status),
                                      _stream_ptr(stream)), "lsbm_merge_gather_dev")
    return GatherResult(out_keys, out_key_offsets, out_values, status)


def merge(keys, key_offsets, values, run_first, cmp=INTERNAL_KEY, drop=False, smallest_snapshot=None,
          bottom_level=False, stream=None):
    """MergeResult(keys, key_offsets int64[n_out + 1], values int64[n_out, 2],
    source int64[n_out], run_status int32[n_runs]).  plan and gather run back
    to back; the one device -> host read (n_out and the key bytes, to trim the
    tensors) comes after both.  With a run in error the output is empty and
    run_status says why."""
    torch = _torch()
    if stream is not None:  # (the trimming is torch's: on the same stream)
        with torch.cuda.stream(stream):
            return merge(keys, key_offsets, values, run_first, cmp, drop, smallest_snapshot, bottom_level)
    _require_cuda(values)
    values = values.reshape(-1)
    p = plan(keys, key_offsets, run_first, cmp, drop, smallest_snapshot, bottom_level)
    g = gather(keys, key_offsets, values, p)
    n_out, key_bytes = (int(x) for x in p.counts.cpu())
    st = int(g.status.cpu()[0])
    if st != MERGE_OK:
        raise ValueError(f"gather: {STATUS_MESSAGE.get(st, st)}")
    return MergeResult(g.keys[:key_bytes], g.key_offsets[:n_out + 1], g.values[:n_out], p.source[:n_out],
                       p.run_status)


def cut_tables(block_first, block_bytes, max_file_size):
    """DoCompactionWork's output-file cut (lsbm/db_impl.cc:1056-1064) over the
    single-table plan of the merged entries: TableBuilder::FileSize() grows only
    when a block is flushed, by the block and its 5-byte trailer, so table t
    ends after the first block at which the sum of block_bytes + 5 since its
    start reaches max_file_size, and the last block closes the last table.
    block_first has one slot more than block_bytes.  Returns (table_first,
    table_block_first): table t owns entries [table_first[t], table_first[t+1])
    and blocks [table_block_first[t], table_block_first[t+1])."""
    block_first = [int(x) for x in block_first]
    block_bytes = [int(x) for x in block_bytes]
    if len(block_first) != len(block_bytes) + 1:
        raise ValueError("block_first needs one slot more than block_bytes")
    table_first, table_block_first, size = [block_first[0]], [0], 0
    for b, nbytes in enumerate(block_bytes):
        size += nbytes + 5
        if size >= max_file_size or b + 1 == len(block_bytes):
            table_first.append(block_first[b + 1])
            table_block_first.append(b + 1)
            size = 0
    return table_first, table_block_first


def _get_varint64(buf, p):
    v, shift = 0, 0
    while True:
        b = buf[p]
        p += 1
        v |= (b & 127) << shift
        if b < 128:
            return v, p
        shift += 7


def index_data_handles(image, index_handle):
    """The data block handles an index block lists (BlockHandle::DecodeFrom of
    every index value), as an int64 numpy array of {offset, size} pairs."""
    from . import block
    torch = _torch()
    ih = torch.tensor([int(index_handle[0]), int(index_handle[1])], dtype=torch.int64, device=image.device)
    _, _, values, _, st = block.decode(image, ih)
    if int(st.cpu()[0]) != block.BLOCK_OK:
        raise ValueError("index block: " + block.STATUS_MESSAGE.get(int(st.cpu()[0]), "bad"))
    lo, hi = int(index_handle[0]), int(index_handle[0]) + int(index_handle[1])
    buf = image[lo:hi].cpu().numpy().tobytes()
    out = []
    for off, _ in values.cpu().tolist():
        o, p = _get_varint64(buf, off - lo)
        s, _ = _get_varint64(buf, p)
        out += [o, s]
    return np.array(out, dtype=np.int64)


def compact(images, data_handles=None, max_file_size=2 << 20, index_handles=None, cmp=INTERNAL_KEY, drop=False,
            smallest_snapshot=None, bottom_level=False, block_size=4096, restart_interval=16, bits_per_key=None,
            stream=None):
    """The table-to-table part of DoCompactionWork for device-resident
    kNoCompression tables (sstable.compact: either block type): images[t] is input table t's file image and
    data_handles[t] its data blocks' {offset, size} pairs (or index_handles[t]
    its index block's (offset, size), from which they are read).  Input t is
    run t of the merge, so list the inputs as the reference's MergingIterator
    has them: for equal keys the earlier table wins.

    On one stream: the images are concatenated into one value image, every
    data block is scanned and decoded (block.scan / block.decode), the runs are
    merged (merge), the output is planned as one table (block_build.plan), cut
    into tables by max_file_size (cut_tables) and each table is written by
    block_build.table_build.  No entry touches the host; the host reads counts
    and block sizes.  Returns [OutputTable(image, data_handles, index_handle)]."""
    torch = _torch()
    from . import block, block_build
    if stream is not None:
        with torch.cuda.stream(stream):
            return compact(images, data_handles, max_file_size, index_handles, cmp, drop, smallest_snapshot,
                           bottom_level, block_size, restart_interval, bits_per_key)
    if (data_handles is None) == (index_handles is None):
        raise ValueError("give data_handles or index_handles")
    if len(images) > MAX_RUNS:
        raise ValueError(f"at most {MAX_RUNS} input tables")
    if int(max_file_size) < 1:
        raise ValueError("max_file_size must be at least 1")
    _require_cuda(*images)
    if not images:
        return []
    dev = images[0].device
    if data_handles is None:
        data_handles = [index_data_handles(img, ih) for img, ih in zip(images, index_handles)]
    if len(data_handles) != len(images):
        raise ValueError("one set of handles per image")
    # 1. one value image; every handle moves by its image's place in it
    image = torch.cat([img.reshape(-1) for img in images])
    handles, blocks_before, base = [], [0], 0
    for img, h in zip(images, data_handles):
        h = torch.as_tensor(np.asarray(h.cpu() if hasattr(h, "cpu") else h, dtype=np.int64).reshape(-1, 2).copy())
        h[:, 0] += base
        handles.append(h)
        blocks_before.append(blocks_before[-1] + h.shape[0])
        base += img.numel()
    handles = torch.cat(handles).reshape(-1).contiguous().to(dev)
    # 2. the entries of every data block, one run per input table
    counts, st = block.scan(image, handles)
    _raise_on(st, "scan")
    nb = counts.shape[0]
    entry_base = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    key_base = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    if nb:
        torch.cumsum(counts[:, 0], 0, out=entry_base[1:])
        torch.cumsum(counts[:, 1], 0, out=key_base[1:])
    keys, key_offsets, values, _, st = block.decode(image, handles, entry_base, key_base)
    _raise_on(st, "decode")
    run_first = entry_base[torch.tensor(blocks_before, dtype=torch.int64, device=dev)].contiguous()
    # 3. the merge, the single-table plan of its output, the cut
    m = merge(keys, key_offsets, values, run_first, cmp, drop, smallest_snapshot, bottom_level)
    bad = [(r, int(s)) for r, s in enumerate(m.run_status.cpu().tolist()) if s != MERGE_OK]
    if bad:
        raise ValueError(f"input table {bad[0][0]}: {STATUS_MESSAGE.get(bad[0][1], bad[0][1])}")
    n_out = m.key_offsets.numel() - 1
    if n_out == 0:
        return []
    m_values = m.values.reshape(-1).contiguous()
    p = block_build.plan(m.keys, m.key_offsets, m_values, torch.tensor([0, n_out], dtype=torch.int64, device=dev),
                         block_size, restart_interval)
    _raise_on(p.status, "plan")
    n_blocks = int(p.table_block_first[-1])
    table_first, _ = cut_tables(p.block_first[:n_blocks + 1].cpu().tolist(), p.block_bytes[:n_blocks].cpu().tolist(),
                                int(max_file_size))
    # 4. each output table's slice of the merged entries -> its file
    out = []
    key_at = m.key_offsets[torch.tensor(table_first, dtype=torch.int64, device=dev)].cpu().tolist()
    for t in range(len(table_first) - 1):
        e0, e1 = table_first[t], table_first[t + 1]
        t_off = (m.key_offsets[e0:e1 + 1] - key_at[t]).contiguous()
        t_keys = m.keys[key_at[t]:key_at[t + 1]].contiguous()
        t_values = m_values[2 * e0:2 * e1].contiguous()
        out.append(OutputTable(*block_build.table_build(t_keys, t_off, t_values, image, cmp, block_size,
                                                        restart_interval, bits_per_key)))
    return out
