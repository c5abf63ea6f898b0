"""Compaction merge (MergingIterator of lsbm's table/merger.cc, the drop rule
and the output-file cut of DoCompactionWork, lsbm/db_impl.cc) on the GPU.

Thin wrappers over include/lsbm_merge.h.  Device tensors in, device tensors
out; every call runs on `stream` (default: torch's current stream; the contract is engine.py's).

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
                                      scan, decode, merge, plan, cut and
                                      sstable.finish_tables (one body with
                                      sstable.compact)

Entries are what block.decode returns and block_build reads: a uint8 key buffer
plus int64 offsets and int64 {offset, length} value slices.  Run r owns entries
[run_first[r], run_first[r+1]).
"""
from collections import namedtuple

from ._lib import check, lib
from .block import BYTEWISE, INTERNAL_KEY
from .engine import _check_tensors, _ptr, _require_cuda, _stream_ptr, _torch, on_stream
from .table import kNoCompression

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


@on_stream
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


@on_stream
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


@on_stream
def merge(keys, key_offsets, values, run_first, cmp=INTERNAL_KEY, drop=False, smallest_snapshot=None,
          bottom_level=False, stream=None):
    """MergeResult(keys, key_offsets int64[n_out + 1], values int64[n_out, 2],
    source int64[n_out], run_status int32[n_runs]).  plan and gather run back
    to back; the one device -> host read (n_out and the key bytes, to trim the
    tensors) comes after both.  With a run in error the output is empty and
    run_status says why."""
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


def index_data_handles(image, index_handle):
    """The data block handles an index block lists (BlockHandle::DecodeFrom of
    every index value), as an int64 numpy array of {offset, size} pairs."""
    from . import sstable
    return sstable._index_data_handles(image, index_handle, None, sstable._in_place)


@on_stream
def compact(images, data_handles=None, max_file_size=2 << 20, index_handles=None, cmp=INTERNAL_KEY, drop=False,
            smallest_snapshot=None, bottom_level=False, block_size=4096, restart_interval=16, bits_per_key=None,
            stream=None):
    """The table-to-table part of DoCompactionWork for device-resident
    kNoCompression tables (sstable.compact: either block type): images[t] is
    input table t's file image and data_handles[t] its data blocks' {offset,
    size} pairs (or index_handles[t] its index block's (offset, size), from
    which they are read).  Input t is run t of the merge, so list the inputs as
    the reference's MergingIterator has them: for equal keys the earlier table
    wins.

    On one stream: the images are concatenated into one value image, every
    data block is scanned and decoded where it lies (block.scan / block.decode:
    no ReadBlock, no trailer is verified), the runs are merged (merge), the
    output is planned as one table (block_build.plan) and its data blocks are
    built, the blocks are cut into tables by max_file_size (cut_tables) and
    sstable.finish_tables finishes every table in one chain.  This is
    sstable.compact's body with another way to a block's contents.  No entry
    touches the host; the host reads counts and block sizes.  Returns
    [OutputTable(image, data_handles, index_handle)]; the images are views of
    one arena, so holding one keeps the whole arena alive."""
    from . import sstable
    return sstable._compact(sstable._in_place, images, data_handles, max_file_size, index_handles, cmp, drop,
                            smallest_snapshot, bottom_level, block_size, restart_interval, bits_per_key,
                            kNoCompression, None)
