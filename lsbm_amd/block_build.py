"""SSTable block builder (BlockBuilder of lsbm's table/block_builder.cc, the
flush rule and index block of table/table_builder.cc) on the GPU.

Thin wrappers over include/lsbm_block_build.h.  Device tensors in, device
tensors out; every call runs on `stream` (default: torch's current stream; the contract is engine.py's).

    plan(keys, key_offsets, values, table_first, ...)
                                      where TableBuilder::Add ends each block
                                      (table/table_builder.cc:137-140) and the
                                      size Finish() will return
    build(keys, key_offsets, values, value_image, block_first, out, out_handles, ...)
                                      BlockBuilder::Add for every entry of every
                                      block, then Finish, into windows of `out`
    index_block(keys, key_offsets, block_first, table_block_first, data_handles, ...)
                                      one index block per table: separators,
                                      successor, BlockHandle::EncodeTo
    table_build(keys, key_offsets, values, value_image, ...)
                                      one complete kNoCompression table file:
                                      sstable.write_table without compression

Entries are what block.decode returns: a uint8 key buffer plus int64 offsets
(key e = keys[off[e], off[e+1])) and int64 {offset, length} value slices of
`value_image`.  Handles are int64 {offset, size} pairs.
"""
from collections import namedtuple

from ._lib import check, lib
from .block import INTERNAL_KEY
from .engine import _check_tensors, _ptr, _raise_on as _raise_on_status, _require_cuda, _stream_ptr, _torch, on_stream
from .table import kNoCompression

# per-block / per-table status (include/lsbm_block_build.h)
BUILD_OK = 0
BUILD_NO_ROOM = 1     # the window is smaller than the block
BUILD_BAD_INPUT = 2
BUILD_TOO_LARGE = 3   # the block's contents would reach 2^32 bytes

STATUS_MESSAGE = {BUILD_NO_ROOM: "block window too small", BUILD_BAD_INPUT: "bad block builder input",
                  BUILD_TOO_LARGE: "block would reach 2^32 bytes"}

kTableMagicNumber = 0xdb4775248b80fb57  # table/format.h:81
kFooterEncodedLength = 48               # table/format.h:70
FILTER_KEY = b"filter.leveldb.BuiltinBloomFilter"  # "filter." + BloomFilterPolicy::Name()

PlanResult = namedtuple("PlanResult", "block_first block_bytes table_block_first status")


def _check(**ts):
    _check_tensors(ts, u8=("keys", "value_image", "out"))


def _n_entries(key_offsets, values=None):
    n = key_offsets.numel() - 1
    if n < 0:
        raise ValueError("key_offsets needs at least one entry")
    if values is not None and values.numel() != 2 * n:
        raise ValueError("values must be one {offset, length} pair per entry")
    return n


@on_stream
def plan(keys, key_offsets, values, table_first, block_size=4096, restart_interval=16, blocks_cap=None,
         stream=None):
    """PlanResult(block_first int64[blocks_cap + 1], block_bytes int64[blocks_cap],
    table_block_first int64[n_tables + 1], status int32[n_tables]).  The true
    block count is table_block_first[-1]; blocks_cap defaults to the entry
    count, which always suffices (a block holds at least one entry)."""
    torch = _torch()
    _require_cuda(keys, key_offsets, values, table_first)
    _check(keys=keys, key_offsets=key_offsets, values=values, table_first=table_first)
    n = _n_entries(key_offsets, values)
    n_tables = table_first.numel() - 1
    if n_tables < 0:
        raise ValueError("table_first needs at least one entry")
    cap = n if blocks_cap is None else int(blocks_cap)
    dev = keys.device
    block_first = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    block_bytes = torch.zeros(cap, dtype=torch.int64, device=dev)
    table_block_first = torch.zeros(n_tables + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(n_tables, dtype=torch.int32, device=dev)
    scratch_bytes = lib().lsbm_block_plan_scratch_bytes(n, n_tables)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    check(lib().lsbm_block_plan_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), _ptr(values), n,
                                    _ptr(table_first), n_tables, int(block_size), int(restart_interval),
                                    _ptr(block_first), _ptr(block_bytes), cap, _ptr(table_block_first),
                                    _ptr(status), _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_block_plan_dev")
    return PlanResult(block_first, block_bytes, table_block_first, status)


@on_stream
def build(keys, key_offsets, values, value_image, block_first, out, out_handles, restart_interval=16,
          stream=None):
    """Block b = entries [block_first[b], block_first[b+1]) written at the start
    of out[out_handles[2b], + out_handles[2b+1]).  Returns (built_bytes
    int64[n_blocks], status int32[n_blocks])."""
    torch = _torch()
    _require_cuda(keys, key_offsets, values, value_image, block_first, out, out_handles)
    _check(keys=keys, key_offsets=key_offsets, values=values, value_image=value_image,
           block_first=block_first, out=out, out_handles=out_handles)
    n = _n_entries(key_offsets, values)
    n_blocks = block_first.numel() - 1
    if n_blocks < 0 or out_handles.numel() != 2 * n_blocks:
        raise ValueError("block_first needs n_blocks + 1 entries and out_handles one pair per block")
    dev = keys.device
    built = torch.zeros(n_blocks, dtype=torch.int64, device=dev)
    status = torch.zeros(n_blocks, dtype=torch.int32, device=dev)
    check(lib().lsbm_block_build_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), _ptr(values),
                                     _ptr(value_image), value_image.numel(), n, _ptr(block_first), n_blocks,
                                     int(restart_interval), _ptr(out), out.numel(), _ptr(out_handles),
                                     _ptr(built), _ptr(status), _stream_ptr(stream)), "lsbm_block_build_dev")
    return built, status


@on_stream
def index_block(keys, key_offsets, block_first, table_block_first, data_handles, cmp=INTERNAL_KEY,
                out=None, out_handles=None, stream=None):
    """One index block per table (blocks [table_block_first[t],
    table_block_first[t+1]) with handles data_handles) at the start of
    out[out_handles[2t], + out_handles[2t+1]); without `out` only the sizes.
    Returns (built_bytes int64[n_tables], status int32[n_tables])."""
    torch = _torch()
    _require_cuda(keys, key_offsets, block_first, table_block_first, data_handles, out, out_handles)
    _check(keys=keys, key_offsets=key_offsets, block_first=block_first, table_block_first=table_block_first,
           data_handles=data_handles, out=out, out_handles=out_handles)
    n = _n_entries(key_offsets)
    n_blocks = block_first.numel() - 1
    n_tables = table_block_first.numel() - 1
    if n_blocks < 0 or n_tables < 0 or data_handles.numel() != 2 * n_blocks:
        raise ValueError("block_first / table_block_first need n + 1 entries, data_handles one pair per block")
    if (out is None) != (out_handles is None):
        raise ValueError("out and out_handles come together")
    if out_handles is not None and out_handles.numel() != 2 * n_tables:
        raise ValueError("out_handles needs one pair per table")
    dev = keys.device
    built = torch.zeros(n_tables, dtype=torch.int64, device=dev)
    status = torch.zeros(n_tables, dtype=torch.int32, device=dev)
    check(lib().lsbm_index_block_build_dev(_ptr(keys), keys.numel(), _ptr(key_offsets), n, _ptr(block_first),
                                           n_blocks, _ptr(table_block_first), n_tables, _ptr(data_handles),
                                           int(cmp), _ptr(out), out.numel() if out is not None else 0,
                                           _ptr(out_handles), _ptr(built), _ptr(status), _stream_ptr(stream)),
          "lsbm_index_block_build_dev")
    return built, status


def _raise_on(status, what):
    _raise_on_status(status, what, BUILD_OK, STATUS_MESSAGE)


@on_stream
def table_build(keys, key_offsets, values, value_image, cmp=INTERNAL_KEY, block_size=4096,
                restart_interval=16, bits_per_key=None, compression=kNoCompression, stream=None):
    """TableBuilder (table/table_builder.cc) Add for every entry, then Finish,
    for one complete table file: data blocks, the filter block
    (BloomFilterPolicy(bits_per_key); InternalFilterPolicy under INTERNAL_KEY),
    the metaindex block, the index block, every trailer and the footer
    (kNoCompression only; sstable.write_table writes snappy-compressed tables,
    and this is it with compression=kNoCompression).  Returns (file_image uint8
    device tensor, data_handles int64 device tensor of {offset, size} pairs,
    index_handle (offset, size))."""
    from . import sstable
    if compression != kNoCompression:
        raise ValueError("table_build writes kNoCompression tables only")
    return sstable.write_table(keys, key_offsets, values, value_image, cmp, block_size, restart_interval,
                               bits_per_key, kNoCompression, stream)
