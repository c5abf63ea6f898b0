"""SSTables with either block type (kNoCompression / kSnappyCompression) on the
GPU: TableBuilder::WriteBlock's keep rule and ReadBlock's type switch of lsbm's
table/ layer, and the table writer, Get and compaction built on them.

Thin wrappers over include/lsbm_table_pack.h and the other modules.  Device
tensors in, device tensors out; every call runs on `stream` (default:
torch's current stream; the contract is engine.py's).

    pack_plan(raw_len, comp_len, ...)  the keep rule (table/table_builder.cc:187)
                                       and the offsets that follow from it
    pack(raw, raw_handles, comp, comp_offsets, types, handles, out, ...)
                                       every block, raw or compressed, moved to
                                       its final offset
    read_blocks(image, handles, ...)   batched ReadBlock (table/format.cc:66-148)
    pack_plan_tables, filter_layout, metaindex_blocks, place_tables
                                       include/lsbm_table_write.h: the pack plan
                                       restarting at every table, every table's
                                       filter-block layout, metaindex block and
                                       footer, and the handles at their bases
    finish_tables(keys, key_offsets, block_first, table_block_first, blocks, ...)
                                       TableBuilder from the first WriteBlock to
                                       the footer for many tables in one chain
    write_tables(keys, key_offsets, values, value_image, table_first, ...)
                                       TableBuilder with WriteBlock's rule on the
                                       data, metaindex and index blocks, for many
                                       tables at once: the one table writer
    write_table(keys, key_offsets, values, value_image, ...)
                                       write_tables of one table
    table_get(image, index_handle, keys, key_offsets, ...)
                                       Table::InternalGet over either block type
    compact(images, ...)               merge.compact over either block type

Handles are int64 {offset, size} pairs.  Every table of the library is written
by write_tables / finish_tables: block_build.table_build, memtable.flush and
flush_many plan their entries through write_tables, and merge.compact and
compact finish the blocks they have cut through finish_tables.  The tables of
one call are views of one arena, so holding one image keeps the whole arena
alive.  block.table_get, block_build.table_build and merge.compact keep their
kNoCompression-only behaviour.
"""
from collections import namedtuple

import numpy as np

from ._lib import check, lib
from .block import (BYTEWISE, GET_BAD_CHECKSUM, GET_BAD_TYPE, GET_FILTERED, INTERNAL_KEY, SEEK_BAD_HANDLE,
                    SEEK_VALID)
from .engine import _buf, _check_tensors, _ptr, _raise_on, _require_cuda, _stream_ptr, _torch, on_stream
from .merge import OutputTable
from .table import kBlockTrailerSize, kNoCompression, kSnappyCompression, seal_blocks

# per-block status of pack (include/lsbm_block_build.h)
PACK_OK = 0
PACK_NO_ROOM = 1
PACK_BAD_INPUT = 2

# per-block status of read_blocks (include/lsbm_table_pack.h), in ReadBlock's order
READ_OK = 0
READ_TRUNCATED = 1        # Corruption("truncated block read")
READ_BAD_CHECKSUM = 2     # Corruption("block checksum mismatch")
READ_BAD_COMPRESSED = 3   # Corruption("corrupted compressed block contents")
READ_BAD_TYPE = 4         # Corruption("bad block type")
READ_TOO_LARGE = 5        # the preambles ask for more than max_bytes (no reference verdict)

READ_MESSAGE = {READ_TRUNCATED: "truncated block read", READ_BAD_CHECKSUM: "block checksum mismatch",
                READ_BAD_COMPRESSED: "corrupted compressed block contents", READ_BAD_TYPE: "bad block type",
                READ_TOO_LARGE: "compressed blocks ask for more than max_bytes"}

# table_get: block.table_get's states (GET_NEEDS_UNCOMPRESS never appears) and
GET_BAD_COMPRESSED = 9    # the data block does not uncompress, or is READ_TOO_LARGE

COMP_NONE = -1            # comp_len of a block that could not be compressed (UINT64_MAX)

GetResult = namedtuple("GetResult", "state key_len value data_handle value_image")
# data blocks built (and compressed) once, for finish_tables
_Blocks = namedtuple("_Blocks", "raw raw_handles comp comp_offsets comp_len")


def _check(**ts):
    _check_tensors(ts, u8=("image", "raw", "comp", "types", "out", "arena", "filter", "keys"))


def _scratch(n, dev):
    torch = _torch()
    nbytes = int(lib().lsbm_block_pack_scratch_bytes(n))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def keep_compressed(raw_len, comp_len):
    """WriteBlock's rule as lsbm_block_pack_plan_dev evaluates it: unsigned
    64-bit arithmetic, COMP_NONE (UINT64_MAX) never kept."""
    mask = (1 << 64) - 1
    raw_len, comp_len = int(raw_len) & mask, int(comp_len) & mask
    return comp_len != mask and comp_len < ((raw_len - raw_len // 8) & mask)


@on_stream
def pack_plan(raw_len, comp_len=None, first_offset=0, gap=kBlockTrailerSize, stream=None):
    """(types uint8[n], handles int64[2n], end int64[1]): type[i] = 1 where the
    compressed form is kept (comp_len[i] < raw_len[i] - raw_len[i] / 8; comp_len
    None: nowhere), size[i] the kept form's, offset[i] = first_offset + the
    sizes and gaps before it, end = the offset after the last block's gap."""
    torch = _torch()
    _require_cuda(raw_len, comp_len)
    _check(raw_len=raw_len, comp_len=comp_len)
    n = raw_len.numel()
    if comp_len is not None and comp_len.numel() != n:
        raise ValueError("comp_len needs one entry per block")
    dev = raw_len.device
    types = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)[:n]
    handles = torch.zeros(max(2 * n, 1), dtype=torch.int64, device=dev)[:2 * n]
    end = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = _scratch(n, dev)
    check(lib().lsbm_block_pack_plan_dev(_ptr(raw_len), _ptr(comp_len), n, int(first_offset), int(gap),
                                         _ptr(types), _ptr(handles), _ptr(end), _ptr(scratch),
                                         scratch.numel() * 8, _stream_ptr(stream)), "lsbm_block_pack_plan_dev")
    return types, handles, end


@on_stream
def pack(raw, raw_handles, comp, comp_offsets, types, handles, out, gap=kBlockTrailerSize, stream=None):
    """Block i: handles[2i+1] bytes to out[handles[2i]:], from raw[raw_handles[2i]:]
    where types[i] == 0 and from comp[comp_offsets[i]:] where it is 1 (comp /
    comp_offsets may be None when no block is).  Returns status int32[n]."""
    torch = _torch()
    _require_cuda(raw, raw_handles, comp, comp_offsets, types, handles, out)
    _check(out=out, types=types, handles=handles, raw=raw, comp=comp, raw_handles=raw_handles,
           comp_offsets=comp_offsets)
    n = types.numel()
    if handles.numel() != 2 * n or (raw_handles is not None and raw_handles.numel() != 2 * n) or \
            (comp_offsets is not None and comp_offsets.numel() != n):
        raise ValueError("handles / raw_handles need one pair, comp_offsets one entry per block")
    dev = out.device
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)[:n]
    scratch = _scratch(n, dev)
    check(lib().lsbm_block_pack_dev(_ptr(raw), raw.numel() if raw is not None else 0, _ptr(raw_handles),
                                    _ptr(comp), comp.numel() if comp is not None else 0, _ptr(comp_offsets),
                                    _ptr(types), _ptr(handles), n, int(gap), _ptr(out), out.numel(),
                                    _ptr(status), _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_block_pack_dev")
    return status


def _preamble(image, off, size):
    """snappy::GetUncompressedLength of the blocks at off (int64 tensors; only
    where size >= 0 and the block is inside the image): (ulen, ok), with torch
    ops so that the contents image is sized without a read of its own."""
    torch = _torch()
    ulen = torch.zeros_like(off)
    done = torch.zeros_like(off, dtype=torch.bool)
    ok = torch.zeros_like(off, dtype=torch.bool)
    for i in range(5):
        have = ~done & (size > i)
        b = image[torch.where(have, off + i, torch.zeros_like(off))].to(torch.int64)
        bad = have & (b >= 16) if i == 4 else torch.zeros_like(have)
        have = have & ~bad
        ulen = torch.where(have, ulen | ((b & 127) << (7 * i)), ulen)
        last = have & (b < 128)
        ok = ok | last
        done = done | last | bad | ~have
    return torch.where(ok, ulen, torch.zeros_like(ulen)), ok


@on_stream
def read_blocks(image, handles, verify=True, max_bytes=1 << 30, stream=None):
    """Batched ReadBlock (table/format.cc:66-148) of the blocks `handles` names
    in the file image, in the reference's order of checks: the handle plus its
    trailer inside the image (READ_TRUNCATED), the trailer's CRC when `verify`
    (READ_BAD_CHECKSUM), then the type byte: kNoCompression, the bytes as they
    are; kSnappyCompression, GetUncompressedLength and RawUncompress
    (READ_BAD_COMPRESSED when either fails); anything else READ_BAD_TYPE.
    READ_TOO_LARGE (no reference verdict): a compressed block whose preamble
    alone asks for more than max_bytes, and of the others every one at which
    the running sum of the preambles passes max_bytes; nothing is allocated
    for them.

    Returns (contents uint8, out_handles int64[2n], status int32[n]): block i's
    contents are contents[out_handles[2i], + out_handles[2i+1]); a failed block
    has size 0.  contents holds the snappy blocks' outputs, uncompressed
    straight into their places, then the raw blocks, moved by pack, back to back
    (a snappy block that fails in RawUncompress leaves its place unused).  The
    host reads one pair of numbers: the sizes of contents and of the staging of
    the compressed bytes."""
    torch = _torch()
    from . import snappy, table
    _require_cuda(image, handles)
    _check(image=image, handles=handles)
    if handles.numel() % 2:
        raise ValueError("handles must be {offset, size} pairs")
    n = handles.numel() // 2
    dev = image.device
    numel = image.numel()
    if n == 0:
        return (torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev))
    h = handles.view(n, 2)
    off, size = h[:, 0], h[:, 1]
    zero = torch.zeros_like(off)
    inside = (off >= 0) & (size >= 0) & (off <= numel) & (size <= numel - kBlockTrailerSize - off)
    status = torch.where(inside, torch.full_like(off, READ_OK), torch.full_like(off, READ_TRUNCATED))
    safe = torch.where(inside[:, None], h, torch.zeros_like(h)).reshape(-1).contiguous()
    if verify and numel >= kBlockTrailerSize:
        ok, _ = table.verify_blocks(image, safe)
        status = torch.where(inside & (ok == 0), torch.full_like(status, READ_BAD_CHECKSUM), status)
    if numel:
        btype = torch.where(inside, image[torch.where(inside, off + size, zero)].to(torch.int64), zero)
    else:
        btype = zero
    live = status == READ_OK
    status = torch.where(live & (btype != kNoCompression) & (btype != kSnappyCompression),
                         torch.full_like(status, READ_BAD_TYPE), status)
    is_raw = live & (btype == kNoCompression)
    is_comp = live & (btype == kSnappyCompression)
    # the compressed blocks' places, from their preambles
    ulen, pre_ok = _preamble(image, torch.where(is_comp, off, zero), torch.where(is_comp, size, zero)) \
        if numel else (zero, is_comp)
    status = torch.where(is_comp & ~pre_ok, torch.full_like(status, READ_BAD_COMPRESSED), status)
    want = is_comp & pre_ok
    too = want & (ulen > int(max_bytes))
    asked = torch.where(want & ~too, ulen, zero)
    too = too | (want & (torch.cumsum(asked, 0) > int(max_bytes)))
    status = torch.where(too, torch.full_like(status, READ_TOO_LARGE), status)
    want = want & ~too
    # (a preamble the compressed bytes cannot meet gets no place: RawUncompress fails it)
    placed = want & (ulen <= snappy.MAX_EXPANSION * size)
    windows = torch.cat([torch.where(placed, ulen, zero), torch.where(is_raw, size, zero)]).contiguous()
    _, places, end = pack_plan(windows, None, 0, 0)
    csize = torch.where(want, size, zero)
    coff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(csize, 0, out=coff[1:])
    total, ctotal = (int(x) for x in torch.stack([end[0], coff[-1]]).cpu())
    contents = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
    places = places.view(2 * n, 2)
    zeros8 = torch.zeros(n, dtype=torch.uint8, device=dev)
    if ctotal:
        # the compressed bytes side by side (snappy's blocks tile their buffer), then
        # every block through RawUncompress: one that is not compressed has no input
        # and no place, fails at its preamble and writes nothing
        cbuf = torch.empty(ctotal, dtype=torch.uint8, device=dev)
        pack(image, safe, None, None, zeros8, torch.stack([coff[:-1], csize], 1).reshape(-1).contiguous(), cbuf, 0)
        _, len_ok = snappy.uncompressed_length(cbuf, coff)
        out_offsets = torch.cat([places[:n, 0], places[n:n + 1, 0]]).contiguous()
        room = contents if total else torch.empty(1, dtype=torch.uint8, device=dev)
        _, _, ok, _ = snappy.uncompress(cbuf, coff, room, out_offsets)
        status = torch.where(want & ((ok == 0) | (len_ok == 0)), torch.full_like(status, READ_BAD_COMPRESSED),
                             status)
    # the raw blocks
    raw_dst = torch.stack([places[n:, 0], torch.where(is_raw, size, zero)], 1).reshape(-1).contiguous()
    if total:
        pack(image, safe, None, None, zeros8, raw_dst, contents, 0)
    good = status == READ_OK
    out_off = torch.where(is_raw, places[n:, 0], places[:n, 0])
    out_size = torch.where(is_raw, size, ulen)
    out_handles = torch.where(good[:, None], torch.stack([out_off, out_size], 1),
                              torch.zeros_like(h)).reshape(-1).contiguous()
    return contents, out_handles, status.to(torch.int32)


# ---------------------------------------------------------------- many tables in one chain

TABLE_ALIGN = 256         # finish_tables puts every table at a multiple of it
FilterLayout = namedtuple("FilterLayout", "size count filter_first filter_out status")
PlacedTables = namedtuple("PlacedTables", "table_size data_handles tail_handles status")


class TablesResult(namedtuple("TablesResult", "arena table_handles data_handles table_block_first index_handles "
                                              "smallest largest host")):
    """finish_tables' result: every table of the chain in one arena.
    table_handles int64[T, 2] = {base, size} in the arena (bases multiples of
    TABLE_ALIGN, the bytes between tables zero); data_handles int64[2 n_blocks]
    relative to their table, table t's being pairs [table_block_first[t],
    table_block_first[t + 1]); index_handles int64[T, 2]; smallest / largest
    every table's first and last key as bytes (None for a table without
    entries).  host holds the host's copies of the three small tensors."""
    __slots__ = ()

    def table(self, t):
        """Table t's file image: a view of the arena."""
        base, size = (int(x) for x in self.host["table_handles"][t])
        return self.arena[base:base + size]

    def table_data_handles(self, t):
        b0, b1 = (int(x) for x in self.host["table_block_first"][t:t + 2])
        return self.data_handles[2 * b0:2 * b1]

    def index_handle(self, t):
        return tuple(int(x) for x in self.host["index_handles"][t])


def _tw_scratch(n_blocks, n_tables, dev):
    torch = _torch()
    nbytes = int(lib().lsbm_table_write_scratch_bytes(n_blocks, n_tables))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def _n_tables(table_block_first):
    _check(table_block_first=table_block_first)
    if table_block_first.numel() < 1:
        raise ValueError("table_block_first needs n_tables + 1 entries")
    return table_block_first.numel() - 1


@on_stream
def pack_plan_tables(raw_len, comp_len, table_block_first, first_offset=None, gap=kBlockTrailerSize, types=None,
                     handles=None, end=None, status=None, stream=None):
    """pack_plan with the running offset restarting at every table
    (lsbm_table_pack_plan_dev): (types uint8[n], handles int64[2n], end
    int64[T], status int32[T])."""
    torch = _torch()
    _require_cuda(raw_len, comp_len, table_block_first, first_offset, types, handles, end, status)
    _check(raw_len=raw_len, comp_len=comp_len, first_offset=first_offset)
    n, nt, dev = raw_len.numel(), _n_tables(table_block_first), raw_len.device
    for t, name, count in ((comp_len, "comp_len", n), (first_offset, "first_offset", nt)):
        if t is not None and t.numel() != count:
            raise ValueError(f"{name} needs {count} entries")
    types = _buf(n, torch.uint8, dev) if types is None else types
    handles = _buf(2 * n, torch.int64, dev) if handles is None else handles
    end = _buf(nt, torch.int64, dev) if end is None else end
    status = _buf(nt, torch.int32, dev) if status is None else status
    if types.numel() != n or handles.numel() != 2 * n or end.numel() != nt or status.numel() != nt:
        raise ValueError("types[n], handles[2n], end[T] and status[T] are needed")
    scratch = _tw_scratch(n, nt, dev)
    check(lib().lsbm_table_pack_plan_dev(_ptr(raw_len), _ptr(comp_len), n, _ptr(table_block_first), nt,
                                         _ptr(first_offset), int(gap), _ptr(types), _ptr(handles), _ptr(end),
                                         _ptr(status), _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_table_pack_plan_dev")
    return types, handles, end, status


@on_stream
def filter_layout(block_first, table_block_first, data_handles, data_end, bits_per_key, out=None, out_handles=None,
                  filters_cap=0, stream=None):
    """FilterBlockBuilder's layout for every table (lsbm_filter_layout_dev):
    FilterLayout(size int64[T], count int64[T], filter_first, filter_out,
    status int32[T]).  Without `out` only size and count; with it (and
    out_handles, every table's filter-block window, filters_cap the sum of the
    counts) filter_first / filter_out in bloom.build_filters' shape, and every
    table's trailer written into its window."""
    torch = _torch()
    _require_cuda(block_first, table_block_first, data_handles, data_end, out, out_handles)
    _check(block_first=block_first, data_handles=data_handles, data_end=data_end, out=out, out_handles=out_handles)
    n, nt, dev = block_first.numel() - 1, _n_tables(table_block_first), block_first.device
    if n < 0 or data_handles.numel() != 2 * n or data_end.numel() != nt:
        raise ValueError("block_first[n + 1], data_handles[2n] and data_end[T] are needed")
    if (out is None) != (out_handles is None):
        raise ValueError("out and out_handles come together")
    size, count, status = _buf(nt, torch.int64, dev), _buf(nt, torch.int64, dev), _buf(nt, torch.int32, dev)
    first = out_f = None
    if out is not None:
        if out_handles.numel() != 2 * nt:
            raise ValueError("out_handles needs one pair per table")
        first, out_f = _buf(int(filters_cap) + 1, torch.int64, dev), _buf(int(filters_cap), torch.int64, dev)
    scratch = _tw_scratch(n, nt, dev)
    check(lib().lsbm_filter_layout_dev(_ptr(block_first), _ptr(table_block_first), n, nt, _ptr(data_handles),
                                       _ptr(data_end), int(bits_per_key), _ptr(size), _ptr(count), _ptr(first),
                                       _ptr(out_f), int(filters_cap) if out is not None else 0, _ptr(out),
                                       out.numel() if out is not None else 0, _ptr(out_handles), _ptr(status),
                                       _ptr(scratch), scratch.numel() * 8, _stream_ptr(stream)),
          "lsbm_filter_layout_dev")
    return FilterLayout(size, count, first, out_f, status)


@on_stream
def metaindex_blocks(data_end, filter_size=None, out=None, out_handles=None, stream=None):
    """One metaindex block per table (lsbm_metaindex_build_dev): (sizes
    int64[T], status int32[T]); with out / out_handles the bytes too."""
    torch = _torch()
    _require_cuda(data_end, filter_size, out, out_handles)
    _check(data_end=data_end, filter_size=filter_size, out=out, out_handles=out_handles)
    nt, dev = data_end.numel(), data_end.device
    if (filter_size is not None and filter_size.numel() != nt) or (out is None) != (out_handles is None) or \
            (out_handles is not None and out_handles.numel() != 2 * nt):
        raise ValueError("filter_size[T], and out with out_handles[2T], are needed")
    sizes, status = _buf(nt, torch.int64, dev), _buf(nt, torch.int32, dev)
    check(lib().lsbm_metaindex_build_dev(_ptr(data_end), _ptr(filter_size), nt, _ptr(sizes), _ptr(out),
                                         out.numel() if out is not None else 0, _ptr(out_handles), _ptr(status),
                                         _stream_ptr(stream)), "lsbm_metaindex_build_dev")
    return sizes, status


@on_stream
def place_tables(data_handles, table_block_first, tail_handles, tail_per_table, tail_end, table_base, arena,
                 stream=None):
    """Footers and placement (lsbm_table_place_dev): PlacedTables(table_size
    int64[T], data_handles, tail_handles with their table's base added, status
    int32[T]); every table's footer is written into `arena`."""
    torch = _torch()
    _require_cuda(data_handles, table_block_first, tail_handles, tail_end, table_base, arena)
    _check(data_handles=data_handles, tail_handles=tail_handles, tail_end=tail_end, table_base=table_base, arena=arena)
    nt, dev = _n_tables(table_block_first), arena.device
    n, k = data_handles.numel() // 2, int(tail_per_table)
    if data_handles.numel() % 2 or tail_handles.numel() != 2 * k * nt or tail_end.numel() != nt or \
            table_base.numel() != nt:
        raise ValueError("data_handles[2n], tail_handles[2 k T], tail_end[T] and table_base[T] are needed")
    size, status = _buf(nt, torch.int64, dev), _buf(nt, torch.int32, dev)
    abs_d, abs_t = _buf(2 * n, torch.int64, dev), _buf(2 * k * nt, torch.int64, dev)
    scratch = _tw_scratch(n, nt, dev)
    check(lib().lsbm_table_place_dev(_ptr(data_handles), n, _ptr(table_block_first), _ptr(tail_handles), k,
                                     _ptr(tail_end), _ptr(table_base), nt, _ptr(arena), arena.numel(), _ptr(size),
                                     _ptr(abs_d), _ptr(abs_t), _ptr(status), _ptr(scratch), scratch.numel() * 8,
                                     _stream_ptr(stream)), "lsbm_table_place_dev")
    return PlacedTables(size, abs_d, abs_t, status)


def _worst(*statuses):
    """The largest word of some status tensors, as an int64[1] for a read that is due anyway."""
    torch = _torch()
    live = [s.reshape(-1).to(torch.int64) for s in statuses if s is not None and s.numel()]
    return torch.cat(live).max().reshape(1) if live else None


@on_stream
def finish_tables(keys, key_offsets, block_first, table_block_first, blocks, cmp=INTERNAL_KEY, restart_interval=16,
                  bits_per_key=None, compression=kSnappyCompression, stream=None):
    """TableBuilder from the first WriteBlock to the footer for every table of
    a batch at once, over data blocks that are already built (and compressed):
    block b = entries [block_first[b], block_first[b + 1]) of keys /
    key_offsets, table t = blocks [table_block_first[t], table_block_first[t +
    1]) (device tensors; `blocks` a _Blocks over all of them).  The pack plan
    restarts at every table, the filter blocks are laid out and built on the
    device, every metaindex and index block is built in one call each, the tail
    blocks are compressed and ruled together, and one pack and one seal per kind
    put every block of every table into one arena.  Returns a TablesResult.
    The host reads a fixed number of times, whatever the number of tables or
    blocks: the staging sizes, the arena's size, and the results."""
    torch = _torch()
    from . import block_build, bloom, snappy
    if compression not in (kNoCompression, kSnappyCompression):
        raise ValueError("unknown compression type")
    if cmp not in (BYTEWISE, INTERNAL_KEY):
        raise ValueError("unknown comparator")
    _require_cuda(keys, key_offsets, block_first, table_block_first)
    dev = keys.device
    nb, nt = block_first.numel() - 1, _n_tables(table_block_first)
    if nb < 0 or nt < 1:
        raise ValueError("block_first needs n_blocks + 1 entries and table_block_first at least one table")
    snappy_on = compression == kSnappyCompression
    zeros = lambda n: torch.zeros(max(n, 1), dtype=torch.int64, device=dev)[:n]  # noqa: E731
    # 1. WriteBlock's rule over the data blocks, the offsets restarting at every table
    raw_len = blocks.raw_handles.view(-1, 2)[:, 1].contiguous() if nb else zeros(0)
    d_types, d_handles, data_end, st_plan = pack_plan_tables(raw_len, blocks.comp_len if snappy_on and nb else None,
                                                             table_block_first)
    # 2. the sizes of the blocks that follow: [filter,] metaindex, index
    k = 3 if bits_per_key is not None else 2
    fsize = fcount = st_lay = None
    if bits_per_key is not None:
        lay = filter_layout(block_first, table_block_first, d_handles, data_end, int(bits_per_key))
        fsize, fcount, st_lay = lay.size, lay.count, lay.status
    msize, st_meta = metaindex_blocks(data_end, fsize)
    isize, st_index = block_build.index_block(keys, key_offsets, block_first, table_block_first, d_handles, cmp)
    tail_raw_len = torch.stack(([fsize] if k == 3 else []) + [msize, isize], 1).reshape(-1).contiguous() if nt else \
        zeros(0)
    tail_offsets = zeros(k * nt + 1)
    if nt:
        torch.cumsum(tail_raw_len, 0, out=tail_offsets[1:])
    # the first read: the staging image's size and the filters
    head = torch.cat([tail_offsets[-1:], fcount.sum().reshape(1) if k == 3 and nt else zeros(1),
                      _worst(st_plan, st_lay, st_meta, st_index) if nt else zeros(1)]).cpu().tolist()
    tail_total, n_filters, worst = (int(x) for x in head)
    if worst:
        for st, what in ((st_plan, "table pack plan"), (st_lay, "filter layout"), (st_meta, "metaindex block"),
                         (st_index, "index block")):
            if st is not None:
                _raise_on(st, what)
    tail = torch.zeros(max(tail_total, 1), dtype=torch.uint8, device=dev)[:tail_total]
    tail_raw_handles = torch.stack([tail_offsets[:-1], tail_raw_len], 1).contiguous() if nt else zeros(0).view(0, 2)
    window = lambda j: tail_raw_handles.view(nt, k, 2)[:, j].reshape(-1).contiguous()  # noqa: E731
    # 3. the filter blocks: layout and trailers, then every filter of every table in one launch
    st_room = []
    if k == 3 and nt:
        lay = filter_layout(block_first, table_block_first, d_handles, data_end, int(bits_per_key), tail, window(0),
                            n_filters)
        if int(_worst(lay.status).cpu()[0]):  # (a filter without a place must not reach the bloom kernel)
            _raise_on(lay.status, "filter layout")
        if n_filters:
            bloom.build_filters(keys, key_offsets, lay.filter_first, lay.filter_out, tail, int(bits_per_key),
                                strip=8 if cmp == INTERNAL_KEY else 0)
    # 4. the metaindex blocks and 5. the index blocks
    if nt:
        st_room.append(metaindex_blocks(data_end, fsize, tail, window(k - 2))[1])
        st_room.append(block_build.index_block(keys, key_offsets, block_first, table_block_first, d_handles, cmp,
                                               tail, window(k - 1))[1])
    # WriteBlock's rule over them; the filter block is WriteRawBlock(kNoCompression)
    tail_comp = tail_comp_offsets = tail_comp_len = None
    if snappy_on and nt:
        tail_comp, tail_comp_offsets, tail_comp_len = snappy.compress(tail, tail_offsets)
        tail_comp_offsets = tail_comp_offsets[:-1].contiguous()
        tail_comp_len = tail_comp_len.clone()
        if k == 3:
            tail_comp_len.view(nt, k)[:, 0] = COMP_NONE
    tail_first = torch.arange(nt + 1, dtype=torch.int64, device=dev) * k
    t_types, t_handles, tail_end, st_tail = pack_plan_tables(tail_raw_len, tail_comp_len, tail_first, data_end)
    # 6. every table's place in the arena: the second read
    table_size = tail_end + block_build.kFooterEncodedLength
    padded = (table_size + (TABLE_ALIGN - 1)) // TABLE_ALIGN * TABLE_ALIGN
    table_base = zeros(nt + 1)
    if nt:
        torch.cumsum(padded, 0, out=table_base[1:])
    total, worst = (int(x) for x in torch.cat([table_base[-1:], _worst(st_tail, *st_room) if nt else
                                               zeros(1)]).cpu().tolist())
    if worst:
        for st, what in zip([st_tail] + st_room, ("tail pack plan", "metaindex block", "index block")):
            _raise_on(st, what)
    arena = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)[:total]
    table_base = table_base[:-1].contiguous()
    placed = place_tables(d_handles, table_block_first, t_handles, k, tail_end, table_base, arena)
    # 7. everything to its place, every trailer
    st_pack = [placed.status]
    if nb:
        st_pack.append(pack(blocks.raw, blocks.raw_handles, blocks.comp if snappy_on else None,
                            blocks.comp_offsets if snappy_on else None, d_types, placed.data_handles, arena))
    if nt:
        st_pack.append(pack(tail, tail_raw_handles.reshape(-1), tail_comp, tail_comp_offsets, t_types,
                            placed.tail_handles, arena))
        seal_blocks(arena, torch.cat([placed.data_handles, placed.tail_handles]).contiguous(),
                    torch.cat([d_types, t_types]).contiguous())
    # the third read: the results, and where every table's first and last key lie
    table_handles = torch.stack([table_base, table_size], 1) if nt else zeros(0).view(0, 2)
    index_handles = t_handles.view(nt, k, 2)[:, k - 1].contiguous() if nt else zeros(0).view(0, 2)
    e0 = block_first[table_block_first[:-1]]
    e1 = block_first[table_block_first[1:]]
    last = torch.clamp(e1 - 1, min=0)
    key_at = torch.stack([key_offsets[e0], key_offsets[torch.clamp(e0 + 1, max=key_offsets.numel() - 1)],
                          key_offsets[last], key_offsets[e1]], 1) if nt else zeros(0).view(0, 4)
    host = torch.cat([table_handles.reshape(-1), index_handles.reshape(-1), table_block_first, e0, e1,
                      key_at.reshape(-1), _worst(*st_pack) if nt else zeros(1)]).cpu().numpy()
    th, ih = host[:2 * nt].reshape(nt, 2), host[2 * nt:4 * nt].reshape(nt, 2)
    tbf_host = host[4 * nt:5 * nt + 1]
    e0_host, e1_host = host[5 * nt + 1:6 * nt + 1], host[6 * nt + 1:7 * nt + 1]
    ka = host[7 * nt + 1:11 * nt + 1].reshape(nt, 4)
    if int(host[-1]):
        for st, what in zip(st_pack, ("table placement", "pack", "pack")):
            _raise_on(st, what)
    # the fourth read: those keys' bytes, gathered on the device
    smallest, largest = [None] * nt, [None] * nt
    live = [t for t in range(nt) if e1_host[t] > e0_host[t]]
    if live:
        spans = [(int(ka[t][0]), int(ka[t][1])) for t in live] + [(int(ka[t][2]), int(ka[t][3])) for t in live]
        at = np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in spans])
        got = keys[torch.from_numpy(at).to(dev)].cpu().numpy().tobytes()
        pos = 0
        for j, (lo, hi) in enumerate(spans):
            (smallest if j < len(live) else largest)[live[j % len(live)]] = got[pos:pos + hi - lo]
            pos += hi - lo
    return TablesResult(arena, table_handles, d_handles, table_block_first, index_handles, smallest, largest,
                        {"table_handles": th, "index_handles": ih, "table_block_first": tbf_host})


def _build_blocks(keys, key_offsets, values, value_image, p, restart_interval, compression, raise_on):
    """The data blocks of a plan (block_build.plan's result `p`), built side by
    side into a staging image and, under kSnappyCompression, compressed:
    (block_first, _Blocks).  The sizes stay on the device (running sums,
    snappy.compress's own bounds); the host reads the plan once (its status,
    the number of blocks, their bytes) and the build's status once.  raise_on
    (status, what) words a failure."""
    torch = _torch()
    from . import block_build, snappy
    dev = keys.device
    worst, nb, total = (int(x) for x in torch.cat([_worst(p.status) if p.status.numel() else
                                                   torch.zeros(1, dtype=torch.int64, device=dev),
                                                   p.table_block_first[-1:], p.block_bytes.sum().reshape(1)])
                        .cpu().tolist())
    if worst:
        raise_on(p.status, "plan")
    block_first = p.block_first[:nb + 1].contiguous()
    sizes = p.block_bytes[:nb]
    offsets = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    if nb:
        torch.cumsum(sizes, 0, out=offsets[1:])
    raw = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)[:total]
    raw_handles = torch.stack([offsets[:-1], sizes], 1).reshape(-1).contiguous()
    blocks = _Blocks(raw, raw_handles, None, None, None)
    if nb:
        _, st = block_build.build(keys, key_offsets, values, value_image, block_first, raw, raw_handles,
                                  restart_interval)
        if int(_worst(st).cpu()[0]):
            raise_on(st, "build")
        if compression == kSnappyCompression:
            comp, comp_offsets, comp_len = snappy.compress(raw, offsets)
            blocks = _Blocks(raw, raw_handles, comp, comp_offsets[:-1].contiguous(), comp_len.contiguous())
    return block_first, blocks


@on_stream
def write_tables(keys, key_offsets, values, value_image, table_first, cmp=INTERNAL_KEY, block_size=4096,
                 restart_interval=16, bits_per_key=None, compression=kSnappyCompression, stream=None):
    """TableBuilder (table/table_builder.cc) Add for every entry, then Finish,
    for many tables in one chain: table t = entries [table_first[t],
    table_first[t + 1]) (an int64 device tensor or a list; the tables tile the
    entries).  WriteBlock's rule (the snappy form is kept where it is smaller
    than raw - raw / 8) holds on the data blocks, the metaindex block and the
    index block; the filter block is written raw.  The flush rule looks at the
    uncompressed estimate, so the plan is block_build.plan's.  The data blocks
    of all tables are built into a staging image and compressed (_build_blocks),
    then finish_tables lays them out, builds what follows them and moves
    everything into one arena.  A table without entries is the file TableBuilder
    writes when Finish follows no Add.  Returns a TablesResult."""
    torch = _torch()
    from . import block_build
    if compression not in (kNoCompression, kSnappyCompression):
        raise ValueError("unknown compression type")
    if cmp not in (BYTEWISE, INTERNAL_KEY):
        raise ValueError("unknown comparator")
    _require_cuda(keys, key_offsets, values, value_image)
    dev = keys.device
    n = key_offsets.numel() - 1
    if n < 0 or values.numel() != 2 * n:
        raise ValueError("values must be one {offset, length} pair per entry")
    values = values.reshape(-1)
    if not hasattr(table_first, "is_cuda"):
        table_first = torch.tensor([int(x) for x in table_first], dtype=torch.int64, device=dev)
    _require_cuda(table_first)
    p = block_build.plan(keys, key_offsets, values, table_first, block_size, restart_interval)
    block_first, blocks = _build_blocks(keys, key_offsets, values, value_image, p, restart_interval, compression,
                                        block_build._raise_on)
    return finish_tables(keys, key_offsets, block_first, p.table_block_first, blocks, cmp, restart_interval,
                         bits_per_key, compression)


@on_stream
def write_table(keys, key_offsets, values, value_image, cmp=INTERNAL_KEY, block_size=4096, restart_interval=16,
                bits_per_key=None, compression=kSnappyCompression, stream=None):
    """write_tables of one table: (file_image uint8 device tensor, data_handles
    int64 device tensor of {offset, size} pairs, index_handle (offset, size)).
    The image is a view of write_tables' arena, contiguous and of the file's
    size.  Every failure is write_tables': a plan or a build that fails raises
    in block_build's words ("plan: block would reach 2^32 bytes")."""
    _require_cuda(key_offsets)
    res = write_tables(keys, key_offsets, values, value_image, [0, key_offsets.numel() - 1], cmp, block_size,
                       restart_interval, bits_per_key, compression, stream)
    return res.table(0), res.table_data_handles(0), res.index_handle(0)


# ---------------------------------------------------------------- Get


def _get_state_of(read_status):
    """read_blocks' status -> table_get's state (int64 tensors)."""
    torch = _torch()
    out = torch.full_like(read_status, SEEK_VALID)
    for r, g in ((READ_TRUNCATED, SEEK_BAD_HANDLE), (READ_BAD_CHECKSUM, GET_BAD_CHECKSUM),
                 (READ_BAD_COMPRESSED, GET_BAD_COMPRESSED), (READ_BAD_TYPE, GET_BAD_TYPE),
                 (READ_TOO_LARGE, GET_BAD_COMPRESSED)):
        out = torch.where(read_status == r, torch.full_like(out, g), out)
    return out


@on_stream
def table_get(image, index_handle, keys, key_offsets, filter=None, verify=True,  # noqa: A002
              cmp=INTERNAL_KEY, bits_per_key=10, bloom_bits_use=15, max_bytes=1 << 30, stream=None):
    """Table::InternalGet (table/table.cc:309-339) for a batch of keys over a
    device-resident table image whose blocks are of either type.  The index
    block goes through read_blocks, the queries are seeked in it, the distinct
    data blocks they hit go through read_blocks once each (one host read of
    their count, one of the contents' size), and the data-block Seek runs over
    the contents.

    Returns GetResult(state, key_len, value, data_handle, value_image) as
    block.table_get does, with two differences: value {offset, length} points
    into value_image (the uncompressed contents, not the file image), and a
    block that does not uncompress is GET_BAD_COMPRESSED; GET_NEEDS_UNCOMPRESS
    never appears.  An index block that cannot be read gives every query its
    state."""
    torch = _torch()
    from . import block, bloom
    _require_cuda(image, keys, key_offsets, filter)
    _check(image=image, keys=keys, key_offsets=key_offsets, filter=filter)
    n = key_offsets.numel() - 1
    dev = image.device
    ih = torch.tensor([int(index_handle[0]), int(index_handle[1])], dtype=torch.int64, device=dev)
    # 1. the index block's contents; iiter->Seek(k) and BlockHandle::DecodeFrom(iiter->value())
    icontents, ihandle, istatus = read_blocks(image, ih, verify, max_bytes)
    if icontents.numel() == 0:
        icontents = torch.zeros(1, dtype=torch.uint8, device=dev)
    idx = block.seek(icontents, ihandle.repeat(n), keys, key_offsets, cmp=cmp, value_is_handle=True)
    index_state = _get_state_of(istatus.to(torch.int64))[0].to(torch.int32)
    state = torch.where(index_state != SEEK_VALID, index_state.expand(n), idx.state).contiguous()
    found = state == SEEK_VALID
    handle = torch.where(found[:, None], idx.handle, torch.zeros_like(idx.handle))
    if filter is not None:  # 2. filter->KeyMayMatch(handle.offset(), k)
        fh = torch.tensor([0, filter.numel()], dtype=torch.int64, device=dev).repeat(n)
        may, _ = bloom.filter_block_may_match(filter, fh, handle[:, 0].contiguous(), keys, key_offsets,
                                              bits_per_key, bloom_bits_use,
                                              strip=8 if cmp == INTERNAL_KEY else 0)
        state = torch.where(found & (may == 0), torch.full_like(state, GET_FILTERED), state)
    live = state == SEEK_VALID
    # 3. ReadBlock of the distinct data blocks (a query that ended above asks for no block)
    asked = torch.where(live[:, None], handle, torch.full_like(handle, -1))
    blocks, which = torch.unique(asked, dim=0, return_inverse=True)
    contents, out_handles, bstatus = read_blocks(image, blocks.reshape(-1).contiguous(), verify, max_bytes)
    if contents.numel() == 0:
        contents = torch.zeros(1, dtype=torch.uint8, device=dev)[:0]
    bstate = _get_state_of(bstatus.to(torch.int64))[which].to(torch.int32)
    state = torch.where(live, bstate, state)
    live = state == SEEK_VALID
    # 4. block_iter->Seek(k) over the contents
    dh = torch.where(live[:, None], out_handles.view(-1, 2)[which], torch.zeros_like(handle))
    seek_image = contents if contents.numel() else torch.zeros(1, dtype=torch.uint8, device=dev)
    dat = block.seek(seek_image, dh.reshape(-1).contiguous(), keys, key_offsets, cmp=cmp)
    state = torch.where(live, dat.state, state)
    hit = state == SEEK_VALID
    key_len = torch.where(hit, dat.key_len, torch.zeros_like(dat.key_len))
    value = torch.where(hit[:, None], dat.value, torch.zeros_like(dat.value))
    return GetResult(state, key_len, value, handle, contents)


# ---------------------------------------------------------------- compaction


def _in_place(image, handles, verify=None):
    """read_blocks' shape for blocks taken as they lie in the image, which is how
    merge.compact reads its kNoCompression inputs: no ReadBlock, no status."""
    return image, handles, None


def _get_varint64(buf, p):
    v, shift = 0, 0
    while True:
        b = buf[p]
        p += 1
        v |= (b & 127) << shift
        if b < 128:
            return v, p
        shift += 7


def _index_data_handles(image, index_handle, verify, read):
    """BlockHandle::DecodeFrom of every value of an index block whose contents
    `read` (read_blocks or _in_place) gives: int64 numpy {offset, size} pairs."""
    torch = _torch()
    from . import block
    ih = torch.tensor([int(index_handle[0]), int(index_handle[1])], dtype=torch.int64, device=image.device)
    contents, oh, st = read(image, ih, verify)
    if st is not None and int(st.cpu()[0]) != READ_OK:
        raise ValueError("index block: " + READ_MESSAGE[int(st.cpu()[0])])
    _, _, values, _, dst = block.decode(contents, oh)
    if int(dst.cpu()[0]) != block.BLOCK_OK:
        raise ValueError("index block: " + block.STATUS_MESSAGE.get(int(dst.cpu()[0]), "bad"))
    lo, size = oh.cpu().tolist()
    buf = contents[lo:lo + size].cpu().numpy().tobytes()
    out = []
    for off, _ in values.cpu().tolist():
        o, p = _get_varint64(buf, off - lo)
        out += [o, _get_varint64(buf, p)[0]]
    return np.array(out, dtype=np.int64)


def index_data_handles(image, index_handle, verify=True):
    """The data block handles an index block of either type lists, as an int64
    numpy array of {offset, size} pairs."""
    return _index_data_handles(image, index_handle, verify, read_blocks)


def _compact(read, images, data_handles, max_file_size, index_handles, cmp, drop, smallest_snapshot, bottom_level,
             block_size, restart_interval, bits_per_key, compression, verify):
    """The one body of merge.compact (read = _in_place) and compact (read =
    read_blocks), on torch's current stream."""
    torch = _torch()
    from . import block, block_build, merge
    if (data_handles is None) == (index_handles is None):
        raise ValueError("give data_handles or index_handles")
    if compression not in (kNoCompression, kSnappyCompression):
        raise ValueError("unknown compression type")
    if len(images) > merge.MAX_RUNS:
        raise ValueError(f"at most {merge.MAX_RUNS} input tables")
    if int(max_file_size) < 1:
        raise ValueError("max_file_size must be at least 1")
    _require_cuda(*images)
    if not images:
        return []
    dev = images[0].device
    if data_handles is None:
        data_handles = [_index_data_handles(img, ih, verify, read) for img, ih in zip(images, index_handles)]
    if len(data_handles) != len(images):
        raise ValueError("one set of handles per image")
    # 1. one file image; every handle moves by its image's place in it
    image = torch.cat([img.reshape(-1) for img in images])
    handles, blocks_before, base = [], [0], 0
    for img, h in zip(images, data_handles):
        h = torch.as_tensor(np.asarray(h.cpu() if hasattr(h, "cpu") else h, dtype=np.int64).reshape(-1, 2).copy())
        h[:, 0] += base
        handles.append(h)
        blocks_before.append(blocks_before[-1] + h.shape[0])
        base += img.numel()
    handles = torch.cat(handles).reshape(-1).contiguous().to(dev)
    # 2. every data block's contents (the value image from here on); the entries, one run per input table
    contents, handles, st = read(image, handles, verify)
    if st is not None:
        bad = [(b, int(s)) for b, s in enumerate(st.cpu().tolist()) if s != READ_OK]
        if bad:
            raise ValueError(f"input data block {bad[0][0]}: {READ_MESSAGE[bad[0][1]]}")
        if contents.numel() == 0:
            return []
    counts, st = block.scan(contents, handles)
    _raise_on(st, "scan")
    nb = counts.shape[0]
    entry_base = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    key_base = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    if nb:
        torch.cumsum(counts[:, 0], 0, out=entry_base[1:])
        torch.cumsum(counts[:, 1], 0, out=key_base[1:])
    keys, key_offsets, values, _, st = block.decode(contents, handles, entry_base, key_base)
    _raise_on(st, "decode")
    run_first = entry_base[torch.tensor(blocks_before, dtype=torch.int64, device=dev)].contiguous()
    # 3. the merge and the single-table plan of its output
    m = merge.merge(keys, key_offsets, values, run_first, cmp, drop, smallest_snapshot, bottom_level)
    bad = [(r, int(s)) for r, s in enumerate(m.run_status.cpu().tolist()) if s != merge.MERGE_OK]
    if bad:
        raise ValueError(f"input table {bad[0][0]}: {merge.STATUS_MESSAGE.get(bad[0][1], bad[0][1])}")
    n_out = m.key_offsets.numel() - 1
    if n_out == 0:
        return []
    m_values = m.values.reshape(-1).contiguous()
    p = block_build.plan(m.keys, m.key_offsets, m_values, torch.tensor([0, n_out], dtype=torch.int64, device=dev),
                         block_size, restart_interval)
    # 4. every data block once: built, compressed, ruled; the cut over the packed sizes (one read)
    block_first, blocks = _build_blocks(m.keys, m.key_offsets, m_values, contents, p, restart_interval, compression,
                                        _raise_on)
    n_blocks = block_first.numel() - 1
    _, packed, _ = pack_plan(blocks.raw_handles.view(-1, 2)[:, 1].contiguous(), blocks.comp_len)
    host = torch.cat([block_first, packed.view(-1, 2)[:, 1]]).cpu().tolist()
    table_first, table_block_first = merge.cut_tables(host[:n_blocks + 1], host[n_blocks + 1:], int(max_file_size))
    # 5. every output table in one chain
    res = finish_tables(m.keys, m.key_offsets, block_first,
                        torch.tensor(table_block_first, dtype=torch.int64, device=dev), blocks, cmp, restart_interval,
                        bits_per_key, compression)
    return [OutputTable(res.table(t), res.table_data_handles(t), res.index_handle(t))
            for t in range(len(table_first) - 1)]


@on_stream
def compact(images, data_handles=None, max_file_size=2 << 20, index_handles=None, cmp=INTERNAL_KEY, drop=False,
            smallest_snapshot=None, bottom_level=False, block_size=4096, restart_interval=16, bits_per_key=None,
            compression=kNoCompression, verify=True, stream=None):
    """merge.compact for tables whose blocks are of either type, with output
    tables written under `compression`.  Every input data block goes through
    read_blocks, whose contents are the value image that decode, merge and the
    builder point into.  The merged entries are planned as one table; every
    data block of that plan is built and compressed once; the cut
    (merge.cut_tables) sees each block's packed size, as FileSize() does; and
    finish_tables finishes every output table from its slice of those blocks in
    one chain.  Returns [OutputTable(image, data_handles, index_handle)]; the
    images are views of one arena, so holding one keeps the whole arena alive."""
    return _compact(read_blocks, images, data_handles, max_file_size, index_handles, cmp, drop, smallest_snapshot,
                    bottom_level, block_size, restart_interval, bits_per_key, compression, verify)
