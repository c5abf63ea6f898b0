"""Plain-Python restatement of lsbm's table/ layer for tables whose blocks may
be snappy-compressed: TableBuilder::WriteBlock's keep rule
(table/table_builder.cc:176-206) and Finish over buildmodel's blocks,
Footer::DecodeFrom, ReadBlock (table/format.cc:66-148) and the block walk, and
the compaction of mergemodel with the cut taken over packed sizes -- the model
the GPU table packer (include/lsbm_table_pack.h, lsbm_amd/sstable.py) is
compared with.  The codec is passed in (`compress` / `uncompress` callables),
so the model itself holds no snappy; tests/test_sstable.py pins it to the files
of tests/golden/snappy_tables.json, which libsnappy produced.

Statuses are those of include/lsbm_table_pack.h.
"""
import struct

from golden import blockmodel as bm
from golden import buildmodel as bd
from golden import mergemodel as mm
from golden.blockmodel import INTERNAL_KEY

READ_OK, READ_TRUNCATED, READ_BAD_CHECKSUM, READ_BAD_COMPRESSED, READ_BAD_TYPE, READ_TOO_LARGE = range(6)
NO_COMPRESSION, SNAPPY = 0, 1
U64 = (1 << 64) - 1
TRAILER = 5


def keep_compressed(raw_len, comp_len):
    """compressed.size() < raw.size() - raw.size() / 8 in size_t arithmetic;
    comp_len U64: the block could not be compressed."""
    return comp_len != U64 and comp_len < ((raw_len - raw_len // 8) & U64)


def pack_plan(raw_len, comp_len, first_offset=0, gap=TRAILER):
    """([type], [(offset, size)], end) of blocks written back to back."""
    types, handles, at = [], [], first_offset
    for i, raw in enumerate(raw_len):
        comp = U64 if comp_len is None else comp_len[i]
        t = 1 if keep_compressed(raw, comp) else 0
        size = comp if t else raw
        types.append(t)
        handles.append((at, size))
        at = (at + size + gap) & U64
    return types, handles, at


def write_block(out, raw, compress):
    """WriteBlock + WriteRawBlock: (handle, type)."""
    typ, contents = NO_COMPRESSION, raw
    if compress is not None:
        c = compress(raw)
        if c is not None and keep_compressed(len(raw), len(c)):
            typ, contents = SNAPPY, c
    h = (len(out), len(contents))
    out.extend(contents + bd.trailer(contents, typ))
    return h, typ


def finish_table(entries, first, blocks, cmp, restart_interval, bits_per_key, compress):
    """TableBuilder over built data blocks (block b = entries[first[b]:first[b+1]]):
    (file bytes, [(offset, size)] of the data blocks, index handle, [type of every
    block in file order])."""
    keys = [k for k, _ in entries]
    out, handles, types = bytearray(), [], []
    for block in blocks:
        h, t = write_block(out, block, compress)
        handles.append(h)
        types.append(t)
    meta = []
    if bits_per_key is not None:
        fkeys = [k[:-8] for k in keys] if cmp == INTERNAL_KEY else keys
        fb = bd.filter_block(fkeys, first, [h[0] for h in handles], len(out), bits_per_key)
        fh, t = write_block(out, fb, None)  # WriteRawBlock(kNoCompression)
        types.append(t)
        meta.append((bd.FILTER_KEY, bd.encode_handle(*fh)))
    meta_handle, t = write_block(out, bm.build_block(meta, restart_interval), compress)
    types.append(t)
    index_handle, t = write_block(out, bd.index_block(keys, first, handles, cmp), compress)
    types.append(t)
    out.extend(bd.footer(meta_handle, index_handle))
    return bytes(out), handles, index_handle, types


def data_blocks(entries, block_size, restart_interval):
    first, sizes = bd.plan([(k, len(v)) for k, v in entries], block_size, restart_interval)
    blocks = [bm.build_block(entries[first[b]:first[b + 1]], restart_interval) for b in range(len(sizes))]
    assert [len(b) for b in blocks] == sizes
    return first, blocks


def table_file(entries, cmp=INTERNAL_KEY, block_size=4096, restart_interval=16, bits_per_key=None, compress=None):
    """TableBuilder: Add for every (key, value), Finish, with options.compression
    = kSnappyCompression when `compress` (bytes -> bytes, or None where
    Snappy_Compress returns false) is given.  Returns (file bytes, data block
    handles, index handle, block types in file order)."""
    first, blocks = data_blocks(entries, block_size, restart_interval)
    return finish_table(entries, first, blocks, cmp, restart_interval, bits_per_key, compress)


def unmask(m):
    rot = (m - 0xA282EAD8) & 0xFFFFFFFF
    return ((rot >> 17) | (rot << 15)) & 0xFFFFFFFF


def read_block(data, handle, uncompress, verify=True, max_bytes=1 << 30):
    """ReadBlock: (status, contents, type byte)."""
    off, size = handle
    if off < 0 or size < 0 or off + size + TRAILER > len(data):
        return READ_TRUNCATED, b"", None
    body = data[off:off + size]
    typ = data[off + size]
    if verify:
        crc = unmask(struct.unpack_from("<I", data, off + size + 1)[0])
        if crc != bd.crc32c(bytes([typ]), bd.crc32c(body)):
            return READ_BAD_CHECKSUM, b"", typ
    if typ == NO_COMPRESSION:
        return READ_OK, bytes(body), typ
    if typ == SNAPPY:
        pre = bm.get_varint32(body, 0, len(body))  # GetUncompressedLength
        if pre is not None and pre[0] > max_bytes:
            return READ_TOO_LARGE, b"", typ
        out = uncompress(bytes(body))
        return (READ_OK, out, typ) if out is not None else (READ_BAD_COMPRESSED, b"", typ)
    return READ_BAD_TYPE, b"", typ


def decode_footer(data):
    """Footer::DecodeFrom: (metaindex handle, index handle)."""
    foot = data[-48:]
    assert struct.unpack("<Q", foot[40:])[0] == bd.MAGIC
    a = bm.get_varint64(foot, 0, 40)
    b = bm.get_varint64(foot, a[1], 40)
    c = bm.get_varint64(foot, b[1], 40)
    d = bm.get_varint64(foot, c[1], 40)
    return (a[0], b[0]), (c[0], d[0])


def block_entries(contents):
    st, walked = bm.walk(contents)
    assert st == bm.OK
    return [(k, bytes(contents[vo:vo + vl])) for k, vo, vl, _ in walked]


def read_table(data, uncompress):
    """Table::Open and a full iteration.  Returns a dict: entries [(key,
    value)], data_handles, index_handle, types (every block's type byte in
    file order: data blocks, [filter], metaindex, index), meta_handle,
    filter_handle and filter (the filter block's handle and bytes, or None),
    blocks (each data block's contents) and index (the index block's)."""
    meta_handle, index_handle = decode_footer(data)

    def read(h):
        st, contents, typ = read_block(data, h, uncompress)
        assert st == READ_OK, (h, st)
        return contents, typ

    index, index_type = read(index_handle)
    meta, meta_type = read(meta_handle)
    handles = [bm.decode_handle(v) for _, v in block_entries(index)]
    entries, types, blocks = [], [], []
    for h in handles:
        contents, typ = read(h)
        blocks.append(contents)
        types.append(typ)
        entries += block_entries(contents)
    filt = filter_handle = None
    for k, v in block_entries(meta):
        if k == bd.FILTER_KEY:
            filter_handle = bm.decode_handle(v)
            filt, typ = read(filter_handle)
            types.append(typ)
    return {"entries": entries, "data_handles": handles, "index_handle": index_handle, "meta_handle": meta_handle,
            "filter_handle": filter_handle, "types": types + [meta_type, index_type], "filter": filt,
            "blocks": blocks, "index": index}


def compact(runs, cmp, max_file_size, drop=False, smallest_snapshot=0, bottom_level=False, block_size=4096,
            restart_interval=16, bits_per_key=None, compress=None):
    """mergemodel's merge and drop, buildmodel.plan over the output, the cut over
    the blocks' packed sizes (FileSize() grows by what WriteRawBlock appended),
    table_file per table: [file bytes]."""
    entries, _ = mm.merge_entries(runs, cmp, drop, smallest_snapshot, bottom_level)
    first, blocks = data_blocks(entries, block_size, restart_interval)
    comp_len = None if compress is None else [U64 if c is None else len(c) for c in map(compress, blocks)]
    _, handles, _ = pack_plan([len(b) for b in blocks], comp_len)
    table_first, _ = mm.cut_tables(first, [s for _, s in handles], max_file_size)
    return [table_file(entries[table_first[t]:table_first[t + 1]], cmp, block_size, restart_interval, bits_per_key,
                       compress)[0] for t in range(len(table_first) - 1)]
