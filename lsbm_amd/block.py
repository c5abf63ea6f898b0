"""SSTable block reader (Block::Iter of lsbm's table/block.cc) on the GPU.

Thin wrappers over include/lsbm_block.h.  Device tensors in, device tensors
out; every call runs on `stream` (default: torch's current stream; the contract is engine.py's).

    scan(image, handles)              SeekToFirst / Next until !Valid of every
                                      block: entry count, key bytes, value
                                      bytes, status (table/block.cc:288-315)
    decode(image, handles, ...)       the same walk written out: keys +
                                      key_offsets (the pair bloom.build_filters
                                      reads) and value {offset, length} slices
    seek(image, handles, keys, ...)   Block::Iter::Seek for many lookups
                                      (table/block.cc:223-265)
    table_get(image, index_handle, keys, key_offsets, ...)
                                      Table::InternalGet for a batch of keys
                                      (table/table.cc:309-339)

A block is image[handles[2i], handles[2i] + handles[2i+1]) (int64 {offset,
size} pairs, the block contents without the 5-byte trailer).  Keys are a uint8
buffer plus int64 offsets (key i = keys[off[i], off[i+1])).
"""
from collections import namedtuple

from ._lib import check, lib
from .engine import _check_tensors, _ptr, _require_cuda, _stream_ptr, _torch, on_stream
from .table import kNoCompression, kSnappyCompression

# comparators (include/lsbm_block.h)
BYTEWISE = 0
INTERNAL_KEY = 1
SEEK_VALUE_IS_HANDLE = 0x1

# scan / decode status per block
BLOCK_OK = 0
BLOCK_BAD_CONTENTS = 1   # Corruption("bad block contents")
BLOCK_BAD_ENTRY = 2      # Corruption("bad entry in block")
BLOCK_NO_ROOM = 3        # decode: window too small

# seek / table_get state per query
SEEK_VALID = 0
SEEK_NOT_VALID = 1       # !Valid(), status OK
SEEK_BAD_ENTRY = 2
SEEK_BAD_CONTENTS = 3
SEEK_BAD_HANDLE = 4      # Corruption("bad block handle")
# table_get only
GET_NEEDS_UNCOMPRESS = 5  # the data block is compressed (chain snappy.uncompress)
GET_FILTERED = 6          # the filter says the key is not in the block
GET_BAD_CHECKSUM = 7      # Corruption("block checksum mismatch")
GET_BAD_TYPE = 8          # Corruption("bad block type")

STATUS_MESSAGE = {BLOCK_BAD_CONTENTS: "bad block contents", BLOCK_BAD_ENTRY: "bad entry in block"}
STATE_MESSAGE = {SEEK_BAD_ENTRY: "bad entry in block", SEEK_BAD_CONTENTS: "bad block contents",
                 SEEK_BAD_HANDLE: "bad block handle", GET_BAD_CHECKSUM: "block checksum mismatch",
                 GET_BAD_TYPE: "bad block type"}

SeekResult = namedtuple("SeekResult", "state pos key_len value handle found found_offsets")
GetResult = namedtuple("GetResult", "state key_len value data_handle")


def _check(**ts):
    _check_tensors(ts, u8=("image", "keys", "found"), i32=("status", "state"))


def _n_handles(handles):
    if handles.numel() % 2:
        raise ValueError("handles must be {offset, size} pairs")
    return handles.numel() // 2


@on_stream
def scan(image, handles, stream=None):
    """(counts int64[n, 3] = {entries, key bytes, value bytes}, status int32[n])."""
    torch = _torch()
    _require_cuda(image, handles)
    _check(image=image, handles=handles)
    n = _n_handles(handles)
    counts = torch.zeros((n, 3), dtype=torch.int64, device=image.device)
    status = torch.zeros(n, dtype=torch.int32, device=image.device)
    check(lib().lsbm_block_scan_dev(_ptr(image), image.numel(), _ptr(handles), n, _ptr(counts),
                                    _ptr(status), _stream_ptr(stream)), "lsbm_block_scan_dev")
    return counts, status


@on_stream
def decode(image, handles, entry_base=None, key_base=None, keys=None, key_offsets=None,
           values=None, stream=None):
    """Returns (keys, key_offsets, values int64[entries, 2], entry_base, status).
    Block i's entries are [entry_base[i], entry_base[i+1]).  Without entry_base /
    key_base the windows are the running sums of a scan's counts (one device ->
    host read of the totals, to size the outputs)."""
    torch = _torch()
    _require_cuda(image, handles, entry_base, key_base, keys, key_offsets, values)
    _check(image=image, handles=handles, entry_base=entry_base, key_base=key_base, keys=keys,
           key_offsets=key_offsets, values=values)
    n = _n_handles(handles)
    dev = image.device
    if (entry_base is None) != (key_base is None):
        raise ValueError("entry_base and key_base come together")
    if entry_base is None:
        counts, _ = scan(image, handles, stream)
        entry_base = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        key_base = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            torch.cumsum(counts[:, 0], 0, out=entry_base[1:])
            torch.cumsum(counts[:, 1], 0, out=key_base[1:])
    if entry_base.numel() != n + 1 or key_base.numel() != n + 1:
        raise ValueError("entry_base and key_base need n + 1 entries")
    if key_offsets is None or values is None or keys is None:
        totals = torch.stack([entry_base[-1], key_base[-1]]).cpu()
        ne, nk = int(totals[0]), int(totals[1])
        if key_offsets is None:
            key_offsets = torch.zeros(ne + 1, dtype=torch.int64, device=dev)
        if values is None:
            values = torch.zeros((ne, 2), dtype=torch.int64, device=dev)
        if keys is None:
            keys = torch.zeros(max(nk, 1), dtype=torch.uint8, device=dev)[:nk]
    entries_cap = min(key_offsets.numel() - 1, values.numel() // 2)
    if entries_cap < 0:
        raise ValueError("key_offsets needs at least one entry")
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    check(lib().lsbm_block_decode_dev(_ptr(image), image.numel(), _ptr(handles), n, _ptr(entry_base),
                                      _ptr(key_base), _ptr(keys), keys.numel(), _ptr(key_offsets),
                                      _ptr(values), entries_cap, None, _ptr(status),
                                      _stream_ptr(stream)), "lsbm_block_decode_dev")
    return keys, key_offsets, values, entry_base, status


@on_stream
def seek(image, handles, keys, key_offsets, cmp=BYTEWISE, value_is_handle=False, found=None,
         found_offsets=None, stream=None):
    """Seek(key q) in block q.  Returns SeekResult(state int32[n], pos, key_len
    int64[n], value int64[n, 2], handle int64[n, 2] or None, found,
    found_offsets).  found / found_offsets: optional windows for the found keys
    (window q = found[found_offsets[q], found_offsets[q+1]))."""
    torch = _torch()
    _require_cuda(image, handles, keys, key_offsets, found, found_offsets)
    _check(image=image, handles=handles, keys=keys, key_offsets=key_offsets, found=found,
           found_offsets=found_offsets)
    n = _n_handles(handles)
    if key_offsets.numel() != n + 1:
        raise ValueError("key_offsets needs one key per handle pair (n + 1 entries)")
    if (found is None) != (found_offsets is None):
        raise ValueError("found and found_offsets come together")
    if found_offsets is not None and found_offsets.numel() != n + 1:
        raise ValueError("found_offsets needs n + 1 entries")
    dev = image.device
    state = torch.zeros(n, dtype=torch.int32, device=dev)
    pos = torch.zeros(n, dtype=torch.int64, device=dev)
    key_len = torch.zeros(n, dtype=torch.int64, device=dev)
    value = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    handle = torch.zeros((n, 2), dtype=torch.int64, device=dev) if value_is_handle else None
    check(lib().lsbm_block_seek_dev(_ptr(image), image.numel(), _ptr(handles), _ptr(keys),
                                    _ptr(key_offsets), n, int(cmp),
                                    SEEK_VALUE_IS_HANDLE if value_is_handle else 0, _ptr(state),
                                    _ptr(pos), _ptr(key_len), _ptr(value), _ptr(handle), _ptr(found),
                                    _ptr(found_offsets), found.numel() if found is not None else 0,
                                    _stream_ptr(stream)), "lsbm_block_seek_dev")
    return SeekResult(state, pos, key_len, value, handle, found, found_offsets)


@on_stream
def table_get(image, index_handle, keys, key_offsets, filter=None, verify=True,  # noqa: A002
              cmp=INTERNAL_KEY, bits_per_key=10, bloom_bits_use=15, stream=None):
    """Table::InternalGet (table/table.cc:309-339) for a batch of keys over a
    device-resident table image: index-block Seek with BlockHandle decode, the
    filter probe (filter: the table's filter block as a uint8 device tensor,
    read with BloomFilterPolicy(bits_per_key)), ReadBlock's trailer check
    (verify) and the data-block Seek -- device calls on one stream with no host
    synchronisation between them.  index_handle: the index block's (offset,
    size) in the image.

    Returns GetResult(state int32[n], key_len int64[n], value int64[n, 2],
    data_handle int64[n, 2]): state SEEK_VALID with the found entry's key length
    and value {offset, length}; SEEK_NOT_VALID when the index or the data block
    has no entry at or after the key; SEEK_BAD_* from either Seek;
    GET_FILTERED; GET_BAD_CHECKSUM; GET_BAD_TYPE; GET_NEEDS_UNCOMPRESS for a
    block that is not kNoCompression (sstable.table_get reads tables of either
    block type).  As in the reference the caller compares the found key's user
    key with its own (SaveValue)."""
    torch = _torch()
    from . import bloom, table
    _require_cuda(image, keys, key_offsets, filter)
    _check(image=image, keys=keys, key_offsets=key_offsets)
    n = key_offsets.numel() - 1
    dev = image.device
    ih = torch.tensor([int(index_handle[0]), int(index_handle[1])], dtype=torch.int64, device=dev)
    # 1. iiter->Seek(k) and BlockHandle::DecodeFrom(iiter->value())
    idx = seek(image, ih.repeat(n), keys, key_offsets, cmp=cmp, value_is_handle=True, stream=stream)
    state = idx.state.clone()
    found = state == SEEK_VALID
    handle = torch.where(found[:, None], idx.handle, torch.zeros_like(idx.handle))
    if filter is not None:  # 2. filter->KeyMayMatch(handle.offset(), k)
        _check(image=filter)
        fh = torch.tensor([0, filter.numel()], dtype=torch.int64, device=dev).repeat(n)
        may, _ = bloom.filter_block_may_match(filter, fh, handle[:, 0].contiguous(), keys, key_offsets,
                                              bits_per_key, bloom_bits_use,
                                              strip=8 if cmp == INTERNAL_KEY else 0, stream=stream)
        state = torch.where(found & (may == 0), torch.full_like(state, GET_FILTERED), state)
    flat = handle.reshape(-1).contiguous()
    # the block's trailer: type byte at image[off + size] (table/format.cc:104)
    tpos = handle[:, 0] + handle[:, 1]
    inside = (handle[:, 0] >= 0) & (handle[:, 1] >= 0) & (tpos >= 0) & (tpos < image.numel())
    if image.numel():
        at = torch.where(inside, tpos, torch.zeros_like(tpos))
        btype = torch.where(inside, image[at].to(torch.int32), torch.zeros_like(state))
    else:
        btype = torch.zeros_like(state)
    live = state == SEEK_VALID
    if verify:  # 3. ReadBlock's checksum (a block past the image is not ok: the Seek reports it)
        ok, _ = table.verify_blocks(image, flat, stream=stream)
        state = torch.where(live & inside & (ok == 0), torch.full_like(state, GET_BAD_CHECKSUM), state)
        live = state == SEEK_VALID
    other = (btype != kNoCompression) & (btype != kSnappyCompression)
    state = torch.where(live & inside & (btype == kSnappyCompression),
                        torch.full_like(state, GET_NEEDS_UNCOMPRESS), state)
    state = torch.where(live & inside & other, torch.full_like(state, GET_BAD_TYPE), state)
    live = state == SEEK_VALID
    # 4. block_iter->Seek(k): queries that ended above seek an empty handle and are masked out
    dh = torch.where(live[:, None], handle, torch.zeros_like(handle)).reshape(-1).contiguous()
    dat = seek(image, dh, keys, key_offsets, cmp=cmp, stream=stream)
    state = torch.where(live, dat.state, state)
    hit = state == SEEK_VALID
    key_len = torch.where(hit, dat.key_len, torch.zeros_like(dat.key_len))
    value = torch.where(hit[:, None], dat.value, torch.zeros_like(dat.value))
    return GetResult(state, key_len, value, handle)
