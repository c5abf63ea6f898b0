"""Models of include/lsbm_table_write.h for tests/test_table_write*.py.

filter_layout is FilterBlockBuilder (table/filter_block.cc:22-76) in closed
form, as the device lays it out: with fi(b) = start(b) >> 11, the blocks that
share one fi form one filter, which takes slot fi of the offset array; the
slots between two filters repeat the running size; the array has
fi(end) + (fi(end) == fi(last block)) slots.  No loop over StartBlock calls:
lsbm_amd.bloom.layout_filter_block is that loop, and tests/test_table_write.py
holds the two against each other.

LAYOUT_CASES are the block-size sequences both tests use; starts follow from
the sizes (size + 5 a block), so "one byte either side of 2,048" is a size
that is one byte smaller or larger.
"""
import numpy as np

BASE_LG = 11
TRAILER = 5  # kBlockTrailerSize


def filter_bytes(n_keys, bits_per_key):
    """util/bloom.cc:39-50: the bit array (at least 64 bits) and the k byte."""
    return (np.maximum(np.asarray(n_keys, dtype=np.int64) * bits_per_key, 64) + 7) // 8 + 1


def filter_layout(block_start, block_first, data_end, bits_per_key):
    """block_start[nb], block_first[nb + 1], data_end -> dict(filter_first
    [(k0, k1)], filter_out, offsets, data_bytes, trailer, size, count)."""
    start = np.asarray(block_start, dtype=np.int64)
    first = np.asarray(block_first, dtype=np.int64)
    nb = start.size
    if nb == 0:
        keys, out, offsets, data_bytes = [], [], np.zeros(0, dtype=np.int64), 0
    else:
        fi = start >> BASE_LG
        edge = fi[1:] != fi[:-1]
        g0 = np.nonzero(np.concatenate([[True], edge]))[0]   # every filter's first block
        g1 = np.nonzero(np.concatenate([edge, [True]]))[0]   # and its last
        k0, k1 = first[g0], first[g1 + 1]
        size = filter_bytes(k1 - k0, bits_per_key)
        before = np.concatenate([[0], np.cumsum(size)])
        fi_end = int(data_end) >> BASE_LG
        slots = fi_end + (1 if fi_end == int(fi[-1]) else 0)
        # slot s: the bytes of the filters whose slot is below s
        offsets = before[np.searchsorted(fi[g0], np.arange(slots), side="left")]
        keys, out, data_bytes = list(zip(k0.tolist(), k1.tolist())), before[:-1].tolist(), int(before[-1])
    trailer = b"".join(int(o).to_bytes(4, "little") for o in offsets) + int(data_bytes).to_bytes(4, "little") + \
        bytes([BASE_LG])
    return dict(filter_keys=keys, filter_out=out, offsets=[int(o) for o in offsets], data_bytes=data_bytes,
                trailer=trailer, size=data_bytes + len(trailer), count=len(keys))


def starts_of(sizes):
    """(block_start, data_end) of blocks written back to back with their trailers."""
    sizes = np.asarray(sizes, dtype=np.int64)
    ends = np.cumsum(sizes + TRAILER)
    return np.concatenate([[0], ends[:-1]]).astype(np.int64) if sizes.size else np.zeros(0, dtype=np.int64), \
        int(ends[-1]) if sizes.size else 0


def firsts_of(n_blocks, base=0):
    """block_first for blocks of 1..5 keys in turn, from entry `base`."""
    return base + np.concatenate([[0], np.cumsum([(b % 5) + 1 for b in range(n_blocks)])]).astype(np.int64)


# name -> block sizes
LAYOUT_CASES = {
    "many_32": [32] * 200,                        # 55 blocks a window
    "many_256": [256] * 40,
    "above_4k": [5000, 9000, 100, 3 * 4096, 60],  # empty slots
    "on_2048": [2043, 300, 300],                  # block 1 starts at 2,048
    "below_2048": [2042, 300, 300],               # at 2,047
    "above_2048": [2044, 300, 300],               # at 2,049
    "end_on_2048": [2043, 2043],                  # data_end 4,096
    "end_below": [2043, 2042],
    "end_above": [2043, 2044],
    "single": [100],
    "single_large": [7000],
    "none": [],
}
