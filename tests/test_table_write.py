"""CPU tests of the batched table finish (include/lsbm_table_write.h): the
closed-form filter layout the device uses against FilterBlockBuilder's loop
(lsbm_amd.bloom.layout_filter_block), and the header against the library.
"""
import os
import re

import numpy as np
import pytest

from golden import tablewritemodel as tw

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def loop_layout(bloom, sizes, bits_per_key, entry_base=0):
    """layout_filter_block as the table writers call it: StartBlock for every
    block and for the offset after the last one."""
    start, end = tw.starts_of(sizes)
    first = tw.firsts_of(len(sizes), entry_base)
    nb = len(sizes)
    return bloom.layout_filter_block(list(start) + ([end] if nb else []), list(first) + ([first[-1]] if nb else []),
                                     bits_per_key)


@pytest.mark.parametrize("name", sorted(tw.LAYOUT_CASES))
@pytest.mark.parametrize("bits_per_key", [10, 1])
def test_closed_form_equals_the_loop(product_lib, name, bits_per_key):
    from lsbm_amd import bloom
    sizes = tw.LAYOUT_CASES[name]
    start, end = tw.starts_of(sizes)
    first = tw.firsts_of(len(sizes), 7)
    got = tw.filter_layout(start, first, end, bits_per_key)
    want = loop_layout(bloom, sizes, bits_per_key, 7)
    assert got["filter_keys"] == [tuple(int(x) for x in k) for k in want.filter_keys]
    assert got["filter_out"] == want.filter_out and got["offsets"] == want.offsets
    assert got["data_bytes"] == want.data_bytes and got["trailer"] == want.trailer
    assert got["size"] == want.total_bytes


def test_cases_land_where_they_say():
    at = {name: tw.starts_of(s) for name, s in tw.LAYOUT_CASES.items()}
    assert at["on_2048"][0][1] == 2048 and at["below_2048"][0][1] == 2047 and at["above_2048"][0][1] == 2049
    assert at["end_on_2048"][1] == 4096 and at["end_below"][1] == 4095 and at["end_above"][1] == 4097
    assert max(np.diff(at["above_4k"][0])) > 4096 and at["none"][1] == 0
    # many blocks in one 2 KiB window, and empty slots
    assert len(set((at["many_32"][0] >> 11).tolist())) == 4  # (200 blocks: more than 50 a window)
    lay = tw.filter_layout(at["above_4k"][0], tw.firsts_of(5), at["above_4k"][1], 10)
    assert len(lay["offsets"]) > lay["count"] + 3


def test_symbols_exported_and_declared(product_lib):
    from lsbm_amd import _lib
    text = open(os.path.join(REPO, "include", "lsbm_table_write.h")).read()
    names = sorted(set(re.findall(r"\b(lsbm_\w+)\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(_lib.TABLE_WRITE_SIGNATURES) and len(names) == 7
    for name in names:
        assert hasattr(product_lib, name), name


def test_entry_points_check_arguments(product_lib):
    """Null pointers, a short or misaligned scratch and a tail of 4 blocks are
    LSBM_ERR_INVALID before any device is touched."""
    import ctypes
    from lsbm_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.lsbm_table_write_scratch_bytes(0, 0) == 8 * 3
    assert lib.lsbm_table_write_scratch_bytes(257, 3) == 8 * (2 * 257 + 2 * 3 + 1)
    assert lib.lsbm_memtable_sort_segments_scratch_bytes(3, 2) == 48 + 3 * 16 + 8 + 8 + 8
    assert lib.lsbm_table_pack_plan_dev(p, None, 1, None, 1, None, 5, p, p, p, p, p, 512, None) == _lib.LSBM_ERR_INVALID
    assert lib.lsbm_table_pack_plan_dev(p, None, 1, p, 1, None, 5, p, p, p, p, p, 8, None) == _lib.LSBM_ERR_INVALID
    assert lib.lsbm_table_place_dev(p, 0, p, p, 4, p, p, 1, p, 64, p, p, p, p, p, 512, None) == _lib.LSBM_ERR_INVALID
    assert lib.lsbm_memtable_sort_segments_dev(None, 0, p, 0, None, 0, None, p, p, p, p, 512, None) == \
        _lib.LSBM_ERR_INVALID
    assert lib.lsbm_metaindex_build_dev(None, None, 1, p, None, 0, None, p, None) == _lib.LSBM_ERR_INVALID
    assert lib.lsbm_filter_layout_dev(p, p, 0, 0, None, None, -1, None, None, None, None, 0, None, 0, None, None, p,
                                      512, None) == _lib.LSBM_ERR_INVALID
