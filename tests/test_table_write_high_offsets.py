"""The batched table finish at offsets past 4 GiB (arranged like
tests/test_high_offsets.py, whose helpers' constants it shares): two small
tables placed by lsbm_table_place_dev at bases past 2^32 in a sparse arena,
with a decoy table 2^32 below each base, and the segmented sort with its key
window past 4 GiB.  A kernel that drops the high half of an offset writes the
decoy's place or sorts the decoy's keys.
"""
import random

import numpy as np
import pytest

from golden import blockmodel as bm
from golden import memtablemodel as mt
from golden import snappy_table_cases as tc
from high_offsets import ARENA_BYTES, FILL, GUARD, LINE
from test_memtable_gpu import ikey
from test_sstable import Entries, _dev

pytestmark = pytest.mark.gpu


def test_tables_and_segmented_sort_past_4gib(torch_cuda):
    from lsbm_amd import memtable, sstable
    torch = torch_cuda
    # ---- two tables through the chain at base 0: the reference run
    tables = [tc._blocks_of_kinds("rxr", 128, 4, 11), tc._blocks_of_kinds("xr", 128, 4, 12)]
    E = Entries(torch, [e for t in tables for e in t])
    first = _dev(torch, np.array([0, len(tables[0]), len(tables[0]) + len(tables[1])], dtype=np.int64))
    res = sstable.write_tables(E.keys, E.koff, E.values, E.image, first, bm.BYTEWISE, 128, 4, 10, 1)
    want = [res.table(t).cpu().numpy() for t in range(2)]
    sizes = [w.size for w in want]
    # ---- the same handles placed past the line, every block moved there
    arena = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    bases = [LINE + 4096 + 768, LINE + (1 << 24) + 256]
    decoy = [bytes([0x5A + t]) * sizes[t] for t in range(2)]
    for t, b in enumerate(bases):
        arena[b - GUARD:b + sizes[t] + GUARD].fill_(FILL)
        arena[b - LINE - GUARD:b - LINE + sizes[t] + GUARD].fill_(FILL)
        arena[b - LINE:b - LINE + sizes[t]] = torch.from_numpy(np.frombuffer(decoy[t], np.uint8).copy()).cuda()
    # the tail handles and ends of each table, read back from its own file image
    host = res.host
    tail_handles, tail_end = [], []
    for t in range(2):
        footer = want[t][-48:].tobytes()
        pos, vals = 0, []
        for _ in range(4):
            v, shift = 0, 0
            while True:
                byte = footer[pos]
                pos += 1
                v |= (byte & 127) << shift
                shift += 7
                if byte < 128:
                    break
            vals.append(v)
        tail_handles += vals
        tail_end.append(sizes[t] - 48)
        assert vals[2:] == [int(x) for x in host["index_handles"][t]]
    placed = sstable.place_tables(res.data_handles, res.table_block_first, _dev(torch, np.array(tail_handles)), 2,
                                  _dev(torch, np.array(tail_end)), _dev(torch, np.array(bases)), arena)
    assert placed.status.cpu().tolist() == [0, 0] and placed.table_size.cpu().tolist() == sizes
    tbf = [int(x) for x in host["table_block_first"]]
    rel = res.data_handles.cpu().numpy().reshape(-1, 2)
    got = placed.data_handles.cpu().numpy().reshape(-1, 2)
    for t in range(2):
        assert (got[tbf[t]:tbf[t + 1], 0] == rel[tbf[t]:tbf[t + 1], 0] + bases[t]).all()
        assert (got[tbf[t]:tbf[t + 1], 1] == rel[tbf[t]:tbf[t + 1], 1]).all()
    assert placed.tail_handles.cpu().tolist() == [v + (bases[i // 4] if i % 2 == 0 else 0)
                                                  for i, v in enumerate(tail_handles)]
    for t, b in enumerate(bases):
        assert arena[b + sizes[t] - 48:b + sizes[t]].cpu().numpy().tobytes() == want[t][-48:].tobytes()
        assert (arena[b - GUARD:b + sizes[t] - 48] == FILL).all()
        assert (arena[b + sizes[t]:b + sizes[t] + GUARD] == FILL).all()
        low = arena[b - LINE - GUARD:b - LINE + sizes[t] + GUARD].cpu().numpy().tobytes()
        assert low == bytes([FILL]) * GUARD + decoy[t] + bytes([FILL]) * GUARD  # the decoy is untouched
    # the data blocks moved to the absolute handles: the bytes at the bases equal the base-0 run's
    src = torch.cat([torch.from_numpy(w).cuda() for w in want])
    src_handles = rel.copy()
    for t in range(2):
        src_handles[tbf[t]:tbf[t + 1], 0] += sum(sizes[:t])
    types = torch.zeros(rel.shape[0], dtype=torch.uint8, device="cuda")
    st = sstable.pack(src, _dev(torch, src_handles.reshape(-1)), None, None, types, placed.data_handles, arena)
    assert st.cpu().tolist() == [0] * rel.shape[0]
    for t, b in enumerate(bases):
        for off, size in rel[tbf[t]:tbf[t + 1]].tolist():
            assert arena[b + off:b + off + size].cpu().numpy().tobytes() == want[t][off:off + size].tobytes()
        low = arena[b - LINE:b - LINE + sizes[t]].cpu().numpy().tobytes()
        assert low == decoy[t]
    # ---- the segmented sort with the key window past 4 GiB
    rng = random.Random(0x4617)
    keys = [ikey(bytes(rng.choice(b"ab") for _ in range(rng.randint(0, 9))), rng.randrange(1, 30)) for _ in range(300)]
    other = [ikey(bytes(rng.choice(b"yz") for _ in range(len(k) - 8)), rng.randrange(1, 30)) for k in keys]
    seg_first = [0, 130, 130, 300]
    koff = np.zeros(301, dtype=np.int64)
    koff[1:] = np.cumsum([len(k) for k in keys])
    at = LINE + (1 << 25) + 3
    nbytes = int(koff[-1])
    arena[at:at + nbytes] = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    arena[at - LINE:at - LINE + nbytes] = torch.from_numpy(np.frombuffer(b"".join(other), np.uint8).copy()).cuda()
    p = memtable.sort_segments(arena[:at + nbytes], _dev(torch, koff + at), _dev(torch, np.array(seg_first)))
    order = []
    for lo, hi in zip(seg_first[:-1], seg_first[1:]):
        order += [lo + i for i in mt.skiplist_order(keys[lo:hi])]
    decoy_order = []
    for lo, hi in zip(seg_first[:-1], seg_first[1:]):
        decoy_order += [lo + i for i in mt.skiplist_order(other[lo:hi])]
    assert order != decoy_order
    assert p.run_status.cpu().tolist() == [0] and p.source.cpu().tolist() == order
    assert p.counts.cpu().tolist() == [300, nbytes]
