#!/usr/bin/env python3
"""The calls that write tables, end to end on one GPU:
all of them go through the one chain (sstable.write_tables / finish_tables).
Host clock around whole calls that end in a synchronise, as section 21 timed
recover_all; each figure is the median of `rounds` calls after `warmup` untimed
ones, and every line carries the fastest and the slowest round too.  One JSON
line per measurement:

  recover_all    memtable.recover_all of a log of --ops entries of 23-byte keys
                 and 100-byte values in 1,000-entry batches, at write_buffer_size
                 64 KiB and 8 MiB
  compact        sstable.compact of three overlapping runs of --compact-ops
                 entries each into files of --max-file-size bytes (at least 100
                 output tables), both compressions; merge_compact: merge.compact
                 of the same runs
  write_table    sstable.write_table of one table: the entries of --table-blocks
                 db_bench-shaped blocks (tools/bench_table_pack.py's shape), both
                 compressions, bloom 10; table_build: block_build.table_build of
                 the same entries
  flush          memtable.flush of one memtable: the entries of --flush-blocks
                 such blocks as WriteBatch payloads in a random arrival order
                 (tools/bench_memtable.py's shape)

Every line carries the count of device-to-host reads (torch.Tensor.cpu, .item
and .tolist) one call makes.  Recorded, not gated.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)


def host_clock(torch, fn, warmup, rounds):
    """Seconds of `rounds` calls of fn, each ending in a synchronise, after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def count_reads(torch, fn):
    """The device-to-host reads of one call of fn."""
    counts, real = {}, {}
    for name in ("cpu", "item", "tolist"):
        real[name] = getattr(torch.Tensor, name)

        def call(self, *a, _name=name, **kw):
            counts[_name] = counts.get(_name, 0) + 1
            return real[_name](self, *a, **kw)
        setattr(torch.Tensor, name, call)
    try:
        fn()
    finally:
        for name, f in real.items():
            setattr(torch.Tensor, name, f)
    return sum(counts.values())


def recover_log(torch, ops, key_bytes=23, value_bytes=100):
    """A sealed log of `ops` entries in 1,000-entry batches, in device memory."""
    from lsbm_amd import write
    g = torch.Generator(device="cuda").manual_seed(7)
    keys = torch.randint(0, 256, (ops * key_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    vimg = torch.randint(0, 256, (ops * value_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    ko = torch.arange(ops + 1, dtype=torch.int64, device="cuda") * key_bytes
    vals = torch.stack([torch.arange(ops, dtype=torch.int64, device="cuda") * value_bytes,
                        torch.full((ops,), value_bytes, dtype=torch.int64, device="cuda")], 1)
    vals = vals.reshape(-1).contiguous()
    types = torch.ones(ops, dtype=torch.uint8, device="cuda")
    nw = (ops + 999) // 1000
    bf = (torch.arange(nw + 1, dtype=torch.int64, device="cuda") * 1000).clamp(max=ops)
    return write.write_batches(types, keys, ko, vimg, vals, bf).log


def compact_runs(torch, n, value_bytes=100):
    """Three overlapping kNoCompression runs of n entries each: (images, handles)."""
    from lsbm_amd import sstable
    images, handles = [], []
    for r in range(3):  # run r: every (r + 1)-th user key of 2n, newest run first
        users = torch.arange(0, 2 * n, r + 1, dtype=torch.int64, device="cuda")[:n]
        m = users.numel()
        # internal keys: the user number big-endian, twice (16 bytes), then the tag
        ub = torch.stack([(users >> (8 * (7 - i))) & 255 for i in range(8)], 1).to(torch.uint8)
        tag = torch.full((m,), ((100 - r) << 8) | 1, dtype=torch.int64, device="cuda")
        tb = torch.stack([(tag >> (8 * i)) & 255 for i in range(8)], 1).to(torch.uint8)
        keys = torch.cat([ub, ub, tb], 1).reshape(-1).contiguous()
        ko = torch.arange(m + 1, dtype=torch.int64, device="cuda") * 24
        g = torch.Generator(device="cuda").manual_seed(11 + r)
        vimg = torch.randint(0, 256, (m * value_bytes,), dtype=torch.uint8, device="cuda", generator=g)
        vals = torch.stack([torch.arange(m, dtype=torch.int64, device="cuda") * value_bytes,
                            torch.full((m,), value_bytes, dtype=torch.int64, device="cuda")], 1)
        image, h, _ = sstable.write_table(keys, ko, vals, vimg, bits_per_key=10, compression=0)
        images.append(image)
        handles.append(h.cpu().numpy())
    return images, handles


def table_entries(torch, n_blocks):
    """The entries of n_blocks db_bench-shaped blocks: (keys, key_offsets, values, value_image)."""
    from bench_snappy import make_blocks
    from lsbm_amd import block
    img, offs = make_blocks(n_blocks)
    raw = torch.from_numpy(img).cuda()
    handles = torch.from_numpy(np.stack([offs[:-1], offs[1:] - offs[:-1]], 1).astype(np.int64).reshape(-1)).cuda()
    keys, koff, values, _, st = block.decode(raw, handles)
    assert int(st.max()) == 0
    return keys, koff, values.reshape(-1).contiguous(), raw


def memtable_records(torch, n_blocks):
    """Those entries as one-entry WriteBatch payloads in a random arrival order: (image, records)."""
    from bench_memtable import payloads
    keys, koff, values, raw = table_entries(torch, n_blocks)
    n = koff.numel() - 1
    klen, vlen = int(koff[1] - koff[0]), int(values[1])
    users = keys.view(n, klen)[:, :klen - 8]
    vals = raw[(values.view(n, 2)[:, 0:1] + torch.arange(vlen, device="cuda")).reshape(-1)].view(n, vlen)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x3E37AB1E)
    return payloads(torch, users, vals, torch.randperm(n, device="cuda", generator=g), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=2000000)
    ap.add_argument("--compact-ops", type=int, default=30000)
    ap.add_argument("--max-file-size", type=int, default=64 << 10)
    ap.add_argument("--table-blocks", type=int, default=512)
    ap.add_argument("--flush-blocks", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-recover", action="store_true")
    ap.add_argument("--no-compact", action="store_true")
    ap.add_argument("--no-table", action="store_true")
    ap.add_argument("--no-flush", action="store_true")
    a = ap.parse_args()
    import torch
    from lsbm_amd import block_build, engine, memtable, merge, sstable
    from lsbm_amd.block import INTERNAL_KEY
    engine.init(0)
    dev = torch.cuda.get_device_name(0)

    def row(what, fn, **kw):
        ts = host_clock(torch, fn, a.warmup, a.rounds)
        print(json.dumps({"what": what, **kw, "ms": round(statistics.median(ts) * 1e3, 1),
                          "ms_min": round(min(ts) * 1e3, 1), "ms_max": round(max(ts) * 1e3, 1),
                          "host_reads": count_reads(torch, fn), "device": dev}), flush=True)

    if not a.no_recover:
        log = recover_log(torch, a.ops)
        for wbs in (64 << 10, 8 << 20):
            tables = len(memtable.recover_all(log, write_buffer_size=wbs).flushes)
            row("recover_all", lambda: memtable.recover_all(log, write_buffer_size=wbs), entries=a.ops,
                log_bytes=log.numel(), write_buffer_size=wbs, tables=tables)
        del log

    if not a.no_compact:
        images, handles = compact_runs(torch, a.compact_ops)
        shape = dict(entries=3 * a.compact_ops, max_file_size=a.max_file_size)
        for compression in (0, 1):
            tables = len(sstable.compact(images, handles, a.max_file_size, bits_per_key=10, compression=compression))
            row("compact", lambda: sstable.compact(images, handles, a.max_file_size, bits_per_key=10,
                                                   compression=compression), compression=compression, tables=tables,
                **shape)
        tables = len(merge.compact(images, handles, a.max_file_size, bits_per_key=10))
        row("merge_compact", lambda: merge.compact(images, handles, a.max_file_size, bits_per_key=10), compression=0,
            tables=tables, **shape)
        del images

    if not a.no_table:
        keys, koff, values, raw = table_entries(torch, a.table_blocks)
        shape = dict(entries=koff.numel() - 1, table_blocks=a.table_blocks, tables=1)
        for compression in (1, 0):
            row("write_table", lambda: sstable.write_table(keys, koff, values, raw, INTERNAL_KEY, 4096, 16, 10,
                                                           compression), compression=compression, **shape)
        row("table_build", lambda: block_build.table_build(keys, koff, values, raw, INTERNAL_KEY, 4096, 16, 10),
            compression=0, **shape)
        del keys, koff, values, raw

    if not a.no_flush:
        image, records = memtable_records(torch, a.flush_blocks)
        row("flush", lambda: memtable.flush(image, records), compression=0, entries=records.numel() // 2, tables=1)


if __name__ == "__main__":
    main()
