#!/usr/bin/env python3
"""The batched table finish against the per-table loop on one GPU (DESIGN.md
section 22), both in the same run: the loop is the code the batched path
leaves untouched (batched=False).  Host clock around whole calls, as section
21 timed recover_all; each figure is the median of `rounds` calls after
`warmup` untimed ones.  One JSON line per measurement:

  recover_all    memtable.recover_all of a log of --ops entries of 23-byte keys
                 and 100-byte values in 1,000-entry batches, at write_buffer_size
                 64 KiB and 8 MiB, batched False and True
  compact        sstable.compact of three overlapping runs of --compact-ops
                 entries each into files of --max-file-size bytes (at least 100
                 output tables), batched False and True

Every line carries the count of device-to-host reads (torch.Tensor.cpu, .item
and .tolist) one call makes.  Recorded, not gated.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def host_clock(torch, fn, warmup, rounds):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=2000000)
    ap.add_argument("--key-bytes", type=int, default=23)
    ap.add_argument("--value-bytes", type=int, default=100)
    ap.add_argument("--compact-ops", type=int, default=30000)
    ap.add_argument("--max-file-size", type=int, default=64 << 10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-recover", action="store_true")
    ap.add_argument("--no-compact", action="store_true")
    a = ap.parse_args()
    import torch
    from lsbm_amd import engine, memtable, sstable, write
    engine.init(0)
    dev = torch.cuda.get_device_name(0)

    if not a.no_recover:
        ne = a.ops
        g = torch.Generator(device="cuda").manual_seed(7)
        keys = torch.randint(0, 256, (ne * a.key_bytes,), dtype=torch.uint8, device="cuda", generator=g)
        vimg = torch.randint(0, 256, (ne * a.value_bytes,), dtype=torch.uint8, device="cuda", generator=g)
        ko = torch.arange(ne + 1, dtype=torch.int64, device="cuda") * a.key_bytes
        vals = torch.stack([torch.arange(ne, dtype=torch.int64, device="cuda") * a.value_bytes,
                            torch.full((ne,), a.value_bytes, dtype=torch.int64, device="cuda")], 1)
        vals = vals.reshape(-1).contiguous()
        types = torch.ones(ne, dtype=torch.uint8, device="cuda")
        nw = (ne + 999) // 1000
        bf = (torch.arange(nw + 1, dtype=torch.int64, device="cuda") * 1000).clamp(max=ne)
        log = write.write_batches(types, keys, ko, vimg, vals, bf).log
        del keys, vimg
        for wbs in (64 << 10, 8 << 20):
            for batched in (False, True):
                tables = []

                def fn():
                    tables.append(len(memtable.recover_all(log, write_buffer_size=wbs, batched=batched).flushes))
                t = host_clock(torch, fn, a.warmup, a.rounds)
                reads = count_reads(torch, fn)
                print(json.dumps({"what": "recover_all", "batched": batched, "entries": ne, "log_bytes": log.numel(),
                                  "write_buffer_size": wbs, "tables": tables[-1], "ms": round(t * 1e3, 1),
                                  "host_reads": reads, "device": dev}), flush=True)
        del log

    if not a.no_compact:
        n = a.compact_ops
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
            vimg = torch.randint(0, 256, (m * a.value_bytes,), dtype=torch.uint8, device="cuda", generator=g)
            vals = torch.stack([torch.arange(m, dtype=torch.int64, device="cuda") * a.value_bytes,
                                torch.full((m,), a.value_bytes, dtype=torch.int64, device="cuda")], 1)
            image, h, _ = sstable.write_table(keys, ko, vals, vimg, bits_per_key=10, compression=0)
            images.append(image)
            handles.append(h.cpu().numpy())
        for compression in (0, 1):
            for batched in (False, True):
                tables = []

                def fn():
                    tables.append(len(sstable.compact(images, handles, a.max_file_size, bits_per_key=10,
                                                      compression=compression, batched=batched)))
                t = host_clock(torch, fn, a.warmup, a.rounds)
                reads = count_reads(torch, fn)
                print(json.dumps({"what": "compact", "batched": batched, "compression": compression,
                                  "entries": 3 * n, "max_file_size": a.max_file_size, "tables": tables[-1],
                                  "ms": round(t * 1e3, 1), "host_reads": reads, "device": dev}), flush=True)


if __name__ == "__main__":
    main()
