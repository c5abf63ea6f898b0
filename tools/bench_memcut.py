#!/usr/bin/env python3
"""The memtable switch's times on one GPU, on the
db_bench shape of section 16: 9,437,184 entries of 23-byte keys and 100-byte
values, as one-entry and as 1,000-entry records, with write_buffer_size 8 MiB
and 64 KiB.  Kernel times are HIP events around `reps` calls after warm-up
calls; each figure is the median of `rounds` such measurements.  One JSON line
per measurement:

  heights        lsbm_skiplist_heights_dev of all the entries
  cut            lsbm_memtable_cut_dev (its two heights tables included), RECOVER
                 and WRITE; walk "wave" is the kept arrangement, "lane" the
                 one-lane walk (LSBM_MEMCUT_WALK=lane), RECOVER
  host_copy      what the device call replaces, part 1: the key and value lengths
                 (two uint32 arrays) and the records' running sums copied to the
                 host (host clock, pageable destination as torch's .cpu() gives it)
  host_loop      part 2: tools/memcut_host.cc's loop over them, one thread (host
                 clock); its cut list is checked against the device's
  recover_all    memtable.recover_all of a log of --e2e-ops such entries, end to
                 end (host clock), and one memtable.flush of the same log's records

Recorded, not gated.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from bench_snappy import timed  # noqa: E402


def host_lib(path):
    if path is None:
        path = os.path.join(tempfile.mkdtemp(), "libmemcut_host.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", path, os.path.join(HERE, "memcut_host.cc")],
                       check=True)
    lib = ctypes.CDLL(path)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    lib.memcut_host.restype = ctypes.c_int
    lib.memcut_host.argtypes = [vp, vp, u64, vp, u64, vp, u32, u64, vp, vp, vp, vp, u64, vp, vp]
    return lib


def host_clock(torch, fn, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=9437184)
    ap.add_argument("--e2e-ops", type=int, default=None)
    ap.add_argument("--key-bytes", type=int, default=23)
    ap.add_argument("--value-bytes", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-lib", default=None, help="a built tools/memcut_host.cc (default: built into a temp dir)")
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from lsbm_amd import engine, memtable, write
    engine.init(0)
    lib = host_lib(a.host_lib)
    n = a.ops
    dev = torch.cuda.get_device_name(0)

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    t = median(lambda: memtable.heights(n))
    print(json.dumps({"what": "heights", "entries": n, "ms": round(t * 1e3, 4), "device": dev}), flush=True)

    koff = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (a.key_bytes + 8)
    values = torch.stack([torch.zeros(n, dtype=torch.int64, device="cuda"),
                          torch.full((n,), a.value_bytes, dtype=torch.int64, device="cuda")], 1).reshape(-1).contiguous()
    for batch in (1, 1000):
        nr = (n + batch - 1) // batch
        base = (torch.arange(nr + 1, dtype=torch.int64, device="cuda") * batch).clamp(max=n)
        for wbs in (8 << 20, 64 << 10):
            shape = {"entries": n, "records": nr, "write_buffer_size": wbs, "device": dev}
            outs = dict(usage=torch.zeros(nr, dtype=torch.int64, device="cuda"),
                        mem_first=torch.zeros(nr + 2, dtype=torch.int64, device="cuda"),
                        mem_usage=torch.zeros(nr + 1, dtype=torch.int64, device="cuda"))
            for mode, name in ((memtable.RECOVER, "recover"), (memtable.WRITE, "write")):
                def fn():
                    return memtable.cut(koff, values, base, mode, wbs, **outs)
                r = fn()
                assert int(r.status.cpu()[0]) == 0
                n_mem = int(r.counts.cpu()[0])
                t = median(fn)
                print(json.dumps(dict(shape, what="cut", walk="wave", mode=name, memtables=n_mem,
                                      ms=round(t * 1e3, 4), ns_per_entry=round(t * 1e9 / n, 3))), flush=True)
            os.environ["LSBM_MEMCUT_WALK"] = "lane"
            try:
                mode = memtable.RECOVER
                n_mem = int(fn().counts.cpu()[0])
                t = statistics.median(timed(torch, fn, 2) for _ in range(3))  # (median of 3 x 2: it is the slow one)
            finally:
                del os.environ["LSBM_MEMCUT_WALK"]
            print(json.dumps(dict(shape, what="cut", walk="lane", mode="recover", memtables=n_mem,
                                  ms=round(t * 1e3, 4), ns_per_entry=round(t * 1e9 / n, 3))), flush=True)
            # the alternative: the lengths and the running sums to the host, then one thread
            def copy():
                ikl = (koff[1:] - koff[:-1]).to(torch.int32)
                vl = values[1::2].to(torch.int32)
                return ikl.cpu(), vl.cpu(), base.cpu()
            t_copy = host_clock(torch, copy, a.rounds)
            ikl, vl, hbase = (x.numpy() for x in copy())
            usage, first = np.zeros(nr, np.uint64), np.zeros(nr + 2, np.uint64)
            ended, counts, state = np.zeros(nr + 1, np.uint64), np.zeros(2, np.uint64), np.zeros(6, np.uint64)

            def loop(mode=memtable.RECOVER):
                rc = lib.memcut_host(ikl.ctypes.data, vl.ctypes.data, n, hbase.ctypes.data, nr, None, mode, wbs, None,
                                     usage.ctypes.data, first.ctypes.data, ended.ctypes.data, nr + 1,
                                     counts.ctypes.data, state.ctypes.data)
                assert rc == 0
            t_loop = host_clock(torch, loop, a.rounds)
            r = memtable.cut(koff, values, base, memtable.RECOVER, wbs, **outs)
            n_mem = int(r.counts.cpu()[0])
            assert int(counts[0]) == n_mem
            assert np.array_equal(first[:n_mem + 1].astype(np.int64), r.mem_first[:n_mem + 1].cpu().numpy())
            assert np.array_equal(usage.astype(np.int64), r.usage.cpu().numpy())
            assert np.array_equal(state.astype(np.int64), r.state.cpu().numpy())
            print(json.dumps(dict(shape, what="host_copy", ms=round(t_copy * 1e3, 3))), flush=True)
            print(json.dumps(dict(shape, what="host_loop", mode="recover", ms=round(t_loop * 1e3, 3),
                                  ns_per_entry=round(t_loop * 1e9 / n, 3))), flush=True)
    if a.no_e2e:
        return
    # end to end: a log of 1,000-entry batches, recovered into its memtables, and flushed as one
    ne = a.e2e_ops or n
    g = torch.Generator(device="cuda").manual_seed(7)
    keys = torch.randint(0, 256, (ne * a.key_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    vimg = torch.randint(0, 256, (ne * a.value_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    ko = torch.arange(ne + 1, dtype=torch.int64, device="cuda") * a.key_bytes
    vals = torch.stack([torch.arange(ne, dtype=torch.int64, device="cuda") * a.value_bytes,
                        torch.full((ne,), a.value_bytes, dtype=torch.int64, device="cuda")], 1).reshape(-1).contiguous()
    types = torch.ones(ne, dtype=torch.uint8, device="cuda")
    nw = (ne + 999) // 1000
    bf = (torch.arange(nw + 1, dtype=torch.int64, device="cuda") * 1000).clamp(max=ne)
    log = write.write_batches(types, keys, ko, vimg, vals, bf).log
    del keys, vimg
    for wbs in (8 << 20, 64 << 10):
        small = wbs < (1 << 20)  # thousands of tables: one timed run, after the other size has warmed the allocator
        if not small:
            memtable.recover_all(log, write_buffer_size=wbs)
        tables = []
        t = host_clock(torch, lambda: tables.append(len(memtable.recover_all(log, write_buffer_size=wbs).flushes)),
                       1 if small else 3)
        print(json.dumps({"what": "recover_all", "entries": ne, "log_bytes": log.numel(), "write_buffer_size": wbs,
                          "tables": tables[-1], "ms": round(t * 1e3, 1), "device": dev}), flush=True)
    t = host_clock(torch, lambda: memtable.recover(log), 3)
    print(json.dumps({"what": "recover_one_flush", "entries": ne, "log_bytes": log.numel(), "ms": round(t * 1e3, 1),
                      "device": dev}), flush=True)


if __name__ == "__main__":
    main()
