#!/usr/bin/env python3
"""LSbM's RangeQuery on one GPU: RangeQuery.query over
the tree of tools/bench_buffered_get.py (section 24: the reference's default list
lengths, compaction_buffer_use_length 0, 20, 20, 0, buffered_merge on), all
resident in HBM, read_upto_key above every key so that the compaction buffers
are read.

Queries come in batches of `--queries` ranges of `--range-sizes` consecutive
keys of the universe (db_bench's FLAGS_range_size: lsbm/db_bench.cc:1004-1026),
starting at random present keys.

One JSON line per measurement.  Device times are HIP events around one call
after a warm-up call, the median of `--rounds`; end-to-end times are the host
clock around a synchronised call, the median of `--rounds`:

  index        the range index's build (once; host clock), its bytes and entries
  plan         lsbm_range_plan_dev, the prefix sum, lsbm_range_emit_dev
  count        lsbm_range_count_dev: `pairs` (query, file) pairs, `entries` entries counted
  query        RangeQuery.query end to end
  host_count   tools/range_host.cc over the same pairs of the first `--host-queries` queries, one thread

Recorded, not gated.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

KLEN = 16
PREFIX = b"userkey-"


def host_lib():
    so = os.path.join(REPO, "build", "librangehost.so")
    src = os.path.join(HERE, "range_host.cc")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.range_host_count.restype = ctypes.c_double
    lib.range_host_count.argtypes = [vp, u64, vp, vp, vp, vp, vp, u64, vp]
    return lib


def user_keys(ids):
    """uint8[len(ids), 16]: the prefix, then the id big-endian (so ids order the keys)."""
    out = np.empty((len(ids), KLEN), dtype=np.uint8)
    out[:, :8] = np.frombuffer(PREFIX, dtype=np.uint8)
    out[:, 8:] = np.asarray(ids, dtype=">u8").view(np.uint8).reshape(-1, 8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--universe", type=int, default=1 << 16)
    ap.add_argument("--queries", type=int, default=1 << 16)
    ap.add_argument("--range-sizes", type=int, nargs="+", default=[100, 10000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=2048)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    from lsbm_amd import buffered, db, engine, rangequery, sstable
    from lsbm_amd.table import kNoCompression
    engine.init(0)
    rng = np.random.default_rng(0xB0FF)
    M = a.universe
    universe = user_keys(np.arange(M, dtype=np.uint64) * 7919)
    value_image = torch.from_numpy(rng.integers(0, 256, size=64 * M, dtype=np.uint8)).cuda()
    tables = []  # (sorted ids into the universe, file bytes, internal keys)

    def table(share):
        ids = np.flatnonzero(rng.random(M) < share)
        number = len(tables) + 1
        keys = np.concatenate([universe[ids], np.tile(np.frombuffer(((number << 8) | 1).to_bytes(8, "little"),
                                                                    dtype=np.uint8), (len(ids), 1))], 1)
        dk = torch.from_numpy(keys.reshape(-1).copy()).cuda()
        off = torch.arange(len(ids) + 1, device="cuda", dtype=torch.int64) * (KLEN + 8)
        values = torch.stack([torch.from_numpy(ids.astype(np.int64)).cuda() * 64,
                              torch.full((len(ids),), 64, dtype=torch.int64, device="cuda")], 1)
        image, _, _ = sstable.write_table(dk, off, values.reshape(-1).contiguous(), value_image, bits_per_key=10,
                                          compression=kNoCompression)
        data = bytes(image.cpu().numpy())
        tables.append((ids, data, keys))
        return (number, len(data), keys[0].tobytes(), keys[-1].tobytes())

    structure = {(0, 0): [[table(1 / 32), table(1 / 32)]], (0, 1): [[table(1 / 32)]]}
    cb_length, ins_share = (0, 20, 20, 3), (0, 1 / 8, 1 / 2, 1.0)
    for level in (1, 2, 3):
        structure[(level, 0)] = [[table(1 / 16)]]
        structure[(level, 1)] = [[table(ins_share[level])]]
        structure[(level, 2)] = [[]] + [[table(1 / 16)] for _ in range(cb_length[level])]
        structure[(level, 3)] = [[]] + ([[table(1 / 16)] for _ in range(20)] if level > 1 else [])
    files = {t + 1: db.TableFile(data, t + 1, 10) for t, (_, data, _) in enumerate(tables)}
    use_length = (0, 20, 20, 0)
    bv = buffered.BufferedVersion(structure, files, use_length, True)
    rq = rangequery.RangeQuery(bv, b"\xff")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = rq.index
    torch.cuda.synchronize()
    t_index = time.perf_counter() - t0
    shape = {"universe": M, "queries": a.queries, "tables": len(tables), "slots": len(rq.slots),
             "arena_bytes": bv.version.arena.numel(), "use_length": list(use_length),
             "device": torch.cuda.get_device_name(0)}
    nq = a.queries
    print(json.dumps({"metric": "index", "ms": round(t_index * 1e3, 3), "host_clock": True,
                      "entries": index.key_offsets.numel() - 1,
                      "index_bytes": index.keys.numel() + 8 * index.key_offsets.numel(), **shape}), flush=True)
    uoff = torch.arange(nq + 1, device="cuda", dtype=torch.int64) * KLEN
    snapshot = (1 << 56) - 1

    def device_time(fn):
        fn()  # warm-up
        times = []
        for _ in range(a.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop) / 1e3)
        return statistics.median(times)

    def host_time(fn):
        fn()  # warm-up
        times = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return statistics.median(times)

    for size in a.range_sizes:
        def emit(metric, seconds, n=nq, **kw):
            print(json.dumps({"metric": metric, "range_size": size, "queries_per_s": round(n / seconds),
                              "ms": round(seconds * 1e3, 3), **shape, **kw}), flush=True)

        pick = rng.integers(0, M, size=nq)
        upto = np.minimum(pick + size, M - 1)
        sk = torch.from_numpy(user_keys(pick.astype(np.uint64) * 7919).reshape(-1).copy()).cuda()
        ek = torch.from_numpy(user_keys(upto.astype(np.uint64) * 7919).reshape(-1).copy()).cuda()
        skeys, soff, _ = db.lookup_keys(sk, uoff, snapshot)
        ekeys, eoff, _ = db.lookup_keys(ek, uoff, snapshot)
        plan_args = rq._plan_args() + (skeys, soff, ekeys, eoff)
        count, _ = rangequery.range_plan(*plan_args)
        first = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(count, 0, out=first[1:])
        pairs = int(first[-1].cpu())
        pair_run = torch.zeros(max(pairs, 1), dtype=torch.int32, device="cuda")[:pairs]
        pair_flags = torch.zeros(max(pairs, 1), dtype=torch.int32, device="cuda")[:pairs]
        checked = torch.zeros(nq, dtype=torch.int32, device="cuda")

        def plan():
            c, _ = rangequery.range_plan(*plan_args)
            torch.cumsum(c, 0, out=first[1:])
            rangequery.range_emit(*plan_args, first, pair_run, pair_flags, checked, pairs)
        emit("plan", device_time(plan), pairs=pairs, max_pairs=int(count.max().cpu()))
        pair_file = rq.run_file[pair_run.to(torch.int64)].contiguous()
        outs = rangequery.range_count(index, skeys, soff, ekeys, eoff, first, pair_file, pair_flags)
        t = device_time(lambda: rangequery.range_count(index, skeys, soff, ekeys, eoff, first, pair_file, pair_flags,
                                                       *outs[:4]))
        entries = int(outs[3].sum().cpu())
        emit("count", t, pairs=pairs, entries=entries, entries_per_s=round(entries / t),
             found=int(outs[2].to(torch.int64).sum().cpu()))
        emit("query", host_time(lambda: rq.query(sk, uoff, ek, uoff, snapshot)), host_clock=True, pairs=pairs,
             entries=entries)
        if a.no_host:
            continue
        hl = host_lib()
        hn = min(a.host_queries, nq)
        hkeys = np.ascontiguousarray(np.concatenate([keys for _, _, keys in tables]))
        tfirst = np.zeros(len(tables) + 1, np.uint64)
        np.cumsum([len(ids) for ids, _, _ in tables], out=tfirst[1:])
        hfirst = first.cpu().numpy().astype(np.uint64)
        # (file f of the version is table f: BufferedVersion opens the files in the structure's order)
        numbers = rq.numbers.cpu().numpy()
        htable = np.ascontiguousarray((numbers[pair_file.cpu().numpy()] - 1).astype(np.int32))
        hs, he = skeys.cpu().numpy(), ekeys.cpu().numpy()
        hcounts = np.zeros(max(pairs, 1), np.uint32)
        dt = hl.range_host_count(hkeys.ctypes.data, KLEN + 8, tfirst.ctypes.data, hs.ctypes.data, he.ctypes.data,
                                 hfirst.ctypes.data, htable.ctypes.data, hn, hcounts.ctypes.data)
        hp = int(hfirst[hn])
        assert np.array_equal(hcounts[:hp], outs[0].cpu().numpy()[:hp].astype(np.uint32)), "host loop != GPU count"
        emit("host_count", dt, n=hn, threads=1, host_queries=hn, pairs=hp, entries=int(hcounts[:hp].sum()),
             entries_per_s=round(int(hcounts[:hp].sum()) / dt))


if __name__ == "__main__":
    main()
