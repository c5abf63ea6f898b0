#!/usr/bin/env python3
"""Batched DB::Get rates on one GPU, db_bench shaped: the
decoded entries of section 13's 262,144 data blocks (9,437,184 entries, fixed
key and value lengths; tools/dbbench_blocks.c) dealt at random into one
memtable of 1/16 of them, four overlapping Level-0 tables of 1/16 each, a
level 1 of four files (1/4) and a level 2 of eight files (the rest), all
resident in HBM; tables kNoCompression with a 10-bit bloom.  Queries come in
batches of `--queries` random present keys and as many absent keys (a present
key with its last byte replaced).  Kernel times are HIP events around `reps`
launches after warm-up launches; each figure is the median of `rounds` such
measurements.  One JSON line per measurement, queries/s:

  lookup_keys    lsbm_lookup_keys_dev
  memtable_get   lsbm_memtable_get_dev over the memtable (verdicts reset before each launch)
  find_file      lsbm_find_file_dev over every run
  save_value     lsbm_save_value_dev over the first table round's results (verdicts reset as above)
  slices_gather  lsbm_slices_gather_dev of the values one source found
  get            Version.get end to end by the host clock, median of 3
  host_get       the same lookups on the host (tools/get_host.cc): binary searches and
                 std::string compares, 1 thread and `--threads` threads

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
sys.path.insert(0, HERE)

from bench_snappy import make_blocks, timed  # noqa: E402


def host_lib():
    so = os.path.join(REPO, "build", "libgethost.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(HERE, "get_host.cc")], check=True)
    lib = ctypes.CDLL(so)
    vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.get_host_lookup.restype = ctypes.c_double
    lib.get_host_lookup.argtypes = [vp, u64, vp, u64, vp, vp, u64, vp, u64, u64, i, vp]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    from lsbm_amd import block, db, engine, sstable
    from lsbm_amd._lib import lib
    from lsbm_amd.engine import _ptr, _stream_ptr
    from lsbm_amd.table import kNoCompression
    engine.init(0)
    img, offs = make_blocks(a.blocks)
    in_handles = np.stack([offs[:-1], offs[1:] - offs[:-1]], 1).astype(np.int64).reshape(-1)
    dimg, dh = torch.from_numpy(img).cuda(), torch.from_numpy(in_handles).cuda()
    keys0, koff0, values0, _, st = block.decode(dimg, dh)
    assert int(st.max()) == 0
    n = koff0.numel() - 1
    klen = int(koff0[1] - koff0[0])
    assert bool(((koff0[1:] - koff0[:-1]) == klen).all()), "fixed key length"
    ulen = klen - 8
    rows = keys0.view(n, klen)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x6E7)
    # the deal: source 0 the memtable, 1-4 Level 0, 5 level 1, 6 level 2
    draw = torch.randint(0, 16, (n,), device="cuda", generator=g)
    source = torch.where(draw < 5, draw, torch.where(draw < 9, torch.full_like(draw, 5), torch.full_like(draw, 6)))

    def part(sel):
        """(keys, key_offsets, values) of the entries `sel` (ascending indices)."""
        m = sel.numel()
        return (rows[sel].reshape(-1).contiguous(), torch.arange(m + 1, device="cuda", dtype=torch.int64) * klen,
                values0[sel].contiguous())

    def table(sel, number):
        keys, off, values = part(sel)
        image, _, _ = sstable.write_table(keys, off, values.reshape(-1), dimg, bits_per_key=10,
                                          compression=kNoCompression)
        m = sel.numel()
        return db.TableFile(bytes(image.cpu().numpy()), number, 10, bytes(keys[:klen].cpu().numpy()),
                            bytes(keys[(m - 1) * klen:].cpu().numpy())), keys

    mem_sel = (source == 0).nonzero().reshape(-1)
    mk, moff, mvalues = part(mem_sel)
    mem = db.MemTable(mk, moff, mvalues, dimg)
    host_sources, level0, levels = [mk], [], []
    for s in range(1, 5):
        f, keys = table((source == s).nonzero().reshape(-1), 100 + s)
        level0.append(f)
        host_sources.append(keys)
    level0_order = sorted(range(4), key=lambda i: -level0[i].number)
    for s, pieces in ((5, 4), (6, 8)):
        sel = (source == s).nonzero().reshape(-1)
        files = []
        for p in range(pieces):
            f, keys = table(sel[sel.numel() * p // pieces:sel.numel() * (p + 1) // pieces], 10 * s + p)
            files.append(f)
            host_sources.append(keys)
        levels.append((files, []))
    version = db.Version.for_levels(level0, [], levels)
    shape = {"blocks": a.blocks, "entries": n, "queries": a.queries, "memtable_entries": mem_sel.numel(),
             "files": len(version.files), "runs": len(version.runs), "arena_bytes": version.arena.numel(),
             "user_key_bytes": ulen, "device": torch.cuda.get_device_name(0)}
    pick = torch.randint(0, n, (a.queries,), device="cuda", generator=g)
    present = rows[pick][:, :ulen].contiguous()
    absent = present.clone()
    absent[:, -1] = ord("x")
    uoff = torch.arange(a.queries + 1, device="cuda", dtype=torch.int64) * ulen
    snapshot = (1 << 56) - 1
    nq = a.queries

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    def emit(metric, seconds, **kw):
        print(json.dumps({"metric": metric, "queries_per_s": round(nq / seconds), "ms": round(seconds * 1e3, 3),
                          **shape, **kw}), flush=True)

    L, sp = lib(), _stream_ptr(None)
    for name, users in (("present", present), ("absent", absent)):
        uk = users.reshape(-1)
        keys, off, st = db.lookup_keys(uk, uoff, snapshot)
        assert int(st[0]) == 0
        t = median(lambda: L.lsbm_lookup_keys_dev(_ptr(uk), uk.numel(), _ptr(uoff), nq, snapshot, None, _ptr(keys),
                                                  keys.numel(), _ptr(off), _ptr(st), sp))
        emit("lookup_keys", t, batch=name)
        verdict, value, where = db.new_verdicts(nq, keys.device)

        def mem_probe():
            verdict.zero_()
            L.lsbm_memtable_get_dev(_ptr(mem.keys), mem.keys.numel(), _ptr(mem.key_offsets), _ptr(mem.values),
                                    mem_sel.numel(), _ptr(keys), keys.numel(), _ptr(off), nq, 0, _ptr(verdict),
                                    _ptr(value), _ptr(where), _ptr(st), sp)
        t = median(mem_probe)
        emit("memtable_get", t, batch=name, decided=int((verdict != 0).sum()))
        visible = version._visible_in_run_order()
        file, st2 = db.find_file(version.bounds, version.bound_offsets, version.run_first, version.run_flags, visible,
                                 keys, off)
        assert int(st2[0]) == 0
        nr = len(version.runs)
        t = median(lambda: L.lsbm_find_file_dev(_ptr(version.bounds), version.bounds.numel(),
                                                _ptr(version.bound_offsets), visible.numel(), _ptr(version.run_first),
                                                _ptr(version.run_flags), _ptr(visible), nr, _ptr(keys), keys.numel(),
                                                _ptr(off), nq, _ptr(file), _ptr(st2), sp))
        emit("find_file", t, batch=name, candidates=int((file >= 0).sum()))
        # one whole Get with the first round's save_value and the largest gather captured
        kept = {}
        real_save, real_gather = db.save_value, db.slices_gather

        def save(*args, **kw):
            kept.setdefault("save", args)
            return real_save(*args, **kw)

        def gather(image, slices, where_, lo, hi, out, out_offsets, **kw):
            count = int(((where_ >= lo) & (where_ < hi)).sum())
            if count >= kept.get("gather_count", 0):
                kept["gather_count"], kept["gather"] = count, (image, slices, where_, lo, hi, out, out_offsets)
            return real_gather(image, slices, where_, lo, hi, out, out_offsets, **kw)

        db.save_value, db.slices_gather = save, gather
        try:
            r = version.get(uk, uoff, snapshot, [mem])
        finally:
            db.save_value, db.slices_gather = real_save, real_gather
        found = int((r.status == db.FOUND).sum())
        assert found == (nq if name == "present" else 0), (name, found)
        state, key_len, window, foff, value_in, skeys, soff, sid, _, _, _ = kept["save"]

        def save_launch():
            verdict.zero_()
            L.lsbm_save_value_dev(_ptr(state), _ptr(key_len), _ptr(window), window.numel(), _ptr(foff), _ptr(value_in),
                                  _ptr(skeys), skeys.numel(), _ptr(soff), nq, sid, _ptr(verdict), _ptr(value),
                                  _ptr(where), _ptr(st), sp)
        t = median(save_launch)
        emit("save_value", t, batch=name, decided=int((verdict != 0).sum()))
        image, slices, where_, lo, hi, out, out_offsets = kept["gather"]
        t = median(lambda: L.lsbm_slices_gather_dev(_ptr(image), image.numel(), _ptr(slices), _ptr(where_), lo, hi,
                                                    _ptr(out), out.numel(), _ptr(out_offsets), nq, _ptr(st), sp))
        emit("slices_gather", t, batch=name, copied=kept["gather_count"], value_bytes=out.numel())
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = version.get(uk, uoff, snapshot, [mem])
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        emit("get", statistics.median(times), batch=name, host_clock=True, found=found)
        if a.no_host:
            continue
        hl = host_lib()
        hkeys = np.concatenate([k.cpu().numpy() for k in host_sources])
        counts = [k.numel() // klen for k in host_sources]
        first = np.zeros(len(counts) + 1, np.uint64)
        np.cumsum(counts, out=first[1:])
        # the memtable as a run of its own, Level 0 newest first, the two levels
        order = [0] + [1 + i for i in level0_order] + list(range(5, len(counts)))
        hkeys = np.concatenate([hkeys[int(first[s]) * klen:int(first[s + 1]) * klen] for s in order])
        first = np.zeros(len(counts) + 1, np.uint64)
        np.cumsum([counts[s] for s in order], out=first[1:])
        run_first = np.array([0, 1, 2, 3, 4, 5, 9, 17], np.uint64)
        run_flags = np.array([1, 1, 1, 1, 1, 0, 0], np.uint32)
        hq = keys.cpu().numpy()
        hwhere = np.zeros(nq, np.int32)
        want = np.where(r.where.cpu().numpy() < 0, -1, r.where.cpu().numpy())
        # (the GPU's run list has Level 0's empty insertion part and each level's empty one)
        remap = {-1: -1, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 6: 5, 8: 6}
        want = np.array([remap[int(w)] for w in want], np.int32)
        for threads in (1, a.threads):
            dt = hl.get_host_lookup(hkeys.ctypes.data, klen, first.ctypes.data, len(counts), run_first.ctypes.data,
                                    run_flags.ctypes.data, 7, hq.ctypes.data, klen, nq, threads, hwhere.ctypes.data)
            assert dt >= 0 and np.array_equal(hwhere, want), "host lookups != GPU Get"
            emit("host_get", dt, batch=name, threads=threads)


if __name__ == "__main__":
    main()
