#!/usr/bin/env python3
"""Batched range-scan rates on one GPU, on section 17's
workload (tools/bench_get.py): the 9,437,184 db_bench entries dealt at random
into one memtable of 1/16 of them, four overlapping Level-0 tables of 1/16
each, a level 1 of four files and a level 2 of eight, all resident in HBM.
Queries are `--queries` random present user keys k; a forward scan is
[k, end) and a reverse scan [start, k), each with limit 1, 10 and 100.  Kernel
times are HIP events around `reps` launches after warm-up launches; each figure
is the median of `rounds` such measurements.  One JSON line per measurement:

  view          Version.view once, by the host clock (read, decode, merge, plan, gather)
  plan          lsbm_dbiter_plan_dev over the merged entries
  gather        lsbm_merge_gather_dev of the live entries
  range         lsbm_dbiter_range_dev, per limit and direction
  emit          lsbm_dbiter_emit_dev, per limit and direction
  scan          SnapshotView.scan end to end by the host clock, median of 3
  host_merge    the k-way merge of the same runs on the host (tools/scan_host.cc)
  host_scan     the same queries through the DBIter port there, 1 thread and
                `--threads` threads, over the first `--host-queries` queries

The GPU's entries (the window's first and last merged position and its count)
and status are compared with the host's, query for query.  Recorded, not gated.
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
    so = os.path.join(REPO, "build", "libscanhost.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(HERE, "scan_host.cc")], check=True)
    lib = ctypes.CDLL(so)
    vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.scan_host_open.restype = vp
    lib.scan_host_open.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.scan_host_entries.restype = u64
    lib.scan_host_entries.argtypes = [vp]
    lib.scan_host_close.argtypes = [vp]
    lib.scan_host_scan.restype = ctypes.c_double
    lib.scan_host_scan.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, u64, u64, i, i, vp, vp, vp, vp]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--host-queries", type=int, default=None, help="queries the host answers (default: all)")
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
    # the deal of tools/bench_get.py: source 0 the memtable, 1-4 Level 0, 5 level 1, 6 level 2
    draw = torch.randint(0, 16, (n,), device="cuda", generator=g)
    source = torch.where(draw < 5, draw, torch.where(draw < 9, torch.full_like(draw, 5), torch.full_like(draw, 6)))

    def part(sel):
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
    run_keys, level0, levels = {}, [], []
    for s in range(1, 5):
        f, keys = table((source == s).nonzero().reshape(-1), 100 + s)
        level0.append(f)
        run_keys[f.number] = [keys]
    for s, pieces in ((5, 4), (6, 8)):
        sel = (source == s).nonzero().reshape(-1)
        files, held = [], []
        for p in range(pieces):
            f, keys = table(sel[sel.numel() * p // pieces:sel.numel() * (p + 1) // pieces], 10 * s + p)
            files.append(f)
            held.append(keys)
        levels.append((files, []))
        run_keys[files[0].number] = held
    version = db.Version.for_levels(level0, [], levels)
    snapshot = (1 << 56) - 1
    nq = a.queries
    shape = {"blocks": a.blocks, "entries": n, "queries": nq, "memtable_entries": mem_sel.numel(),
             "files": len(version.files), "user_key_bytes": ulen, "device": torch.cuda.get_device_name(0)}

    def emit(metric, seconds, per=None, **kw):
        print(json.dumps({"metric": metric, "per_s": round((per or nq) / seconds), "ms": round(seconds * 1e3, 3),
                          **shape, **kw}), flush=True)

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    view = version.view(snapshot, [mem], runs=version.scan_runs())
    torch.cuda.synchronize()
    emit("view", time.perf_counter() - t0, per=n, host_clock=True, n_yield=view.n_yield)
    assert view.n == n and view.n_yield == n  # (every db_bench key is distinct and a value)
    L, sp = lib(), _stream_ptr(None)
    p = view.plan
    scratch = torch.empty((L.lsbm_dbiter_scratch_bytes(n) + 7) // 8, dtype=torch.int64, device="cuda")
    t = median(lambda: L.lsbm_dbiter_plan_dev(_ptr(view.keys), view.keys.numel(), _ptr(view.key_offsets), n, snapshot,
                                              _ptr(p.source), _ptr(p.out_key_offsets), _ptr(p.counts),
                                              _ptr(p.yield_rank), _ptr(p.corrupt_rank), _ptr(p.first), _ptr(p.back),
                                              _ptr(p.status), _ptr(scratch), scratch.numel() * 8, sp))
    emit("plan", t, per=n, key_bytes=view.keys.numel())
    vals = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    gk, go, gv = torch.empty_like(view.keys), torch.empty_like(view.key_offsets), torch.empty_like(vals)
    gst = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = median(lambda: L.lsbm_merge_gather_dev(_ptr(view.keys), view.keys.numel(), _ptr(view.key_offsets), _ptr(vals),
                                               n, _ptr(p.source), _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(gk),
                                               gk.numel(), _ptr(go), _ptr(gv), n, _ptr(gst), sp))
    emit("gather", t, per=n)
    pick = torch.randint(0, n, (nq,), device="cuda", generator=g)
    users = rows[pick][:, :ulen].contiguous().reshape(-1)
    uoff = torch.arange(nq + 1, device="cuda", dtype=torch.int64) * ulen
    hosted = None
    if not a.no_host:
        hl = host_lib()
        # the runs as AddIterators lists them: the memtable, Level 0 newest first, then the levels
        order = [mk] + [k for num in sorted((f.number for f in level0), reverse=True) for k in run_keys[num]]
        firsts = [0, mem_sel.numel()]
        for num in sorted((f.number for f in level0), reverse=True):
            firsts.append(firsts[-1] + run_keys[num][0].numel() // klen)
        for files, _ in levels:
            order += run_keys[files[0].number]
            firsts.append(firsts[-1] + sum(k.numel() // klen for k in run_keys[files[0].number]))
        hkeys = np.concatenate([k.cpu().numpy() for k in order])
        hoff = np.arange(n + 1, dtype=np.uint64) * klen
        run_first = np.array(firsts, dtype=np.uint64)
        secs = ctypes.c_double(0)
        store = hl.scan_host_open(hkeys.ctypes.data, hoff.ctypes.data, n, run_first.ctypes.data, len(firsts) - 1,
                                  ctypes.byref(secs))
        assert hl.scan_host_entries(store) == n
        emit("host_merge", secs.value, per=n, runs=len(firsts) - 1)
        hq = min(nq, a.host_queries or nq)
        husers, huoff = users.cpu().numpy(), uoff.cpu().numpy().astype(np.uint64)
        hosted = (hl, store, hq, husers, huoff)
    for reverse in (False, True):
        for limit in (1, 10, 100):
            kw = {"hi": users, "hi_offsets": uoff} if reverse else {"lo": users, "lo_offsets": uoff}
            args = (users, uoff, None, None) if not reverse else (None, None, users, uoff)
            r = view.range(*args, limit=limit, reverse=reverse)
            assert int(r.call_status[0]) == 0
            # the raw launch, with the arguments SnapshotView.range passes
            zero_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
            none_p = torch.zeros(nq, dtype=torch.uint8, device="cuda")
            lo_args = (_ptr(users), users.numel(), _ptr(uoff), None) if not reverse else \
                (_ptr(users[:0]), 0, _ptr(zero_off), _ptr(none_p))
            hi_args = (None, 0, None, None) if not reverse else (_ptr(users), users.numel(), _ptr(uoff), None)
            t = median(lambda: L.lsbm_dbiter_range_dev(
                _ptr(view.keys), view.keys.numel(), _ptr(view.key_offsets), n, snapshot, _ptr(p.source),
                _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(p.yield_rank), _ptr(p.corrupt_rank), _ptr(p.first),
                _ptr(p.back), _ptr(view.value_prefix), *lo_args, *hi_args, nq, limit, None, int(reverse),
                _ptr(r.j_begin), _ptr(r.count), _ptr(r.status), _ptr(r.key_bytes), _ptr(r.value_bytes),
                _ptr(r.call_status), sp))
            emit("range", t, limit=limit, reverse=reverse)
            sums = torch.zeros((3, nq + 1), dtype=torch.int64, device="cuda")
            for i, x in enumerate((r.count, r.key_bytes, r.value_bytes)):
                torch.cumsum(x, 0, out=sums[i, 1:])
            totals = sums[:, -1].cpu().tolist()
            outs = view.emit(r.j_begin, sums[0], sums[1], sums[2], reverse, totals=totals)
            assert int(outs[4][0]) == 0
            t = median(lambda: view.emit(r.j_begin, sums[0], sums[1], sums[2], reverse, out_keys=outs[0],
                                         out_key_offsets=outs[1], out_values=outs[2], out_value_offsets=outs[3]))
            emit("emit", t, per=totals[0], limit=limit, reverse=reverse, out_entries=totals[0], key_bytes=totals[1],
                 value_bytes=totals[2])
            times = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                view.scan(**kw, limit=limit, reverse=reverse)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            emit("scan", statistics.median(times), limit=limit, reverse=reverse, host_clock=True, out_entries=totals[0])
            if hosted is None:
                continue
            hl, store, hq, husers, huoff = hosted
            live = p.source.cpu().numpy()
            jb, cnt = r.j_begin.cpu().numpy()[:hq], r.count.cpu().numpy()[:hq]
            last_j = np.maximum(jb + cnt - 1, 0)
            lo_pos, hi_pos = live[np.minimum(jb, n - 1)], live[np.minimum(last_j, n - 1)]
            want_first = np.where(cnt > 0, hi_pos if reverse else lo_pos, -1)
            want_last = np.where(cnt > 0, lo_pos if reverse else hi_pos, -1)
            want_status = r.status.cpu().numpy()[:hq]
            for threads in (1, a.threads):
                hc, hs = np.zeros(hq, np.uint64), np.zeros(hq, np.uint32)
                hf, hlast = np.zeros(hq, np.int64), np.zeros(hq, np.int64)
                none = ctypes.c_void_p(None)
                b = (husers.ctypes.data, huoff.ctypes.data, none)
                lo_h, hi_h = ((none, none, none), b) if reverse else (b, (none, none, none))
                dt = hl.scan_host_scan(store, snapshot, *lo_h, *hi_h, hq, limit, int(reverse), threads,
                                       hc.ctypes.data, hs.ctypes.data, hf.ctypes.data, hlast.ctypes.data)
                assert np.array_equal(hc, cnt.astype(np.uint64)) and np.array_equal(hs, want_status.astype(np.uint32)) \
                    and np.array_equal(hf, want_first) and np.array_equal(hlast, want_last), "host scan != GPU scan"
                emit("host_scan", dt, per=hq, limit=limit, reverse=reverse, threads=threads, host_queries=hq)
    if hosted is not None:
        hosted[0].scan_host_close(hosted[1])


if __name__ == "__main__":
    main()
