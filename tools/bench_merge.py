#!/usr/bin/env python3
"""Compaction merge rates on one GPU, db_bench shaped:
the decoded entries of section 13's 262,144 data blocks (36 entries per block,
31-byte internal keys; tools/dbbench_blocks.c), dealt by a hash of their
position into 4 sorted runs that overlap over the whole key range, resident in
HBM.  The plan runs with the drop rule on (every key is its user key's only
version, so nothing is dropped and the output is the input's size).  Kernel
times are HIP events around `reps` launches after warm-up launches; each figure
is the median of `rounds` such measurements.  One JSON line per measurement,
entries/s and GB/s of key bytes:

  merge_plan     lsbm_merge_plan_dev: check, rank, drop rule, scan, emit
  merge_gather   lsbm_merge_gather_dev: offsets, value slices and key bytes
  d2d_copy       a device-to-device copy of the key bytes: the gather's ceiling
  host_merge     the reference-shaped loop on the host (tools/merge_host.c): a
                 k-way compare-and-advance merge, the drop rule and the key
                 copy, on one thread as the reference runs it and on 16

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
    so = os.path.join(REPO, "build", "libmergehost.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(HERE, "merge_host.c")], check=True)
    lib = ctypes.CDLL(so)
    vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.merge_host.restype = i
    lib.merge_host.argtypes = [vp, vp, vp, u64, vp, u32, i, u32, u64, vp, vp, vp, vp, vp, vp, vp, i]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    from lsbm_amd import block, engine, merge
    from lsbm_amd._lib import lib
    from lsbm_amd.engine import _ptr, _stream_ptr
    engine.init(0)
    img, offs = make_blocks(a.blocks)
    in_handles = np.stack([offs[:-1], offs[1:] - offs[:-1]], 1).astype(np.int64).reshape(-1)
    dimg, dh = torch.from_numpy(img).cuda(), torch.from_numpy(in_handles).cuda()
    keys0, koff0, values0, _, st = block.decode(dimg, dh)
    assert int(st.max()) == 0
    values0 = values0.reshape(-1).contiguous()
    n = koff0.numel() - 1
    # deal the (sorted) entries into runs by a hash of their position; each run stays sorted
    run_of = ((torch.arange(n, device="cuda") * 0x9E3779B1) >> 16) % a.runs
    perm = torch.sort(run_of, stable=True).indices.contiguous()
    lens = koff0[1:] - koff0[:-1]
    dealt_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens[perm], 0, out=dealt_off[1:])
    deal = merge.PlanResult(perm, dealt_off, torch.tensor([n, keys0.numel()], dtype=torch.int64, device="cuda"), None)
    g = merge.gather(keys0, koff0, values0, deal)
    assert int(g.status[0]) == 0
    keys, koff, values = g.keys, g.key_offsets, g.values.reshape(-1).contiguous()
    run_first = torch.zeros(a.runs + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(torch.bincount(run_of, minlength=a.runs), 0, out=run_first[1:])
    nbytes = keys.numel()
    shape = {"blocks": a.blocks, "entries": n, "runs": a.runs, "key_bytes": nbytes,
             "device": torch.cuda.get_device_name(0)}

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    def emit(metric, seconds, **kw):
        print(json.dumps({"metric": metric, "entries_per_s": round(n / seconds),
                          "value": round(nbytes / seconds / 1e9, 2), "unit": "GB/s of key bytes",
                          "kernel_ms": round(seconds * 1e3, 4), **shape, **kw}), flush=True)

    L, sp = lib(), _stream_ptr(None)
    snapshot = 1 << 40
    # plan (outputs and scratch allocated once; the wrapper's allocations stay out of the timing)
    p = merge.plan(keys, koff, run_first, merge.INTERNAL_KEY, drop=True, smallest_snapshot=snapshot)
    assert int(p.run_status.max()) == 0 and p.counts.tolist() == [n, nbytes]
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(n, device="cuda")
    assert bool((p.source == inverse).all()), "the merge puts the dealt entries back in order"
    assert bool((p.out_key_offsets == koff0).all())
    scratch = torch.empty(L.lsbm_merge_scratch_bytes(n, a.runs) // 8 + 1, dtype=torch.int64, device="cuda")
    t = median(lambda: L.lsbm_merge_plan_dev(_ptr(keys), nbytes, _ptr(koff), n, _ptr(run_first), a.runs,
                                             merge.INTERNAL_KEY, merge.MERGE_DROP, snapshot, _ptr(p.source),
                                             _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(p.run_status),
                                             _ptr(scratch), scratch.numel() * 8, sp))
    emit("merge_plan", t)

    out = merge.gather(keys, koff, values, p)
    assert int(out.status[0]) == 0
    assert bool((out.keys == keys0).all()) and bool((out.key_offsets == koff0).all())
    assert bool((out.values.reshape(-1) == values0).all())
    t = median(lambda: L.lsbm_merge_gather_dev(_ptr(keys), nbytes, _ptr(koff), _ptr(values), n, _ptr(p.source),
                                               _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(out.keys), nbytes,
                                               _ptr(out.key_offsets), _ptr(out.values), n, _ptr(out.status), sp))
    emit("merge_gather", t)

    dst = torch.empty_like(keys)
    t = median(lambda: dst.copy_(keys))
    emit("d2d_copy", t)

    # the host's loop over the same arrays
    hl = host_lib()
    hk, ho, hv, hr = keys.cpu().numpy(), koff.cpu().numpy(), values.cpu().numpy(), run_first.cpu().numpy()
    order, keep = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    source, okeys = np.zeros(n, np.uint64), np.zeros(nbytes, np.uint8)
    ooff, ovals, counts = np.zeros(n + 1, np.uint64), np.zeros(2 * n, np.uint64), np.zeros(2, np.uint64)
    want = p.source.cpu().numpy().astype(np.uint64)
    for threads in (1, a.threads):
        best = None
        for _ in range(3):  # (the first pass also faults the pages in)
            t0 = time.perf_counter()
            assert hl.merge_host(hk.ctypes.data, ho.ctypes.data, hv.ctypes.data, n, hr.ctypes.data, a.runs, 1,
                                 merge.MERGE_DROP, snapshot, order.ctypes.data, keep.ctypes.data,
                                 source.ctypes.data, okeys.ctypes.data, ooff.ctypes.data, ovals.ctypes.data,
                                 counts.ctypes.data, threads) == 0
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert list(counts) == [n, nbytes] and np.array_equal(source, want), "host loop != GPU merge"
        assert np.array_equal(okeys, keys0.cpu().numpy())
        emit("host_merge", best, threads=threads)


if __name__ == "__main__":
    main()
