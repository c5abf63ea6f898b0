#!/usr/bin/env python3
"""Block reader rates on one GPU, db_bench shaped:
~4,118-B data blocks as db_bench's fill workload writes them (BlockBuilder
layout, restart interval 16, internal keys, 100-byte values;
tools/dbbench_blocks.c).  Every block of the batch is distinct (262,144 blocks,
1.08 GB by default: well past the 256 MB Infinity Cache), built on the host and
copied to HBM before timing.  Kernel times are HIP events around `reps`
launches after warm-up launches; each figure is the median of `rounds` such
measurements.  One JSON line per measurement:

  block_scan     lsbm_block_scan_dev over the batch (block GB/s)
  block_decode   lsbm_block_decode_dev with windows from a prior scan
  stream_read    lsbm_stream_read_dev over the same bytes (what reading them costs)
  host_walk      the same forward walk on the host, 16 threads (tools/block_walk_host.c)
  block_seek     lsbm_block_seek_dev, 1M lookups of present keys (M queries/s)

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


def host_walk(img, handles, threads):
    so = os.path.join(REPO, "build", "libblockwalk.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(HERE, "block_walk_host.c")], check=True)
    lib = ctypes.CDLL(so)
    lib.block_walk_host.restype = ctypes.c_int
    lib.block_walk_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                    ctypes.c_void_p]
    out = np.zeros(4, np.uint64)
    h = np.ascontiguousarray(handles, dtype=np.uint64)
    best = None
    for _ in range(4):  # (the first pass also faults the pages in)
        t0 = time.perf_counter()
        assert lib.block_walk_host(img.ctypes.data, h.ctypes.data, h.size // 2, threads, out.ctypes.data) == 0
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    from lsbm_amd import block, engine
    from lsbm_amd._lib import lib
    from lsbm_amd.engine import _ptr, _stream_ptr
    engine.init(0)
    img, offs = make_blocks(a.blocks)
    handles = np.stack([offs[:-1], offs[1:] - offs[:-1]], 1).astype(np.int64).reshape(-1)
    nbytes = int(offs[-1])
    dimg, dh = torch.from_numpy(img).cuda(), torch.from_numpy(handles).cuda()
    shape = {"blocks": a.blocks, "bytes": nbytes, "device": torch.cuda.get_device_name(0)}

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    def emit(metric, value, unit, seconds, **kw):
        print(json.dumps({"metric": metric, "value": round(value, 2), "unit": unit,
                          "kernel_ms": round(seconds * 1e3, 4), **shape, **kw}), flush=True)

    # scan (outputs allocated once; the wrapper's allocations stay out of the timing)
    counts, status = block.scan(dimg, dh)
    assert int(status.max()) == 0
    tot = counts.sum(0).cpu().tolist()
    L = lib()
    st = _stream_ptr(None)
    t = median(lambda: L.lsbm_block_scan_dev(_ptr(dimg), dimg.numel(), _ptr(dh), a.blocks, _ptr(counts),
                                             _ptr(status), st))
    emit("block_scan", nbytes / t / 1e9, "GB/s", t, entries=tot[0], key_bytes=tot[1], value_bytes=tot[2])

    # decode into preallocated outputs, windows from the scan
    keys, koff, values, ebase, dstatus = block.decode(dimg, dh)
    assert int(dstatus.max()) == 0 and int(ebase[-1]) == tot[0]
    kbase = torch.zeros(a.blocks + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(counts[:, 1], 0, out=kbase[1:])
    t = median(lambda: L.lsbm_block_decode_dev(_ptr(dimg), dimg.numel(), _ptr(dh), a.blocks, _ptr(ebase),
                                               _ptr(kbase), _ptr(keys), keys.numel(), _ptr(koff), _ptr(values),
                                               tot[0], None, _ptr(dstatus), st))
    assert int(dstatus.max()) == 0
    emit("block_decode", nbytes / t / 1e9, "GB/s", t, out_bytes=keys.numel() + 8 * koff.numel() + 8 * values.numel())

    # what reading the same bytes costs
    sink = torch.zeros(4096, dtype=torch.int32, device="cuda")
    whole = dimg[:nbytes & ~15]  # (the helper reads multiples of 16 bytes)
    t = median(lambda: engine.stream_read(whole, sink))
    emit("stream_read", whole.numel() / t / 1e9, "GB/s", t)

    # the host's walk
    t, out = host_walk(img, handles, a.threads)
    assert out.tolist() == tot + [0], (out, tot)
    emit("host_walk", nbytes / t / 1e9, "GB/s", t, threads=a.threads)

    # seek: present keys, uniformly over the entries
    rng = np.random.default_rng(3)
    hk, ho, eb = keys.cpu().numpy(), koff.cpu().numpy(), ebase.cpu().numpy()
    idx = np.sort(rng.integers(0, tot[0], size=a.queries))
    lens = ho[idx + 1] - ho[idx]
    to = np.zeros(a.queries + 1, dtype=np.int64)
    to[1:] = np.cumsum(lens)
    tk = hk[np.repeat(ho[idx] - to[:-1], lens) + np.arange(int(to[-1]))]
    qb = np.searchsorted(eb, idx, side="right") - 1
    perm = rng.permutation(a.queries)  # (lookups arrive in no order)
    qh = handles.reshape(-1, 2)[qb][perm].reshape(-1)
    pl = lens[perm]
    po = np.zeros(a.queries + 1, dtype=np.int64)
    po[1:] = np.cumsum(pl)
    pk = tk[np.repeat(to[:-1][perm] - po[:-1], pl) + np.arange(int(po[-1]))]
    dqh, dpk, dpo = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (qh, pk, po))
    r = block.seek(dimg, dqh, dpk, dpo, cmp=block.INTERNAL_KEY)
    assert int(r.state.max()) == 0 and bool((r.key_len == dpo[1:] - dpo[:-1]).all())
    t = median(lambda: L.lsbm_block_seek_dev(_ptr(dimg), dimg.numel(), _ptr(dqh), _ptr(dpk), _ptr(dpo), a.queries,
                                             block.INTERNAL_KEY, 0, _ptr(r.state), _ptr(r.pos), _ptr(r.key_len),
                                             _ptr(r.value), None, None, None, 0, st))
    emit("block_seek", a.queries / t / 1e6, "Mqueries/s", t, queries=a.queries)


if __name__ == "__main__":
    main()
