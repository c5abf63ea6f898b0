#!/usr/bin/env python3
"""Block builder rates on one GPU, db_bench shaped: the
entries of ~4,118-B data blocks as db_bench's fill workload writes them
(36 entries per block, 31-byte internal keys, 100-byte values, restart interval
16; tools/dbbench_blocks.c), decoded on the device by lsbm_block_decode_dev and
resident in HBM.  Every block of the batch is distinct (262,144 blocks, 1.08 GB
of output by default: well past the 256 MB Infinity Cache), cut into tables of
512 blocks (a 2 MB table file).  Kernel times are HIP events around `reps`
launches after warm-up launches; each figure is the median of `rounds` such
measurements.  One JSON line per measurement, GB/s of block bytes written:

  block_plan     lsbm_block_plan_dev over the entries (GB/s of the blocks it sizes)
  block_build    lsbm_block_build_dev into a laid-out image
  index_build    lsbm_index_block_build_dev, one index block per table (its own bytes)
  d2d_copy       a device-to-device copy of the built image: the ceiling
  host_build     the reference's Add / Finish loop on the host, 16 threads
                 (tools/block_build_host.c), same entries, same output

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
    so = os.path.join(REPO, "build", "libblockbuild.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(HERE, "block_build_host.c")], check=True)
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.block_build_host.restype = ctypes.c_int
    lib.block_build_host.argtypes = [vp, vp, vp, vp, vp, u64, ctypes.c_uint32, vp, vp, vp, ctypes.c_int]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--table-blocks", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    from lsbm_amd import block, block_build, engine, table
    from lsbm_amd._lib import lib
    from lsbm_amd.engine import _ptr, _stream_ptr
    engine.init(0)
    img, offs = make_blocks(a.blocks)
    in_handles = np.stack([offs[:-1], offs[1:] - offs[:-1]], 1).astype(np.int64).reshape(-1)
    dimg, dh = torch.from_numpy(img).cuda(), torch.from_numpy(in_handles).cuda()
    # the entries, as the reader leaves them in HBM
    keys, koff, values, ebase, st = block.decode(dimg, dh)
    assert int(st.max()) == 0
    values = values.reshape(-1).contiguous()
    n = koff.numel() - 1
    tables = (a.blocks + a.table_blocks - 1) // a.table_blocks
    tf = ebase[(torch.arange(tables + 1, device="cuda") * a.table_blocks).clamp(max=a.blocks)].contiguous()
    shape = {"blocks": a.blocks, "entries": n, "tables": tables, "device": torch.cuda.get_device_name(0)}

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    def emit(metric, nbytes, seconds, **kw):
        print(json.dumps({"metric": metric, "value": round(nbytes / seconds / 1e9, 2), "unit": "GB/s",
                          "kernel_ms": round(seconds * 1e3, 4), "bytes": int(nbytes), **shape, **kw}), flush=True)

    L, sp = lib(), _stream_ptr(None)
    # plan (outputs and scratch allocated once; the wrapper's allocations stay out of the timing)
    p = block_build.plan(keys, koff, values, tf, 4096, 16, blocks_cap=a.blocks)
    assert int(p.status.max()) == 0 and int(p.table_block_first[-1]) == a.blocks
    assert bool((p.block_first == ebase).all()), "the plan cuts where db_bench's builder did"
    sizes = p.block_bytes.cpu().numpy()
    assert np.array_equal(sizes, in_handles[1::2])
    nbytes = int(sizes.sum())
    scratch = torch.empty(L.lsbm_block_plan_scratch_bytes(n, tables) // 8 + 1, dtype=torch.int64, device="cuda")
    t = median(lambda: L.lsbm_block_plan_dev(_ptr(keys), keys.numel(), _ptr(koff), _ptr(values), n, _ptr(tf), tables,
                                             4096, 16, _ptr(p.block_first), _ptr(p.block_bytes), a.blocks,
                                             _ptr(p.table_block_first), _ptr(p.status), _ptr(scratch),
                                             scratch.numel() * 8, sp))
    emit("block_plan", nbytes, t)

    # build into the laid-out image (blocks back to back with their trailers' gaps)
    handles, total = table.layout_blocks(sizes)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_handles = torch.from_numpy(handles).cuda()
    built, bst = block_build.build(keys, koff, values, dimg, p.block_first, out, d_handles, 16)
    assert int(bst.max()) == 0 and bool((built == p.block_bytes).all())
    # the builder's blocks are the ones the entries were decoded from (a sample; the host's
    # loop below is compared with the whole image)
    gout = out.cpu().numpy()
    for b in np.random.default_rng(5).integers(0, a.blocks, size=4096):
        o = int(handles[2 * b])
        assert np.array_equal(gout[o:o + int(sizes[b])], img[int(offs[b]):int(offs[b + 1])]), int(b)
    t = median(lambda: L.lsbm_block_build_dev(_ptr(keys), keys.numel(), _ptr(koff), _ptr(values), _ptr(dimg),
                                              dimg.numel(), n, _ptr(p.block_first), a.blocks, 16, _ptr(out),
                                              out.numel(), _ptr(d_handles), _ptr(built), _ptr(bst), sp))
    emit("block_build", nbytes, t)

    # one index block per table
    isz, ist = block_build.index_block(keys, koff, p.block_first, p.table_block_first, d_handles)
    assert int(ist.max()) == 0
    ih, itotal = table.layout_blocks(isz.cpu().numpy())
    iout = torch.zeros(itotal, dtype=torch.uint8, device="cuda")
    d_ih = torch.from_numpy(ih).cuda()
    t = median(lambda: L.lsbm_index_block_build_dev(_ptr(keys), keys.numel(), _ptr(koff), n, _ptr(p.block_first),
                                                    a.blocks, _ptr(p.table_block_first), tables, _ptr(d_handles),
                                                    block.INTERNAL_KEY, _ptr(iout), iout.numel(), _ptr(d_ih),
                                                    _ptr(isz), _ptr(ist), sp))
    assert int(ist.max()) == 0
    emit("index_build", int(isz.sum()), t)

    # the ceiling: copying the same output bytes
    dst = torch.empty_like(out)
    t = median(lambda: dst.copy_(out))
    emit("d2d_copy", total, t)

    # the host's loop over the same entries
    hl = host_lib()
    hk, ho, hv = keys.cpu().numpy(), koff.cpu().numpy(), values.cpu().numpy()
    hf, hout, hbuilt = p.block_first.cpu().numpy(), np.zeros(total, np.uint8), np.zeros(a.blocks, np.uint64)
    best = None
    for _ in range(4):  # (the first pass also faults the pages in)
        t0 = time.perf_counter()
        assert hl.block_build_host(hk.ctypes.data, ho.ctypes.data, hv.ctypes.data, img.ctypes.data, hf.ctypes.data,
                                   a.blocks, 16, hout.ctypes.data, handles.ctypes.data, hbuilt.ctypes.data,
                                   a.threads) == 0
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert np.array_equal(hbuilt.astype(np.int64), sizes)
    assert np.array_equal(hout, gout), "host loop != GPU build"
    emit("host_build", nbytes, best, threads=a.threads)


if __name__ == "__main__":
    main()
