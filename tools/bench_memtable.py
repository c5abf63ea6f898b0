#!/usr/bin/env python3
"""Memtable flush rates on one GPU, db_bench shaped: the
decoded entries of section 13's 262,144 data blocks (9,437,184 entries, fixed
key and value lengths; tools/dbbench_blocks.c) written as WriteBatch payloads
in a random arrival order, `--batch` entries per batch (1, and 1,000 in a
second run), resident in HBM.  Kernel times are HIP events around `reps`
launches after warm-up launches; each figure is the median of `rounds` such
measurements.  One JSON line per measurement, entries/s:

  wb_scan        lsbm_wb_scan_dev over every record
  wb_decode      lsbm_wb_decode_dev into the entry layout
  memtable_sort  lsbm_memtable_sort_dev: check, tile sort, merge passes, offsets
  sort_gather    lsbm_merge_gather_dev of the sorted order (the one move of key bytes)
  flush          memtable.flush end to end by the host clock (kNoCompression)
  host_insert    the reference-shaped loop on the host (tools/memtable_host.cc):
                 batch walk, MemTable::Add into an arena, skiplist insert, one
                 thread as the reference runs it
  host_sort      std::sort of the same decoded entries on `--threads` threads

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
    so = os.path.join(REPO, "build", "libmemtablehost.so")
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", so,
                        os.path.join(HERE, "memtable_host.cc")], check=True)
    lib = ctypes.CDLL(so)
    vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.memtable_host_insert.restype = ctypes.c_longlong
    lib.memtable_host_insert.argtypes = [vp, vp, u64, vp, u64]
    lib.memtable_host_sort.restype = i
    lib.memtable_host_sort.argtypes = [vp, vp, u64, vp, i]
    return lib


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return list(out)


def payloads(torch, users, vals, perm, batch, first_seq=1):
    """The WriteBatch image of the entries users[perm] / vals[perm], `batch`
    entries per record: (image uint8, records int64 pairs)."""
    n, U = users.shape
    V = vals.shape[1]
    kv, vv = varint(U), varint(V)
    esize = 1 + len(kv) + U + len(vv) + V
    ent = torch.empty((n, esize), dtype=torch.uint8, device="cuda")
    ent[:, 0] = 1  # kTypeValue
    c = 1
    for b in kv:
        ent[:, c] = b
        c += 1
    ent[:, c:c + U] = users[perm]
    c += U
    for b in vv:
        ent[:, c] = b
        c += 1
    ent[:, c:] = vals[perm]
    nrec = (n + batch - 1) // batch
    first = torch.arange(nrec, device="cuda", dtype=torch.int64) * batch
    count = torch.clamp(n - first, max=batch)
    head = torch.zeros((nrec, 12), dtype=torch.uint8, device="cuda")
    seq = first + first_seq
    for b in range(8):
        head[:, b] = ((seq >> (8 * b)) & 255).to(torch.uint8)
    for b in range(4):
        head[:, 8 + b] = ((count >> (8 * b)) & 255).to(torch.uint8)
    off = first * esize + 12 * torch.arange(nrec, device="cuda", dtype=torch.int64)
    length = 12 + count * esize
    image = torch.empty(n * esize + 12 * nrec, dtype=torch.uint8, device="cuda")
    if n % batch == 0:
        image.view(nrec, 12 + batch * esize)[:, :12] = head
        image.view(nrec, 12 + batch * esize)[:, 12:] = ent.view(nrec, batch * esize)
    else:
        full = n // batch
        body = image[:full * (12 + batch * esize)].view(full, 12 + batch * esize)
        body[:, :12] = head[:full]
        body[:, 12:] = ent[:full * batch].view(full, batch * esize)
        tail = image[full * (12 + batch * esize):]
        tail[:12] = head[full]
        tail[12:] = ent[full * batch:].reshape(-1)
    return image, torch.stack([off, length], 1).reshape(-1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    from lsbm_amd import block, engine, memtable, merge
    from lsbm_amd._lib import lib
    from lsbm_amd.engine import _ptr, _stream_ptr
    engine.init(0)
    img, offs = make_blocks(a.blocks)
    in_handles = np.stack([offs[:-1], offs[1:] - offs[:-1]], 1).astype(np.int64).reshape(-1)
    dimg, dh = torch.from_numpy(img).cuda(), torch.from_numpy(in_handles).cuda()
    keys0, koff0, values0, _, st = block.decode(dimg, dh)
    assert int(st.max()) == 0
    n = koff0.numel() - 1
    klen, vlen = int(koff0[1] - koff0[0]), int(values0[0, 1])
    assert bool(((koff0[1:] - koff0[:-1]) == klen).all()) and bool((values0[:, 1] == vlen).all()), "fixed lengths"
    users = keys0.view(n, klen)[:, :klen - 8]
    assert bool((users[1:].to(torch.int16) - users[:-1].to(torch.int16)).ne(0).any(1).all()), "distinct user keys"
    vals = dimg[(values0[:, 0:1] + torch.arange(vlen, device="cuda")).reshape(-1)].view(n, vlen)
    del dimg
    g = torch.Generator(device="cuda")
    g.manual_seed(0x3E37AB1E)
    perm = torch.randperm(n, device="cuda", generator=g)
    image, records = payloads(torch, users, vals, perm, a.batch)
    del vals
    nrec = records.numel() // 2
    shape = {"blocks": a.blocks, "entries": n, "batch": a.batch, "records": nrec, "image_bytes": image.numel(),
             "user_key_bytes": klen - 8, "value_bytes": vlen, "device": torch.cuda.get_device_name(0)}

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    def emit(metric, seconds, **kw):
        print(json.dumps({"metric": metric, "entries_per_s": round(n / seconds), "ms": round(seconds * 1e3, 3),
                          **shape, **kw}), flush=True)

    L, sp = lib(), _stream_ptr(None)
    counts, status = memtable.scan(image, records)
    assert int(status.max()) == 0 and int(counts[:, 0].sum()) == n
    t = median(lambda: L.lsbm_wb_scan_dev(_ptr(image), image.numel(), _ptr(records), nrec, _ptr(counts), _ptr(status),
                                          sp))
    emit("wb_scan", t, image_GBps=round(image.numel() / t / 1e9, 2))
    entry_base, key_base = memtable.bases(counts)
    d = memtable.decode(image, records, entry_base, key_base)
    assert int(d.status.max()) == 0 and memtable.max_sequence_of(d.max_sequence) == n
    assert bool((d.keys.view(n, klen)[:, :klen - 8] == users[perm]).all())
    t = median(lambda: L.lsbm_wb_decode_dev(_ptr(image), image.numel(), _ptr(records), nrec, _ptr(entry_base),
                                            _ptr(key_base), _ptr(d.keys), d.keys.numel(), _ptr(d.key_offsets),
                                            _ptr(d.values), n, _ptr(d.max_sequence), _ptr(d.status), sp))
    emit("wb_decode", t, image_GBps=round(image.numel() / t / 1e9, 2))
    p = memtable.sort(d.keys, d.key_offsets)
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(n, device="cuda")
    assert int(p.run_status[0]) == 0 and bool((p.source == inverse).all()), "the sort puts the entries back in order"
    scratch = torch.empty(L.lsbm_memtable_sort_scratch_bytes(n) // 8 + 1, dtype=torch.int64, device="cuda")
    t = median(lambda: L.lsbm_memtable_sort_dev(_ptr(d.keys), d.keys.numel(), _ptr(d.key_offsets), n, _ptr(p.source),
                                                _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(p.run_status),
                                                _ptr(scratch), scratch.numel() * 8, sp))
    emit("memtable_sort", t, key_GBps=round(d.keys.numel() / t / 1e9, 2))
    flat = d.values.reshape(-1).contiguous()
    out = merge.gather(d.keys, d.key_offsets, flat, p)
    assert int(out.status[0]) == 0 and bool((out.keys.view(n, klen)[:, :klen - 8] == users).all())
    t = median(lambda: L.lsbm_merge_gather_dev(_ptr(d.keys), d.keys.numel(), _ptr(d.key_offsets), _ptr(flat), n,
                                               _ptr(p.source), _ptr(p.out_key_offsets), _ptr(p.counts), _ptr(out.keys),
                                               out.keys.numel(), _ptr(out.key_offsets), _ptr(out.values), n,
                                               _ptr(out.status), sp))
    emit("sort_gather", t, key_GBps=round(d.keys.numel() / t / 1e9, 2))
    del out, scratch

    def flush_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = memtable.flush(image, records)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, f
    flush_once()
    times = []
    for _ in range(3):
        dt, f = flush_once()
        times.append(dt)
    emit("flush", statistics.median(times), table_bytes=f.image.numel(), host_clock=True)
    del f

    if a.no_host:
        return
    hl = host_lib()
    himg, hrec = image.cpu().numpy(), records.cpu().numpy().astype(np.uint64)
    want = p.source.cpu().numpy().astype(np.uint64)
    order = np.zeros(n, np.uint64)
    t0 = time.perf_counter()
    got = hl.memtable_host_insert(himg.ctypes.data, hrec.ctypes.data, nrec, order.ctypes.data, n)
    dt = time.perf_counter() - t0
    assert got == n and np.array_equal(order, want), "host skiplist != GPU sort"
    emit("host_insert", dt, threads=1)
    hk, ho = d.keys.cpu().numpy(), d.key_offsets.cpu().numpy().astype(np.uint64)
    order32 = np.zeros(n, np.uint32)
    for threads in (1, a.threads):
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            assert hl.memtable_host_sort(hk.ctypes.data, ho.ctypes.data, n, order32.ctypes.data, threads) == 0
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert np.array_equal(order32.astype(np.uint64), want), "host sort != GPU sort"
        emit("host_sort", best, threads=threads)


if __name__ == "__main__":
    main()
