#!/usr/bin/env python3
"""LSbM's buffered Get on one GPU: BufferedVersion.get over
a tree with the reference's default list lengths (common/params.cc:49-50:
compaction_buffer_length 0, 20, 20, 3; compaction_buffer_use_length 0, 20, 20, 0;
buffered_merge on), all resident in HBM.

The tree: a universe of `--universe` 16-byte user keys; every sorted table is one
file holding a random share of it (kNoCompression, 10-bit bloom, 64-byte values):
Level 0 two deletion files and an insertion file (1/32 each); level 1, 2, 3 a
deletion part (1/16), an insertion part (1/8, 1/2, all), a compaction buffer of
20, 20, 3 tables (1/16 each) under an empty head, and for levels 2 and 3 a
warm-up list of 20 tables (1/16 each).  Queries come in batches of `--queries`
random present keys and as many absent ones.

One JSON line per measurement.  Device times are HIP events around one call
after a warm-up call, the median of `--rounds`; end-to-end times are the host
clock around a synchronised call, the median of `--rounds`:

  candidates   BufferedVersion.candidates: find_file, then per slot the index Seek and the filter
  plan         lsbm_probe_plan_dev, the prefix sum, lsbm_probe_emit_dev
  get          BufferedVersion.get end to end; `rounds` is the number of rank rounds it ran
  plain_runs   the same files given to db.Version.get as plain runs, one run per slot (the route DESIGN.md
               section 17 offered; its answers may differ: a cost comparison only)
  host_get     tools/buffered_host.cc: a loop shaped like Version::Get, one thread

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
    so = os.path.join(REPO, "build", "libbufferedhost.so")
    src = os.path.join(HERE, "buffered_host.cc")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.buffered_host_get.restype = ctypes.c_double
    lib.buffered_host_get.argtypes = [vp, u64, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, i, vp, u64, vp]
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-plain", action="store_true")
    a = ap.parse_args()
    import torch
    from lsbm_amd import buffered, db, engine, sstable
    from lsbm_amd.table import kNoCompression
    engine.init(0)
    rng = np.random.default_rng(0xB0FF)
    M = a.universe
    universe = user_keys(np.arange(M, dtype=np.uint64) * 7919)
    value_image = torch.from_numpy(rng.integers(0, 256, size=64 * M, dtype=np.uint8)).cuda()
    tables = []  # (sorted ids into the universe, file bytes, smallest, largest)

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
        tables.append((ids, data, keys[0].tobytes(), keys[-1].tobytes()))
        return (number, len(data), keys[0].tobytes(), keys[-1].tobytes())

    structure = {(0, 0): [[table(1 / 32), table(1 / 32)]], (0, 1): [[table(1 / 32)]]}
    cb_length, ins_share = (0, 20, 20, 3), (0, 1 / 8, 1 / 2, 1.0)
    for level in (1, 2, 3):
        structure[(level, 0)] = [[table(1 / 16)]]
        structure[(level, 1)] = [[table(ins_share[level])]]
        structure[(level, 2)] = [[]] + [[table(1 / 16)] for _ in range(cb_length[level])]
        structure[(level, 3)] = [[]] + ([[table(1 / 16)] for _ in range(20)] if level > 1 else [])
    files = {t + 1: db.TableFile(data, t + 1, 10) for t, (_, data, _, _) in enumerate(tables)}
    use_length = (0, 20, 20, 0)
    bv = buffered.BufferedVersion(structure, files, use_length, True)
    shape = {"universe": M, "queries": a.queries, "tables": len(tables), "slots": len(bv.slots),
             "arena_bytes": bv.version.arena.numel(), "use_length": list(use_length),
             "device": torch.cuda.get_device_name(0)}
    nq = a.queries
    pick = rng.integers(0, M, size=nq)
    batches = {"present": user_keys(pick.astype(np.uint64) * 7919), "absent": user_keys(pick.astype(np.uint64) * 7919 + 1)}
    uoff = torch.arange(nq + 1, device="cuda", dtype=torch.int64) * KLEN
    snapshot = (1 << 56) - 1

    def emit(metric, seconds, **kw):
        print(json.dumps({"metric": metric, "queries_per_s": round(nq / seconds), "ms": round(seconds * 1e3, 3),
                          **shape, **kw}), flush=True)

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

    if not a.no_plain:
        flat, runs = [], []
        for s in bv.slots:
            runs.append(db.Run(list(range(len(flat), len(flat) + len(s.files))), s.flags))
            flat += [db.TableFile(tables[e[0] - 1][1], e[0], 10, e[2], e[3]) for e in s.files]
        plain = db.Version(flat, runs)
    for name, users in batches.items():
        uk = torch.from_numpy(users.reshape(-1).copy()).cuda()
        keys, offs, _ = db.lookup_keys(uk, uoff, snapshot)
        t = device_time(lambda: bv.candidates(keys, offs))
        file, cand, _, _, _ = bv.candidates(keys, offs)
        emit("candidates", t, batch=name, offered=int((file >= 0).sum()), may=int((cand == buffered.CAND_MAY).sum()))
        count, first, _, params = bv.plan(cand, keys, offs)
        total = int(first[-1].cpu())
        probe_slot = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")

        def plan():
            bv.plan(cand, keys, offs)
            buffered.probe_emit(cand.reshape(-1), bv.slot_info, *params, keys, offs, first, probe_slot, total)
        emit("plan", device_time(plan), batch=name, probes=total, max_probes=int(count.max().cpu()))
        rounds = [0]
        real_save = buffered.save_value

        def save(*args, **kw):
            rounds[0] += 1
            return real_save(*args, **kw)
        buffered.save_value = save
        try:
            r = bv.get(uk, uoff, snapshot)
        finally:
            buffered.save_value = real_save
        found = int((r.status == db.FOUND).sum())
        t = host_time(lambda: bv.get(uk, uoff, snapshot))
        emit("get", t, batch=name, host_clock=True, found=found, rounds=rounds[0])
        if not a.no_plain:
            t = host_time(lambda: plain.get(uk, uoff, snapshot))
            emit("plain_runs", t, batch=name, host_clock=True, runs=len(plain.runs),
                 found=int((plain.get(uk, uoff, snapshot).status == db.FOUND).sum()))
        if a.no_host:
            continue
        hl = host_lib()
        hkeys = np.concatenate([universe[ids] for ids, _, _, _ in tables])
        tfirst = np.zeros(len(tables) + 1, np.uint64)
        np.cumsum([len(ids) for ids, _, _, _ in tables], out=tfirst[1:])
        ids_of = lambda tabs: [t[0][0] - 1 if t else -1 for t in tabs]
        level0 = np.array([e[0] - 1 for e in sorted(structure[(0, 0)][0], key=lambda e: -e[0])] +
                          [structure[(0, 1)][0][0][0] - 1], np.int32)
        dele = np.array([-1] + [structure[(level, 0)][0][0][0] - 1 for level in (1, 2, 3)], np.int32)
        ins = np.array([-1] + [structure[(level, 1)][0][0][0] - 1 for level in (1, 2, 3)], np.int32)
        cb_lists = [[-1]] + [ids_of(structure[(level, 2)]) for level in (1, 2, 3)]
        wb_lists = [[-1]] + [ids_of(structure[(level, 3)]) for level in (1, 2, 3)]
        cb, wb = np.array(sum(cb_lists, []), np.int32), np.array(sum(wb_lists, []), np.int32)
        cb_first, wb_first = (np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
                              for lists in (cb_lists, wb_lists))
        use = np.array(use_length, np.int32)
        where = np.zeros(nq, np.int32)
        hq = np.ascontiguousarray(users)
        dt = hl.buffered_host_get(hkeys.ctypes.data, KLEN, tfirst.ctypes.data, len(tables), level0.ctypes.data,
                                  len(level0), dele.ctypes.data, ins.ctypes.data, cb.ctypes.data, cb_first.ctypes.data,
                                  wb.ctypes.data, wb_first.ctypes.data, use.ctypes.data, 1, hq.ctypes.data, nq,
                                  where.ctypes.data)
        slot_table = np.array([s.files[0][0] - 1 if s.files else -1 for s in bv.slots] + [-1], np.int32)
        # (the loop has no filter: a false positive at a gate can let the GPU, like the reference, walk the warm-up
        # list where the loop does not)
        same = float(np.mean(slot_table[r.where.cpu().numpy()] == where))
        assert same > 0.9, "host loop != GPU Get"
        emit("host_get", dt, batch=name, threads=1, same_table=round(same, 4))


if __name__ == "__main__":
    main()
