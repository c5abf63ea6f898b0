#!/usr/bin/env python3
"""Batched log::Reader rates on one GPU, on the log
tools/bench_write.py writes: 1,000,000 db_bench Puts (23-byte keys, 100-byte
values) in batches of 10, about 126 MB, resident in HBM.  Kernel times are HIP
events around `reps` calls after warm-up calls; each figure is the median of
`rounds` such measurements.  One JSON line per measurement, GB/s of log bytes,
for the clean log, for one with a flipped payload byte in every 64th block, and
for two logs of unfragmented records (99,000 of 1,270 bytes; 2,000,000 empty):

  walk_count, walk_list   lsbm_log_read_walk_dev without and with the header list
  verify                  lsbm_log_verify_dev over the walk's headers
  plan, emit              lsbm_log_read_plan_dev, lsbm_log_read_emit_dev
  steps_total             walk_count + walk_list + verify + plan + emit
  read_records            log.read_records end to end (host clock: its two
                          device -> host reads and its allocations included)
  stream_read             a plain read of the same bytes: the walk's ceiling
  host_path               what the library offered before, on the clean log:
                          memtable.log_records of the host image (host clock:
                          the Python framing walk, the fragment list, the H2D
                          copy, lsbm_log_verify_dev and lsbm_gather_dev)

Recorded, not gated.
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
sys.path.insert(0, HERE)

from bench_snappy import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--key-bytes", type=int, default=23)
    ap.add_argument("--value-bytes", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    from lsbm_amd import engine, log, memtable, write
    engine.init(0)
    n, nw = a.ops, (a.ops + a.batch - 1) // a.batch
    g = torch.Generator(device="cuda").manual_seed(7)
    keys = torch.randint(0, 256, (n * a.key_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    vimg = torch.randint(0, 256, (n * a.value_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    koff = torch.arange(n + 1, dtype=torch.int64, device="cuda") * a.key_bytes
    values = torch.stack([torch.arange(n, dtype=torch.int64, device="cuda") * a.value_bytes,
                          torch.full((n,), a.value_bytes, dtype=torch.int64, device="cuda")], 1).reshape(-1).contiguous()
    types = torch.ones(n, dtype=torch.uint8, device="cuda")
    bf = (torch.arange(nw + 1, dtype=torch.int64, device="cuda") * a.batch).clamp(max=n)
    clean = write.write_batches(types, keys, koff, vimg, values, bf).log
    nbytes = clean.numel()
    flipped = clean.clone()
    at = torch.arange(40, nbytes, 64 * log.kBlockSize, device="cuda")  # inside the first record's payload of a block
    flipped[at] ^= 0x10

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    sink = torch.zeros(1, dtype=torch.int32, device="cuda")
    t_read = median(lambda: engine.stream_read(clean, sink))
    # the same bytes as 99,000 records of 1,270 (25 headers a block, db_bench without the group rule), and 2,000,000
    # empty records (4,681 headers a block: the longest walk a block can have)
    cut = torch.arange(99000, dtype=torch.int64, device="cuda") * 1270
    short = write.frame_records(clean, torch.stack([cut, torch.full_like(cut, 1270)], 1).reshape(-1).contiguous()).log
    empty = write.frame_records(clean, torch.zeros(4000000, dtype=torch.int64, device="cuda")).log
    for what, image in (("clean", clean), ("flipped", flipped), ("short_records", short), ("empty_records", empty)):
        nbytes = image.numel()
        r = log.read_records(image)
        nh = int(log.walk(image, 0, nbytes).n_headers.cpu()[0])
        w = log.walk(image, 0, nbytes, headers_cap=nh)
        ok, _ = log.verify_records(image, w.headers)
        p = log.plan(image, 0, nbytes, 0, w.block_first, w.block_end, w.headers, ok)
        n_rec, n_ev, side, _ = p.totals.cpu().tolist()
        out = torch.empty(nbytes + side, dtype=torch.uint8, device="cuda")
        out[:nbytes] = image
        shape = {"log": what, "log_bytes": nbytes, "headers": nh, "records": n_rec, "events": n_ev, "side_bytes": side,
                 "device": torch.cuda.get_device_name(0)}
        assert n_rec == r.records.numel() // 2 and n_ev == r.events.numel() // 4
        steps = {
            "walk_count": lambda: log.walk(image, 0, nbytes),
            "walk_list": lambda: log.walk(image, 0, nbytes, headers_cap=nh),
            "verify": lambda: log.verify_records(image, w.headers),
            "plan": lambda: log.plan(image, 0, nbytes, 0, w.block_first, w.block_end, w.headers, ok),
            "emit": lambda: log.emit(out, 0, nbytes, 0, p, nbytes, side, n_rec, n_ev),
        }
        total = 0.0
        for name, fn in steps.items():
            t = median(fn)
            total += t
            print(json.dumps(dict(shape, what=name, ms=round(t * 1e3, 4), gbps=round(nbytes / t / 1e9, 1),
                                  of_stream_read=round(nbytes / t / (clean.numel() / t_read), 3))), flush=True)
        print(json.dumps(dict(shape, what="steps_total", ms=round(total * 1e3, 4), gbps=round(nbytes / total / 1e9, 1))),
              flush=True)
        ts = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            log.read_records(image)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        print(json.dumps(dict(shape, what="read_records", ms=round(t * 1e3, 3), gbps=round(nbytes / t / 1e9, 1))),
              flush=True)
    nbytes = clean.numel()
    print(json.dumps({"what": "stream_read", "log_bytes": nbytes, "ms": round(t_read * 1e3, 4),
                      "gbps": round(nbytes / t_read / 1e9, 1)}), flush=True)
    if not a.no_host:
        host = clean.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        image, records = memtable.log_records(host)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        assert records.numel() // 2 == log.read_records(clean).records.numel() // 2
        print(json.dumps({"what": "host_path", "log_bytes": nbytes, "records": records.numel() // 2,
                          "ms": round(t * 1e3, 1), "gbps": round(nbytes / t / 1e9, 4)}), flush=True)


if __name__ == "__main__":
    main()
