#!/usr/bin/env python3
"""The fixed kernel's schedules across XCDs, A/B inside ONE process (round 7):
the static interleave (lsbm_test_fixed_queue(0)), the tail queue (2) with the
last T rows handed out through the cross-XCC queue, and the full queue (1),
alternated over the same device buffer, so that the buffer's physical placement
is the same for all of them.

    python tools/ab/fixed_tail_inproc.py [--blocks 1048576] [--length 4096] [--seed 0x5EED0000]
        [--pairs 6] [--launches 50] [--tails 2,4,6,8] [--full-queue] [--static-only | --default-only]

--blocks / --length / --seed default to bench.py's buffer (config 2);
config 3 is --length 65536 --seed 0x5EED0001, a 10M-block shard --blocks
10000000.  --static-only times mode 0 alone (an older library through
LSBM_LIB_PATH, which has no tail hook), --default-only the schedule that
LSBM_FIXED_QUEUE selects (a profiler run per schedule).  One JSON line per pass and schedule
(microseconds per call, HIP events around --launches calls), then per schedule
the median, the fastest and the slowest pass, and whether its slowest pass beats
the static schedule's fastest (the sets do not overlap).  Every schedule's CRCs
are compared with the static schedule's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=1 << 20)
    p.add_argument("--length", type=int, default=4096)
    p.add_argument("--seed", type=lambda v: int(v, 0), default=0x5EED0000)
    p.add_argument("--pairs", type=int, default=6)
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--tails", default="2,4,6,8", help="tail rows of the schedules to time (0: the engine's default)")
    p.add_argument("--full-queue", action="store_true")
    p.add_argument("--static-only", action="store_true")
    p.add_argument("--default-only", action="store_true")
    p.add_argument("--scratch-heads", action="store_true",
                   help="the queue's heads from per-call scratch zeroed on the stream, not the pool")
    args = p.parse_args()
    import torch
    from lsbm_amd import engine
    from lsbm_amd._lib import lib
    torch.cuda.set_device(0)
    engine.init(0)
    L = lib()
    n, B = args.blocks, args.length
    d = torch.empty(n * B, dtype=torch.uint8, device="cuda")
    engine.fill_splitmix64(d, args.seed)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    step = lambda: engine.crc32c_fixed(d, B, B, n, out=out, stream=s)

    if args.scratch_heads:
        assert L.lsbm_test_queue_pool(0) == 0
    scheds = [("default", -1, -1)] if args.default_only else [("static", 0, -1)]
    if not (args.static_only or args.default_only):
        scheds += [(f"tail{t}" if t else "tail_default", 2, t if t else -1) for t in map(int, args.tails.split(","))]
        if args.full_queue:
            scheds.append(("full", 1, -1))

    def select(mode, tail):
        assert L.lsbm_test_fixed_queue(mode) == 0
        if hasattr(L, "lsbm_test_fixed_tail"):
            assert L.lsbm_test_fixed_tail(-1, tail) == 0

    select(scheds[0][1], -1)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # clock spin-up
        step()
        torch.cuda.synchronize()
    ref = out.clone()
    res = {}
    for ps in range(args.pairs):
        order = scheds if ps % 2 == 0 else scheds[::-1]
        for name, mode, tail in order:
            select(mode, tail)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(args.launches):
                step()
            e1.record(s)
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.launches
            assert torch.equal(out, ref), name
            res.setdefault(name, []).append(us)
            print(json.dumps({"pass": ps, "schedule": name, "us_per_call": round(us, 2),
                              "pct_hbm": round(100 * n * B / (us / 1e6) / 8e12, 2)}), flush=True)
    select(-1, -1)
    base = res[scheds[0][0]]
    for name, _, _ in scheds:
        v = res[name]
        print(json.dumps({"schedule": name, "blocks": n, "length": B, "median_us": round(float(np.median(v)), 2),
                          "fastest_us": round(min(v), 2), "slowest_us": round(max(v), 2),
                          "median_gain_pct": round(100 * (float(np.median(base)) / float(np.median(v)) - 1), 2),
                          "beats_static_without_overlap": bool(max(v) < min(base)),
                          "lib": os.environ.get("LSBM_LIB_PATH", "")}), flush=True)


if __name__ == "__main__":
    main()
