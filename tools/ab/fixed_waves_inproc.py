#!/usr/bin/env python3
"""The fixed kernel's waves per workgroup, A/B inside ONE process (round 8):
16 waves with 4-row banks, 8 waves with 8-row banks and 4 waves with 16-row
banks (lsbm_test_fixed_waves), alternated over the same device buffer, so that
the buffer's physical placement is the same for all of them (processes differ
by 1-2 % with it: DESIGN.md section 4).

    python tools/ab/fixed_waves_inproc.py [--blocks 1048576] [--length 4096] [--seed 0x5EED0000]
        [--passes 6] [--launches 50] [--waves 16,8,4] [--default-only]

--blocks / --length / --seed default to bench.py's buffer (config 2);
config 3 is --length 65536 --seed 0x5EED0001, a 10M-block shard --blocks
10000000.  The first of --waves is the baseline.  --default-only times the
setting that LSBM_FIXED_WAVES selects (a profiler run per setting).  After a
0.5 s spin-up, --passes passes, each over every setting (the order reversed
every other pass), --launches calls a pass between HIP events.  One JSON line
per pass and setting (microseconds per call), then per setting the median, the
fastest and the slowest pass, whether its slowest pass beats the baseline's
fastest (the sets do not overlap), and whether its median is within the
baseline's own fastest-to-slowest range of the baseline's median.  Every
setting's CRCs are compared with the baseline's.
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
    p.add_argument("--passes", type=int, default=6)
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--waves", default="16,8,4")
    p.add_argument("--default-only", action="store_true")
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

    settings = [("default", -1)] if args.default_only else [(f"waves{w}", w) for w in map(int, args.waves.split(","))]

    def select(w):
        assert L.lsbm_test_fixed_waves(w) == 0

    select(settings[0][1])
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # clock spin-up
        step()
        torch.cuda.synchronize()
    ref = out.clone()
    res = {}
    for ps in range(args.passes):
        order = settings if ps % 2 == 0 else settings[::-1]
        for name, w in order:
            select(w)
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
            print(json.dumps({"pass": ps, "setting": name, "us_per_call": round(us, 2),
                              "pct_hbm": round(100 * n * B / (us / 1e6) / 8e12, 2)}), flush=True)
    select(-1)
    base = res[settings[0][0]]
    base_med, base_range = float(np.median(base)), max(base) - min(base)
    for name, _ in settings:
        v = res[name]
        med = float(np.median(v))
        print(json.dumps({"setting": name, "blocks": n, "length": B, "median_us": round(med, 2),
                          "fastest_us": round(min(v), 2), "slowest_us": round(max(v), 2),
                          "median_gain_pct": round(100 * (base_med / med - 1), 2),
                          "beats_baseline_without_overlap": bool(max(v) < min(base)),
                          "median_within_baseline_range": bool(med - base_med <= base_range),
                          "lib": os.environ.get("LSBM_LIB_PATH", "")}), flush=True)


if __name__ == "__main__":
    main()
