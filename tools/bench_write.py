#!/usr/bin/env python3
"""Batched DB::Write rates on one GPU, db_bench shaped
(SURVEY.md 3.3, 8d config 1): 1,000,000 Puts of 23-byte keys and 100-byte
values in batches of 10, no sync, keys and values resident in HBM.  Kernel
times are HIP events around `reps` calls after warm-up calls; each figure is
the median of `rounds` such measurements.  One JSON line per measurement, GB/s
of log bytes written:

  sizes, group, build, frame_plan, frame, seal   the five steps and
                 lsbm_log_seal_dev, each into outputs allocated beforehand
  d2d_copy       a device-to-device copy of the log's bytes: the ceiling
  host_path      what the library offered before for the same job, given the
                 reps on the host: log.layout_records (host clock, once), the
                 H2D copy of its image and lsbm_log_seal_dev
  frame_plan_P   frame_plan alone over records of 32,761 bytes: every record
                 ends on a block end, the adversarial input
  frame_plan_1270  frame_plan alone over 100,000 records of 1,270 bytes

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
    from lsbm_amd import engine, log, write
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

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    # one pass to size everything, outputs kept for the timed calls
    r = write.write_batches(types, keys, koff, vimg, values, bf)
    log_bytes, n_groups, n_frag = r.log.numel(), r.counts.numel(), r.headers.numel()
    shape = {"ops": n, "writers": nw, "groups": n_groups, "rep_bytes": r.reps.numel(), "log_bytes": log_bytes,
             "physical_records": n_frag, "device": torch.cuda.get_device_name(0)}
    s = write.sizes(types, koff, keys.numel(), values, vimg.numel(), bf)
    gr = write.group(batch_sum=s.batch_sum)
    b = write.build(types, keys, koff, vimg, values, bf, s.op_sum, gr.group_first, n_groups, 0, r.reps)
    p = write.frame_plan(b.records, r.reps.numel(), 0)
    out, headers = torch.empty_like(r.log), torch.empty_like(r.headers)
    steps = {
        "sizes": lambda: write.sizes(types, koff, keys.numel(), values, vimg.numel(), bf, s.op_sum, s.batch_sum),
        "group": lambda: write.group(batch_sum=s.batch_sum, group_first=gr.group_first, group_sync=gr.group_sync),
        "build": lambda: write.build(types, keys, koff, vimg, values, bf, s.op_sum, gr.group_first, n_groups, 0,
                                     r.reps, b.records, b.seq_counts),
        "frame_plan": lambda: write.frame_plan(b.records, r.reps.numel(), 0, p.frag_first, p.rec_start),
        "frame": lambda: write.frame(r.reps, b.records, 0, p.frag_first, p.rec_start, out, headers),
        "seal": lambda: log.seal_records(out, headers),
    }
    total = 0.0
    for name, fn in steps.items():
        t = median(fn)
        total += t
        print(json.dumps(dict(shape, what=name, ms=round(t * 1e3, 4), gbps=round(log_bytes / t / 1e9, 1))))
    assert torch.equal(out, r.log)
    print(json.dumps(dict(shape, what="steps_total", ms=round(total * 1e3, 4), gbps=round(log_bytes / total / 1e9, 1))))
    dst = torch.empty_like(out)
    t = median(lambda: dst.copy_(out))
    print(json.dumps(dict(shape, what="d2d_copy", ms=round(t * 1e3, 4), gbps=round(log_bytes / t / 1e9, 1))))

    if not a.no_host:
        reps_host = r.reps.cpu().numpy().tobytes()
        recs = r.records.cpu().tolist()
        payloads = [reps_host[recs[2 * i]:recs[2 * i] + recs[2 * i + 1]] for i in range(n_groups)]
        t0 = time.perf_counter()
        image, heads = log.layout_records(payloads)
        t_layout = time.perf_counter() - t0
        assert image.size == log_bytes
        pinned = torch.from_numpy(image).pin_memory()
        dimg, dheads = torch.empty_like(out), torch.from_numpy(heads).cuda()
        t_h2d = median(lambda: dimg.copy_(pinned, non_blocking=True))
        t_seal = median(lambda: log.seal_records(dimg, dheads))
        assert torch.equal(dimg, r.log)
        th = t_layout + t_h2d + t_seal
        print(json.dumps(dict(shape, what="host_path", layout_records_ms=round(t_layout * 1e3, 2),
                              h2d_ms=round(t_h2d * 1e3, 4), seal_ms=round(t_seal * 1e3, 4), ms=round(th * 1e3, 2),
                              gbps=round(log_bytes / th / 1e9, 3))))

    P = write.kBlockSize - write.kHeaderSize
    for what, length, count in (("frame_plan_P", P, 100000), ("frame_plan_1270", 1270, 100000)):
        recs = torch.stack([torch.zeros(count, dtype=torch.int64, device="cuda"),
                            torch.full((count,), length, dtype=torch.int64, device="cuda")], 1).reshape(-1).contiguous()
        pl = write.frame_plan(recs, length, 0)
        t = median(lambda: write.frame_plan(recs, length, 0, pl.frag_first, pl.rec_start))
        print(json.dumps({"what": what, "records": count, "record_bytes": length, "ms": round(t * 1e3, 4),
                          "records_per_s": round(count / t), "end_offset": int(pl.rec_start[-1].item())}))


if __name__ == "__main__":
    main()
