#!/usr/bin/env python3
"""Table packer rates on one GPU, db_bench shaped: the
262,144 distinct ~4,118-B data blocks of sections 11 and 13 (tools/dbbench_blocks.c)
resident in HBM, and their compressed forms from snappy.compress.  Kernel times
are HIP events around `reps` launches after warm-up launches; each figure is the
median of `rounds` such measurements.  One JSON line per measurement:

  pack_plan        lsbm_block_pack_plan_dev over the blocks' two lengths (ms; GB/s
                   of the bytes it places)
  pack             lsbm_block_pack_dev under the plan's types, into the file layout
                   (gap 5): GB/s of bytes written
  pack_raw         the same with every block kept raw (no comp_len)
  d2d_copy[_raw]   a device-to-device copy of the packed image: the ceiling
  gather[_raw]     lsbm_gather_dev over the same segments: what the library had
                   for this job before
  write_table_*    sstable.write_table over one table's worth of entries with and
                   without compression (host clock around the call and a
                   synchronise: it reads sizes back between its steps)
  read_blocks      sstable.read_blocks over the sealed packed image (host clock;
                   GB/s of contents produced)

Recorded, not gated.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from bench_snappy import make_blocks, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--table-blocks", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from lsbm_amd import block, engine, snappy, sstable, table
    from lsbm_amd._lib import lib
    from lsbm_amd.engine import _ptr, _stream_ptr
    engine.init(0)
    img, offs = make_blocks(a.blocks)
    offs = offs.astype(np.int64)
    raw, d_offs = torch.from_numpy(img).cuda(), torch.from_numpy(offs).cuda()
    raw_handles = torch.stack([d_offs[:-1], d_offs[1:] - d_offs[:-1]], 1).reshape(-1).contiguous()
    raw_len = (d_offs[1:] - d_offs[:-1]).contiguous()
    comp, comp_offsets, comp_len = snappy.compress(raw, d_offs)
    comp_offsets, comp_len = comp_offsets[:-1].contiguous(), comp_len.contiguous()
    n = a.blocks
    shape = {"blocks": n, "device": torch.cuda.get_device_name(0)}

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    def wall(fn):
        def once():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        once()
        return statistics.median(once() for _ in range(a.rounds))

    def emit(metric, nbytes, seconds, **kw):
        print(json.dumps({"metric": metric, "value": round(nbytes / seconds / 1e9, 2), "unit": "GB/s",
                          "ms": round(seconds * 1e3, 4), "bytes": int(nbytes), **shape, **kw}), flush=True)

    L, sp = lib(), _stream_ptr(None)
    scratch = torch.empty(L.lsbm_block_pack_scratch_bytes(n) // 8 + 1, dtype=torch.int64, device="cuda")
    host_raw, host_comp = img, comp.cpu().numpy()
    host_coff, host_roff = comp_offsets.cpu().numpy(), offs
    both = torch.cat([raw, comp])  # lsbm_gather_dev has one source

    for label, clen in (("", comp_len), ("_raw", None)):
        types, handles, end = sstable.pack_plan(raw_len, clen)
        total = int(end[0])
        sizes = handles.view(-1, 2)[:, 1]
        nbytes = int(sizes.sum())
        kept = int(types.sum())
        if not label:
            t = median(lambda: L.lsbm_block_pack_plan_dev(_ptr(raw_len), _ptr(clen), n, 0, 5, _ptr(types),
                                                          _ptr(handles), _ptr(end), _ptr(scratch),
                                                          scratch.numel() * 8, sp))
            emit("pack_plan", nbytes, t, kept_compressed=kept)
        out = torch.zeros(total, dtype=torch.uint8, device="cuda")
        status = sstable.pack(raw, raw_handles, comp, comp_offsets, types, handles, out)
        assert int(status.max()) == 0
        # a sample of the blocks against the host's copies of the two sources
        gout, ht, hh = out.cpu().numpy(), types.cpu().numpy(), handles.cpu().numpy()
        for b in np.random.default_rng(5).integers(0, n, size=4096):
            o, s = int(hh[2 * b]), int(hh[2 * b + 1])
            src = host_comp[int(host_coff[b]):int(host_coff[b]) + s] if ht[b] else \
                host_raw[int(host_roff[b]):int(host_roff[b]) + s]
            assert np.array_equal(gout[o:o + s], src), int(b)
        t = median(lambda: L.lsbm_block_pack_dev(_ptr(raw), raw.numel(), _ptr(raw_handles), _ptr(comp), comp.numel(),
                                                 _ptr(comp_offsets), _ptr(types), _ptr(handles), n, 5, _ptr(out),
                                                 out.numel(), _ptr(status), _ptr(scratch), scratch.numel() * 8, sp))
        emit("pack" + label, nbytes, t, kept_compressed=kept, image_bytes=total)
        dst = torch.empty_like(out)
        t = median(lambda: dst.copy_(out))
        emit("d2d_copy" + label, total, t)
        # the same segments through lsbm_gather_dev
        src_off = torch.where(types != 0, comp_offsets + raw.numel(), d_offs[:-1]).contiguous()
        dst_off, seg_len = handles.view(-1, 2)[:, 0].contiguous(), sizes.contiguous()
        dst.zero_()
        L.lsbm_gather_dev(_ptr(both), _ptr(src_off), _ptr(seg_len), n, _ptr(dst), _ptr(dst_off), sp)
        hd = dst.cpu().numpy()
        for b in np.random.default_rng(6).integers(0, n, size=1024):
            o, s = int(hh[2 * b]), int(hh[2 * b + 1])
            assert np.array_equal(hd[o:o + s], gout[o:o + s]), int(b)
        t = median(lambda: L.lsbm_gather_dev(_ptr(both), _ptr(src_off), _ptr(seg_len), n, _ptr(dst), _ptr(dst_off),
                                             sp))
        emit("gather" + label, nbytes, t)
        if not label:
            # ReadBlock of every block of the sealed image
            table.seal_blocks(out, handles, types)
            contents, oh, st = sstable.read_blocks(out, handles, verify=True, max_bytes=1 << 40)
            assert int(st.max()) == 0 and contents.numel() == int(raw_len.sum())
            hc, hoh = contents.cpu().numpy(), oh.cpu().numpy()
            for b in np.random.default_rng(7).integers(0, n, size=1024):
                o, s = int(hoh[2 * b]), int(hoh[2 * b + 1])
                assert np.array_equal(hc[o:o + s], host_raw[int(host_roff[b]):int(host_roff[b + 1])]), int(b)
            del hc
            t = wall(lambda: sstable.read_blocks(out, handles, verify=True, max_bytes=1 << 40))
            emit("read_blocks", contents.numel(), t, image_bytes=total)
            del contents, oh
        del out, dst, gout

    # one table's worth of entries through the writer
    tb = min(a.table_blocks, n)
    keys, koff, values, _, st = block.decode(raw, raw_handles[:2 * tb].contiguous())
    assert int(st.max()) == 0
    values = values.reshape(-1).contiguous()
    for name, compression in (("write_table_snappy", 1), ("write_table_raw", 0)):
        image, _, _ = sstable.write_table(keys, koff, values, raw, block.INTERNAL_KEY, 4096, 16, 10, compression)
        t = wall(lambda: sstable.write_table(keys, koff, values, raw, block.INTERNAL_KEY, 4096, 16, 10, compression))
        emit(name, int(offs[tb]), t, file_bytes=image.numel(), table_blocks=tb, entries=koff.numel() - 1)


if __name__ == "__main__":
    main()
