#!/usr/bin/env python3
"""MANIFEST snapshot rates on one GPU, db_bench shaped:
files with 31-byte internal keys (a 23-byte user key and the 8-byte tag),
spread over the 4 levels and types 0 and 1.

  snapshot_<n>   one WriteSnapshot record of n files (65,536 and 1,048,576)
  edits_<n>      n one-file edits as separate records (65,536)

Per shape, one JSON line per measurement, seconds and GB/s of record bytes:

  decode         lsbm_edit_decode_plan_dev + lsbm_edit_decode_emit_dev
  encode         lsbm_edit_encode_plan_dev + lsbm_edit_encode_emit_dev
  recover        manifest.recover(host_files=False) over the framed MANIFEST: log.read_records, decode, the fold,
                 with its host reads between the steps
  d2d_copy       a device-to-device copy of the record bytes
  host_decode, host_encode, host_recover
                 the reference-shaped loops on the host (tools/manifest_host.cc), one thread, which is how the
                 reference runs them

Device times are HIP events around `reps` calls after warm-up calls; each figure is the median of `rounds` such
measurements.  Recorded, not gated.
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

from bench_snappy import timed  # noqa: E402


def host_lib():
    so = os.path.join(REPO, "build", "libmanifest_host.so")
    src = os.path.join(HERE, "manifest_host.cc")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.manifest_host_decode.restype = u64
    lib.manifest_host_decode.argtypes = [vp, vp, u64, vp, vp]
    lib.manifest_host_encode.restype = u64
    lib.manifest_host_encode.argtypes = [vp] * 2 + [u64] + [vp] * 7 + [u64, vp]
    lib.manifest_host_recover.restype = u64
    lib.manifest_host_recover.argtypes = [vp, vp, u64, vp]
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def file_table(torch, mf, n):
    """n files, level by level, types alternating; keys %023d + tag."""
    user = np.char.zfill(np.arange(2 * n).astype("U23"), 23).astype("S23")
    keys = np.zeros((2 * n, 31), dtype=np.uint8)
    keys[:, :23] = np.frombuffer(user.tobytes(), dtype=np.uint8).reshape(2 * n, 23)
    keys[:, 23] = 1
    keys[:, 24] = np.arange(2 * n) & 0xFF  # (a sequence number in the tag)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    i = np.arange(n, dtype=np.int64)
    return mf.FileTable(t(i + 10), t(np.full(n, 2 << 20, dtype=np.int64) + i % 4096), t(i * 4 // n), t(i % 2),
                        t(keys.reshape(-1)), t(np.arange(2 * n + 1, dtype=np.int64) * 31))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshots", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--edits", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch

    from lsbm_amd import manifest as mf
    from lsbm_amd import write
    H = host_lib()

    def median(fn):
        return statistics.median(timed(torch, fn, a.reps) for _ in range(a.rounds))

    def host_median(fn):
        out = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            fn()
            out.append(time.perf_counter() - t0)
        return statistics.median(out)

    def emit(shape, metric, seconds, nbytes, **kw):
        print(json.dumps(dict(shape=shape, metric=metric, seconds=round(seconds, 9), record_bytes=nbytes,
                              gb_per_s=round(nbytes / seconds / 1e9, 4), **kw)), flush=True)

    shapes = [("snapshot_%d" % n, n, True) for n in a.snapshots] + [("edits_%d" % a.edits, a.edits, False)]
    for shape, n, one_record in shapes:
        table = file_table(torch, mf, n)
        if one_record:
            enc = mf.snapshot(table, next_file=n + 20, log_number=5, last_sequence=1 << 40)
            # the flat shapes snapshot() hands to the encoder, rebuilt for the timed calls
            order = torch.sort(table.types * 4 + table.levels, stable=True).indices
            items = torch.stack([torch.zeros_like(order), table.types[order], table.levels[order], table.numbers[order],
                                 table.sizes[order]], dim=1).contiguous()
            keys, offs = mf._gather_keys(table.keys, table.key_offsets, order)
            new_first = torch.tensor([0, n], dtype=torch.int64, device="cuda")
            fields = mf.decode_edits(enc.image, enc.records).fields.clone()
            fields[0, mf.CMP_OFF] = 0
            names = torch.tensor(list(mf.BYTEWISE), dtype=torch.uint8, device="cuda")
        else:
            i = torch.arange(n, device="cuda")
            items = torch.stack([i, table.types, table.levels, table.numbers, table.sizes], dim=1).contiguous()
            keys, offs, new_first = table.keys, table.key_offsets, torch.arange(n + 1, device="cuda")
            fields = torch.zeros((n, mf.FIELD_WORDS), dtype=torch.int64, device="cuda")
            fields[:, mf.HAS] = mf.HAS_NEXT_FILE | mf.HAS_LAST_SEQ | mf.HAS_LOG
            fields[:, mf.NEXT_FILE] = i + 20
            fields[:, mf.LOG] = 5
            fields[:, mf.LAST_SEQ] = i * 1000
            names = torch.zeros(1, dtype=torch.uint8, device="cuda")[:0]
            enc = mf.encode_edits(fields, names, None, new_first, items, keys, offs)
        image, records = enc.image, enc.records.contiguous()
        nbytes, n_rec = image.numel(), records.shape[0]
        span, longest = int(records[:, 1].sum()), int(records[:, 1].max())
        p = mf.decode_plan(image, records, span, longest)
        n_new, n_del, kb = p.totals.cpu().tolist()
        assert p.status.item() == 0 and n_new == n and not p.verdict.any()

        def decode():
            q = mf.decode_plan(image, records, span, longest)
            mf.decode_emit(image, records, q, n_new, n_del, kb)
        emit(shape, "decode", median(decode), nbytes, files=n, records=n_rec)
        emit(shape, "decode_plan", median(lambda: mf.decode_plan(image, records, span, longest)), nbytes)
        dele = torch.zeros((1, 4), dtype=torch.int64, device="cuda")[:0]
        del_first = torch.zeros(n_rec + 1, dtype=torch.int64, device="cuda")
        args = (fields, names, del_first, dele, new_first, items, keys, offs)
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def encode():
            q = mf.encode_plan(*args)
            mf.encode_emit(*args, q, out)
        emit(shape, "encode", median(encode), nbytes)
        assert torch.equal(out, image)
        framed = write.frame_records(image, records).log
        rec = mf.recover(framed, host_files=False)
        assert rec.ok and int(rec.live.sum()) == n, rec.status
        emit(shape, "recover", median(lambda: mf.recover(framed, host_files=False)), nbytes, log_bytes=framed.numel())
        emit(shape, "d2d_copy", median(lambda: out.copy_(image)), nbytes)
        # ---- the host loops, one thread
        h_image, h_rec = image.cpu().numpy(), records.cpu().numpy().astype(np.uint64)
        verdict, counts, numbers = np.zeros(n_rec, np.uint32), np.zeros(3, np.uint64), np.zeros(4, np.uint64)
        t = host_median(lambda: H.manifest_host_decode(ptr(h_image), ptr(h_rec), n_rec, ptr(verdict), ptr(counts)))
        assert counts.tolist() == [n_new, n_del, kb] and not verdict.any()
        emit(shape, "host_decode", t, nbytes)
        h = [x.cpu().numpy() for x in args]
        h_out, h_records = np.zeros(nbytes, np.uint8), np.zeros((n_rec, 2), np.uint64)
        t = host_median(lambda: H.manifest_host_encode(ptr(h[0]), ptr(h[1]), n_rec, ptr(h[2]), ptr(h[3]), ptr(h[4]),
                                                       ptr(h[5]), ptr(h[6]), ptr(h[7]), ptr(h_out), nbytes,
                                                       ptr(h_records)))
        assert h_out.tobytes() == h_image.tobytes()
        emit(shape, "host_encode", t, nbytes)
        live = []
        t = host_median(lambda: live.append(H.manifest_host_recover(ptr(h_image), ptr(h_rec), n_rec, ptr(numbers))))
        assert live[0] == n
        emit(shape, "host_recover", t, nbytes)


if __name__ == "__main__":
    main()
