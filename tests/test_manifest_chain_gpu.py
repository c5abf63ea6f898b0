"""The MANIFEST engine in the store's chains (GPU): tables written by
memtable.flush_many are named by manifest.snapshot / manifest_image, read back
by manifest.recover into a db.Version that answers Get as a Version built
directly does; and the reference's DB::Open opens a directory whose tables,
MANIFEST, CURRENT and log the GPU wrote (tests/golden/manifest_cases.py
directory_logs; the MANIFEST byte for byte the one the fixture maker's
directory had, which the reference opened there).
"""
import os

import numpy as np
import pytest

from golden import manifest_cases as cases
from test_db_get_gpu import _dev, dev_keys, values_of
from test_manifest import is_bytes, load_fixture
from test_manifest_gpu import i64, tobytes

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flushed_tables(torch):
    """The first two logs of the directory scenario flushed to two tables in
    one chain, and their device-resident file table at (level 0, type 0)."""
    from lsbm_amd import manifest as mf, memtable
    logs, last = cases.directory_logs()
    D = cases.DIRECTORY
    recs = logs[0] + logs[1]
    at = np.cumsum([0] + [len(r) for r in recs])
    image = _dev(torch, np.frombuffer(b"".join(recs), dtype=np.uint8))
    records = _dev(torch, np.array([[int(at[i]), len(r)] for i, r in enumerate(recs)], dtype=np.int64).reshape(-1))
    fs = memtable.flush_many(image, records, [0, len(logs[0]), len(recs)], block_size=D["block_size"],
                             restart_interval=D["restart_interval"], bits_per_key=None)
    assert len(fs) == 2
    keys, offs = dev_keys(torch, [k for f in fs for k in (bytes(f.smallest), bytes(f.largest))])
    table = mf.FileTable(i64(torch, list(D["table_numbers"])), i64(torch, [f.image.numel() for f in fs]),
                         i64(torch, [0, 0]), i64(torch, [0, 0]), keys, offs)
    return logs, last, fs, table


def test_get_over_a_recovered_version(torch_cuda):
    from lsbm_amd import db, manifest as mf
    torch = torch_cuda
    logs, last, fs, table = flushed_tables(torch)
    D = cases.DIRECTORY
    m = mf.manifest_image(table, log_number=D["log_number"], next_file=D["next_file"], last_sequence=last[1])
    rec = mf.recover(m.log)
    assert rec.status == "OK" and rec.last_sequence == last[1] and rec.log_number == D["log_number"]
    assert list(rec.files) == [(0, 0)]
    by_number = dict(zip(D["table_numbers"], fs))
    assert [(n, size) for n, size, _, _ in rec.files[(0, 0)]] == [(n, by_number[n].image.numel())
                                                                  for n in D["table_numbers"]]
    recovered = db.Version.for_levels([db.TableFile(tobytes(by_number[n].image), n, None, smallest, largest)
                                       for n, _, smallest, largest in rec.files[(0, 0)]], [], [])
    direct = db.Version.for_levels([db.TableFile(tobytes(f.image), n, None) for n, f in by_number.items()], [], [])
    assert list(zip(recovered.smallest, recovered.largest)) == list(zip(direct.smallest, direct.largest))
    users = sorted({k for recs in logs for _, k, _ in cases.directory_ops(recs)})[::2] + [b"", b"key", b"key9999"]
    queries = [(u, s) for u in users for s in (last[0] // 2, last[0], last[2] + 5)]
    uk, uoff = dev_keys(torch, [u for u, _ in queries])
    snap = _dev(torch, np.array([s for _, s in queries], dtype=np.int64))
    a, b = recovered.get(uk, uoff, snap), direct.get(uk, uoff, snap)
    assert a.status.cpu().tolist() == b.status.cpu().tolist() and a.where.cpu().tolist() == b.where.cpu().tolist()
    assert values_of(a) == values_of(b)
    # against the operations themselves: the newest operation on the key at or below the snapshot
    ops, seq = [], 1
    for recs in logs[:2]:
        for t, k, v in cases.directory_ops(recs):
            ops.append((seq, t, k, v))
            seq += 1
    status, values = a.status.cpu().tolist(), values_of(a)
    seen = set()
    for q, (u, s) in enumerate(queries):
        hit = [(sq, t, v) for sq, t, k, v in ops if k == u and sq <= s]
        want = (db.UNDECIDED, b"") if not hit else (db.FOUND, max(hit)[2]) if max(hit)[1] else (db.DELETED, b"")
        assert (status[q], values[q]) == want, (u, s)
        seen.add(want[0])
    assert seen == {db.UNDECIDED, db.FOUND, db.DELETED}


def test_the_reference_opens_a_directory_the_gpu_wrote(torch_cuda, tmp_path):
    from lsbm_amd import manifest as mf, write
    from test_ref_link import db_verify
    torch = torch_cuda
    index, _ = load_fixture()
    logs, last, fs, table = flushed_tables(torch)
    D = cases.DIRECTORY
    m = mf.manifest_image(table, log_number=D["log_number"], next_file=D["next_file"], last_sequence=last[1])
    manifest = tobytes(m.log)
    assert is_bytes(index["directory"]["manifest"], manifest)  # (holds where db_verify is absent, too)
    # the third log through DB::Write: one writer per record
    ops = [[op for op in cases.directory_ops([rec])] for rec in logs[2]]
    flat = [op for w in ops for op in w]
    keys, koff = dev_keys(torch, [k for _, k, _ in flat])
    vimage, voff = dev_keys(torch, [v for _, _, v in flat])
    values = torch.stack([voff[:-1], voff[1:] - voff[:-1]], dim=1).reshape(-1).contiguous()
    types = _dev(torch, np.array([t for t, _, _ in flat], dtype=np.uint8))
    batch_first = _dev(torch, np.cumsum([0] + [len(w) for w in ops]).astype(np.int64))
    w = write.write_batches(types, keys, koff, vimage, values, batch_first, last_sequence=last[1])
    assert w.last_sequence == last[2]
    exe = os.path.join(REPO, "oracle", "_ref", "db_verify")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/db_verify is not built")
    path = tmp_path / "db"
    path.mkdir()
    for number, f in zip(D["table_numbers"], fs):
        (path / ("%06d.ldb" % number)).write_bytes(tobytes(f.image))
    (path / ("%06d.log" % D["log_number"])).write_bytes(tobytes(w.log))
    (path / ("MANIFEST-%06d" % D["manifest_number"])).write_bytes(manifest)
    (path / "CURRENT").write_bytes(mf.current_file(D["manifest_number"]))
    rc, line = db_verify(exe, str(path), str(tmp_path / "copy"))
    assert rc == 0 and line["open_error"] == ""
    assert (line["live"], line["digest"]) == cases.directory_content(logs)
    assert (line["live"], line["digest"]) == (index["directory"]["live"], index["directory"]["digest"])
