"""bench.py's command line: a plain run measures the headline figure only and
--dump-outputs writes what the last timed step returned, the same file from run
to run; what takes runs of its own is behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden.splitmix import stream_bytes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_dump_outputs_samples_a_large_batch_at_fixed_indices(tmp_path):
    """Above DUMP_MAX blocks the dump is a seeded sample: the same sorted,
    distinct block indices every time, each with its own CRC, float64, and both
    files together within 64 MB."""
    import torch
    import bench
    n = bench.DUMP_MAX + 12345
    vals = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)).astype(np.uint32)  # all of uint32's range
    out = torch.from_numpy(vals.view(np.int32))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, n, 0, 1)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["crc32c.npy", "crc32c_index.npy"]
    crc, idx = np.load(a / "crc32c.npy"), np.load(a / "crc32c_index.npy")
    assert crc.dtype == idx.dtype == np.float64 and crc.shape == idx.shape == (bench.DUMP_MAX,)
    assert np.array_equal(crc, np.load(b / "crc32c.npy")) and np.array_equal(idx, np.load(b / "crc32c_index.npy"))
    i = idx.astype(np.int64)
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < n
    assert np.array_equal(crc.astype(np.uint32), vals[i])
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 64 * 1000 * 1000
    # at or below DUMP_MAX: every block, in order, no index file
    bench.dump_outputs(str(tmp_path / "c"), out[:1001], 1001, 0, 1)
    assert os.listdir(tmp_path / "c") == ["crc32c.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "crc32c.npy").astype(np.uint32), vals[:1001])


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_crcs(torch_cuda, oracle, tmp_path):
    """A plain run over 4099 blocks (odd, several workgroups): the result line's
    headline fields, nothing behind --full measured, and the dumped CRCs equal
    the oracle's for every block."""
    n, steps = 4099, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--spin-s", "0", "--blocks", str(n),
                        "--dump-outputs", str(tmp_path / "dump")],
                       env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == steps and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step are one measurement, bytes of a step / time of a
    # step, each rounded for the line (ms to 4 places, GiB/s to 2)
    ms, v = line["ms_per_step"], line["value"]
    assert abs(n * 4096 / (ms / 1e3) / 2**30 - v) <= v * (0.00005 / (ms - 0.00005)) + 0.005 + 1e-9 * v
    assert line["cpu_baseline"] is None and line["host_staged"] is None and line["stream_read"] is None
    assert line["roofline"]["median_launch_ms"] is None and line["roofline"]["avg_launch_ms"] > 0
    assert os.listdir(tmp_path / "dump") == ["crc32c.npy"]
    crc = np.load(tmp_path / "dump" / "crc32c.npy")
    assert crc.dtype == np.float64 and crc.shape == (n,)
    want = oracle.batch_fixed(stream_bytes(0x5EED0000, 0, n * 4096), 4096, 4096, n)
    assert np.array_equal(crc.astype(np.uint32), want)
