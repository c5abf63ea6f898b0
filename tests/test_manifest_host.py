"""tools/manifest_host.cc, the host baseline of tools/bench_manifest.py (CPU):
its DecodeFrom / EncodeTo restatement against the reference's fixture through
the model, its Recover fold against the model's, and its own self-check as a
stand-alone program under AddressSanitizer and UBSan.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from golden import manifest_cases as cases
from golden import manifestmodel as mm
from test_manifest import is_bytes, load_fixture

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "manifest_host.cc")
M64 = (1 << 64) - 1

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("manifest_host") / "libmanifest_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), SRC], check=True)
    lib = ctypes.CDLL(str(so))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.manifest_host_decode.restype = u64
    lib.manifest_host_decode.argtypes = [vp, vp, u64, vp, vp]
    lib.manifest_host_reencode.restype = ctypes.c_uint32
    lib.manifest_host_reencode.argtypes = [vp, u64, vp, u64, vp]
    lib.manifest_host_encode.restype = u64
    lib.manifest_host_encode.argtypes = [vp] * 2 + [u64] + [vp] * 7 + [u64, vp]
    lib.manifest_host_recover.restype = u64
    lib.manifest_host_recover.argtypes = [vp, vp, u64, vp]
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def u8(b):
    return np.frombuffer(bytes(b) + b"\0", dtype=np.uint8).copy()


def test_host_decodes_and_reencodes_as_the_reference(host):
    _, body = load_fixture()
    for name, b in cases.records() + cases.undefined_records():
        src, out, n = u8(b), np.zeros(len(b) + 64, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
        code = host.manifest_host_reencode(ptr(src), len(b), ptr(out), out.size, ptr(n))
        want_code, e = mm.decode(b)
        assert code == want_code, name
        if code == 0:
            got = out[:int(n[0])].tobytes()
            assert got == mm.encode(e), name
            assert name not in body["records"] or is_bytes(body["records"][name]["encoded"], got), name


def test_host_encodes_as_the_reference(host):
    _, body = load_fixture()
    named = cases.edits()
    fields, names, dele, new, del_first, new_first, keys, offs = [], bytearray(), [], [], [0], [0], bytearray(), [0]
    for r, (_, e) in enumerate(named):
        f = [0] * 13
        if e["comparator"] is not None:
            f[0], f[11], f[12] = 1, len(names), len(e["comparator"])
            names += e["comparator"]
        for bit, name, w in ((2, "log_number", 2), (4, "prev_log_number", 3), (8, "next_file", 4), (16, "last_sequence", 5)):
            if e[name] is not None:
                f[0] |= bit
                f[w] = e[name]
        f[6], f[7:11] = e["write_cursor"], e["read_cursors"]
        fields.append(f)
        dele += [[r, *d] for d in e["deleted"]]  # (any order: the host keeps a set, as the reference does)
        del_first.append(len(dele))
        for t, level, number, size, a, b in e["new"]:
            new.append([r, t, level, number, size])
            keys += a
            offs.append(len(keys))
            keys += b
            offs.append(len(keys))
        new_first.append(len(new))
    arr = lambda rows, w: np.array(rows, dtype=np.uint64).reshape(-1, w)  # noqa: E731
    a = [arr(fields, 13), u8(names), arr(del_first, 1), arr(dele, 4), arr(new_first, 1), arr(new, 5), u8(keys), arr(offs, 1)]
    want = [mm.encode(e) for _, e in named]
    out, recs = np.zeros(sum(map(len, want)), dtype=np.uint8), np.zeros((len(named), 2), dtype=np.uint64)
    total = host.manifest_host_encode(ptr(a[0]), ptr(a[1]), len(named), ptr(a[2]), ptr(a[3]), ptr(a[4]), ptr(a[5]),
                                      ptr(a[6]), ptr(a[7]), ptr(out), out.size, ptr(recs))
    assert total == out.size
    for (name, _), (off, ln), w in zip(named, recs.tolist(), want):
        got = out[off:off + ln].tobytes()
        assert got == w and is_bytes(body["edits"][name], got), name


def test_host_recovers_as_the_model(host):
    for name, payloads, how in cases.manifests():
        if how is not None:
            continue
        image, recs, at = bytearray(), [], 0
        for p in payloads:
            recs.append([len(image), len(p)])
            image += p
        img, r, numbers = u8(image), np.array(recs, dtype=np.uint64).reshape(-1, 2), np.zeros(4, dtype=np.uint64)
        got = host.manifest_host_recover(ptr(img), ptr(r), len(recs), ptr(numbers))
        codes = [mm.decode(p)[0] for p in payloads]
        if any(codes):
            assert got == M64 - next(c for c in codes if c), name
            continue
        edits = [mm.decode(p)[1] for p in payloads]
        assert got == sum(len(fs) for fs in mm.live_files(edits).values()), name
        last = lambda k: next((e[k] for e in reversed(edits) if e[k] is not None), 0)  # noqa: E731
        assert numbers.tolist() == [last("log_number"), last("prev_log_number"), last("next_file"),
                                    last("last_sequence")], name


def test_host_self_check_under_sanitizers(tmp_path):
    exe = tmp_path / "manifest_host_check"
    built = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-DMANIFEST_HOST_MAIN", "-o", str(exe), SRC], capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr + built.stdout:
        pytest.skip("no sanitizer runtime for g++")
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "manifest_host self-check ok" in run.stdout, run.stdout + run.stderr
