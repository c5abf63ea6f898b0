"""SSTable block builder (include/lsbm_block_build.h, lsbm_amd/block_build.py).

CPU: the plain-Python model (tests/golden/buildmodel.py) against the
reference's own TableBuilder / comparator results
(tests/golden/build_fixture.json, build_tables.bin, written by
make_build_fixture.py) and against the real db_bench table
(tests/golden/real_sst.bin); the C ABI's symbols and argument checks.
GPU: plan / build / index_block / table_build, bit-exact against the
reference's bytes and, for kernel shapes, against the model.
"""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from golden import blockmodel as bm
from golden import buildmodel as bd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
GUARD = 0xEE


def parse_table(f):
    """A table file's parts, read back through the block model."""
    f = bytes(f)
    footer = f[-48:]
    assert struct.unpack_from("<Q", footer, 40)[0] == bd.MAGIC
    a = bm.get_varint64(footer, 0, 40)
    b = bm.get_varint64(footer, a[1], 40)
    c = bm.get_varint64(footer, b[1], 40)
    d = bm.get_varint64(footer, c[1], 40)
    meta_h, index_h = (a[0], b[0]), (c[0], d[0])
    index = f[index_h[0]:index_h[0] + index_h[1]]
    st, ients = bm.walk(index)
    assert st == bm.OK
    handles = [bm.decode_handle(index[vo:vo + vl]) for _, vo, vl, _ in ients]
    blocks = [f[o:o + s] for o, s in handles]
    entries, first = [], [0]
    for blk in blocks:
        st, ents = bm.walk(blk)
        assert st == bm.OK
        entries += [(k, blk[vo:vo + vl]) for k, vo, vl, _ in ents]
        first.append(len(entries))
    return {"meta_h": meta_h, "index_h": index_h, "index": index, "index_keys": [e[0] for e in ients],
            "handles": handles, "blocks": blocks, "entries": entries, "first": first,
            "meta": f[meta_h[0]:meta_h[0] + meta_h[1]]}


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(G, "build_fixture.json")))


@pytest.fixture(scope="module")
def tables(fx):
    """[(record, file bytes, parse_table(file))]."""
    blob = open(os.path.join(G, "build_tables.bin"), "rb").read()
    out = []
    for r in fx["tables"]:
        f = blob[r["offset"]:r["offset"] + r["size"]]
        out.append((r, f, parse_table(f)))
    return out


@pytest.fixture(scope="module")
def real():
    """The 96 data blocks of the real db_bench table: (meta, image, regions, entries, first)."""
    meta = json.load(open(os.path.join(G, "real_fixture.json")))
    sst = np.fromfile(os.path.join(G, "real_sst.bin"), dtype=np.uint8)
    data = [b for b in meta["table_blocks"] if b["kind"] == "data"]
    entries, first = [], [0]
    for b in data:
        blk = sst[b["offset"]:b["offset"] + b["size"]].tobytes()
        st, ents = bm.walk(blk)
        assert st == bm.OK
        entries += [(k, blk[vo:vo + vl]) for k, vo, vl, _ in ents]
        first.append(len(entries))
    return meta, sst, data, entries, first


def real_index_entries(meta, sst):
    b = [x for x in meta["table_blocks"] if x["kind"] == "index"][0]
    blk = sst[b["offset"]:b["offset"] + b["size"]].tobytes()
    st, ents = bm.walk(blk)
    assert st == bm.OK
    return [(k, blk[vo:vo + vl]) for k, vo, vl, _ in ents]


# ---------------------------------------------------------------- CPU: the model
def test_model_reproduces_fixture_tables(tables):
    for r, f, t in tables:
        name, cmp, ri = r["name"], r["cmp"], r["restart_interval"]
        assert len(t["entries"]) == r["n_entries"], name
        first, sizes = bd.plan([(k, len(v)) for k, v in t["entries"]], r["block_size"], ri)
        assert first == (t["first"] if t["blocks"] else [0]), name
        assert sizes == [len(b) for b in t["blocks"]], name
        for b, blk in enumerate(t["blocks"]):
            assert bm.build_block(t["entries"][first[b]:first[b + 1]], ri) == blk, (name, b)
        keys = [k for k, _ in t["entries"]]
        assert bd.index_block(keys, t["first"], t["handles"], cmp) == t["index"], name
        got, handles, index_h = bd.table_file(t["entries"], cmp, r["block_size"], ri, r["bits_per_key"])
        assert got == f, name
        assert handles == t["handles"] and index_h == t["index_h"], name


def test_model_reproduces_fixture_separators(fx):
    for r in fx["separators"]:
        got = bd.separator(bytes.fromhex(r["start"]), bytes.fromhex(r["limit"]), r["cmp"])
        assert got.hex() == r["out"], r
    for r in fx["successors"]:
        assert bd.successor(bytes.fromhex(r["key"]), r["cmp"]).hex() == r["out"], r


def test_fixture_covers_the_cases(fx, tables):
    by = {r["name"]: t for r, _, t in tables}
    # the estimate exactly on block_size flushes, one byte below does not
    assert by["exact_bs256_ri16"]["first"] == [0, 1, 3, 4, 5]
    assert [len(b) for b in by["exact_bs256_ri16"]["blocks"]][:3] == [256, 260, 256]
    assert not by["empty_bytewise"]["blocks"] and len(by["empty_bytewise"]["index"]) == 8
    assert any(len(e[1]) == 16384 for e in by["edges_bs4096_ri16"]["entries"])
    assert any(len(e[0]) > 16383 for e in by["edges_bs4096_ri16"]["entries"])
    # separators are shortened inside the tables too, under both comparators
    for name in ("internal_bloom10_bs1024_ri16", "bytewise_nofilter_bs256_ri3"):
        t = by[name]
        lasts = [t["entries"][t["first"][b + 1] - 1][0] for b in range(len(t["blocks"]))]
        assert sum(len(k) < len(last) for k, last in zip(t["index_keys"], lasts)) >= 3, name
    for cmp in (0, 1):
        seps = [r for r in fx["separators"] if r["cmp"] == cmp]
        assert sum(len(r["out"]) < len(r["start"]) for r in seps) >= 10
        assert sum(r["out"] == r["start"] for r in seps) >= 10
    assert any(r["cmp"] == 1 and r["out"].endswith(bd.SEEK_TAG.hex()) and r["out"] != r["key"]
               for r in fx["successors"])


def test_model_rebuilds_real_sstable(real, oracle):
    meta, sst, data, entries, first = real
    got_first, sizes = bd.plan([(k, len(v)) for k, v in entries], 4096, 16)
    assert got_first == first and len(sizes) == 96
    off, handles = data[0]["file_offset"], []
    for b, rec in enumerate(data):
        blk = bm.build_block(entries[first[b]:first[b + 1]], 16)
        region = sst[rec["offset"]:rec["offset"] + rec["size"] + 5].tobytes()
        assert blk == region[:-5], b
        assert off == rec["file_offset"], b
        crc = oracle.mask(oracle.extend(oracle.value(blk), b"\0"))
        assert blk + b"\0" + struct.pack("<I", crc) == region, b
        assert bd.trailer(blk) == region[-5:], b
        handles.append((off, len(blk)))
        off += len(blk) + 5
    want = real_index_entries(meta, sst)
    got = bd.index_entries([k for k, _ in entries], first, handles, bm.INTERNAL_KEY)
    assert got[:95] == want[:95]
    m = [x for x in meta["table_blocks"] if x["kind"] == "metaindex"][0]
    fh = meta["filter"]["handle"]
    assert bm.build_block([(bd.FILTER_KEY, bd.encode_handle(fh[0], fh[1]))], 16) == \
        sst[m["offset"]:m["offset"] + m["size"]].tobytes()


# ---------------------------------------------------------------- CPU: the C ABI
NAMES = ["lsbm_block_build_dev", "lsbm_block_plan_dev", "lsbm_block_plan_scratch_bytes",
         "lsbm_index_block_build_dev"]


def test_block_build_symbols_exported_and_declared(product_lib):
    from lsbm_amd import _lib
    text = open(os.path.join(REPO, "include", "lsbm_block_build.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(lsbm_\w+)\s*\(", text))) == NAMES
    assert sorted(_lib.BLOCK_BUILD_SIGNATURES) == NAMES
    out = subprocess.run(["nm", "-D", "--defined-only", product_lib._name], capture_output=True,
                         text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert not [n for n in NAMES if n not in exported]
    import lsbm_amd
    from lsbm_amd import block_build
    assert "block_build" in lsbm_amd.__all__
    for fn in ("plan", "build", "index_block", "table_build"):
        assert callable(getattr(block_build, fn))


def _calls(L):
    """The three entry points on fake host pointers (a buffer of its own for
    every role, so that nothing aliases), one argument replaced at a time."""
    keep = [np.zeros(64, dtype=np.uint64) for _ in range(10)] + [np.zeros(64, dtype=np.uint8) for _ in range(3)]
    p = [x.ctypes.data for x in keep]
    kp, ip, op = p[10], p[11], p[12]

    def plan(**kw):
        return L.lsbm_block_plan_dev(kw.get("keys", kp), 8, kw.get("koff", p[0]), p[1], 1, kw.get("tf", p[2]), 1,
                                     kw.get("block_size", 4096), kw.get("ri", 16), kw.get("bf", p[3]), p[4], 1,
                                     p[5], kw.get("status", p[6]), kw.get("scratch", p[7]),
                                     kw.get("scratch_bytes", 512), None)

    def build(**kw):
        return L.lsbm_block_build_dev(kp, 8, kw.get("koff", p[0]), p[1], kw.get("image", ip), 8, 1,
                                      kw.get("bf", p[2]), 1, kw.get("ri", 16), kw.get("out", op), 8,
                                      kw.get("oh", p[3]), None, kw.get("status", p[4]), None)

    def index(**kw):
        return L.lsbm_index_block_build_dev(kp, 8, kw.get("koff", p[0]), 1, kw.get("bf", p[1]), 1, p[2], 1, p[3],
                                            kw.get("cmp", 1), kw.get("out", None), 0, kw.get("oh", None),
                                            kw.get("built", p[4]), p[5], None)
    return keep, plan, build, index


def test_block_build_entry_points_check_arguments(product_lib):
    """A bad argument is LSBM_ERR_INVALID, with or without a device; a good
    call gets past the checks (to the device, or to LSBM_ERR_NO_DEVICE)."""
    import torch
    from lsbm_amd import _lib
    L = _lib.lib()
    keep, plan, build, index = _calls(L)
    inv = _lib.LSBM_ERR_INVALID
    assert plan(keys=None) == inv
    assert plan(koff=None) == inv
    assert plan(tf=None) == inv
    assert plan(bf=None) == inv
    assert plan(status=None) == inv
    assert plan(scratch=None) == inv
    assert plan(scratch_bytes=8) == inv
    assert plan(ri=0) == inv
    assert plan(block_size=0) == inv
    assert build(koff=None) == inv
    assert build(image=None) == inv
    assert build(bf=None) == inv
    assert build(out=None) == inv
    assert build(oh=None) == inv
    assert build(status=None) == inv
    assert build(ri=0) == inv
    assert index(koff=None) == inv
    assert index(bf=None) == inv
    assert index(built=None) == inv
    assert index(cmp=2) == inv
    assert index(cmp=-1) == inv
    assert index(out=keep[12].ctypes.data, oh=None) == inv
    # outputs that alias inputs
    assert build(out=keep[11].ctypes.data) == inv
    assert build(status=keep[0].ctypes.data) == inv
    assert plan(bf=keep[0].ctypes.data) == inv
    assert index(built=keep[1].ctypes.data) == inv
    if not torch.cuda.is_available():  # (host pointers: only where no kernel can run on them)
        nd = _lib.LSBM_ERR_NO_DEVICE
        assert plan() == nd and build() == nd and index() == nd
    # nothing to do is OK before anything is looked at
    assert L.lsbm_block_build_dev(None, 0, None, None, None, 0, 0, None, 0, 16, None, 0, None, None, None,
                                  None) == _lib.LSBM_OK
    assert L.lsbm_index_block_build_dev(None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, None,
                                        None) == _lib.LSBM_OK
    assert L.lsbm_block_plan_scratch_bytes(1000, 3) >= 32 * 1000 + 16 * 3


def test_block_build_entry_points_fail_loudly_without_device(product_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    from lsbm_amd import _lib
    L = _lib.lib()
    # host pointers are not device pointers, but with no device the calls
    # must refuse before touching anything
    nd = _lib.LSBM_ERR_NO_DEVICE
    a = [np.zeros(64, dtype=np.uint64) for _ in range(10)]
    p = [x.ctypes.data for x in a]
    buf, out = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    bp, op = buf.ctypes.data, out.ctypes.data
    assert L.lsbm_block_plan_dev(bp, 8, p[0], p[1], 1, p[2], 1, 4096, 16, p[3], p[4], 1, p[5], p[6], p[7], 512,
                                 None) == nd
    assert L.lsbm_block_build_dev(bp, 8, p[0], p[1], bp, 8, 1, p[2], 1, 16, op, 8, p[3], p[4], p[5], None) == nd
    assert L.lsbm_index_block_build_dev(bp, 8, p[0], 1, p[1], 1, p[2], 1, p[3], 1, None, 0, None, p[4], p[5],
                                        None) == nd


# ---------------------------------------------------------------- GPU helpers
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Entries:
    """[(key, value)] as the device tensors lsbm_block_decode_dev would write;
    the values sit back to back in an image that starts at an odd phase."""

    def __init__(self, torch, entries, values=None, image=None):
        self.entries = entries
        keys = [k for k, _ in entries]
        koff = np.zeros(len(keys) + 1, dtype=np.int64)
        koff[1:] = np.cumsum([len(k) for k in keys])
        kb = np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy()
        if values is None:
            img, values = bytearray(b"\x5a"), []
            for _, v in entries:
                values.append([len(img), len(v)])
                img += v
            image = np.frombuffer(bytes(img), np.uint8).copy()
        self.koff_host = koff
        self.values_host = np.array(values, dtype=np.int64).reshape(-1, 2)
        self.keys, self.koff = _dev(torch, kb)[:len(kb) - 1], _dev(torch, koff)
        self.values, self.image = _dev(torch, self.values_host), _dev(torch, image)
        self.n = len(entries)


def gpu_plan(torch, E, table_first, block_size, ri, cap=None):
    from lsbm_amd import block_build
    p = block_build.plan(E.keys, E.koff, E.values, _dev(torch, np.array(table_first, dtype=np.int64)),
                         block_size, ri, blocks_cap=cap)
    return [t.cpu().numpy() for t in p]


def layout(sizes, phases=False):
    """Windows with a guard gap between them; with phases, window i starts at i mod 16."""
    handles, off = [], 7
    for i, s in enumerate(sizes):
        while phases and off % 16 != i % 16:
            off += 1
        handles += [off, s]
        off += s + 5
    return np.array(handles, dtype=np.int64), off + 9


def gpu_build(torch, E, block_first, ri, handles, total, skew=0):
    """build into a guard-filled image: (image bytes, built, status)."""
    from lsbm_amd import block_build
    big = torch.full((total + skew,), GUARD, dtype=torch.uint8, device="cuda")
    out = big[skew:]
    built, status = block_build.build(E.keys, E.koff, E.values, E.image,
                                      _dev(torch, np.array(block_first, dtype=np.int64)), out,
                                      _dev(torch, handles), ri)
    return out.cpu().numpy(), built.cpu().numpy(), status.cpu().numpy()


def check_image(img, handles, blocks, label=""):
    """Every block at its window's start, every other byte still the guard."""
    mask = np.ones(img.size, dtype=bool)
    for b, blk in enumerate(blocks):
        o = int(handles[2 * b])
        if blk is not None:
            assert img[o:o + len(blk)].tobytes() == blk, (label, b)
            mask[o:o + len(blk)] = False
        else:
            mask[o:o + int(handles[2 * b + 1])] = False  # (a failed block's window is unspecified)
    assert np.all(img[mask] == GUARD), label


def gpu_index(torch, E, block_first, tbf, data_handles, cmp, sizes_only=False):
    """(blocks' bytes per table, built, status)."""
    from lsbm_amd import block_build
    bf = _dev(torch, np.array(block_first, dtype=np.int64))
    tb = _dev(torch, np.array(tbf, dtype=np.int64))
    dh = _dev(torch, np.array(data_handles, dtype=np.int64).reshape(-1))
    built, status = block_build.index_block(E.keys, E.koff, bf, tb, dh, cmp)
    built_h = built.cpu().numpy()
    if sizes_only:
        return None, built_h, status.cpu().numpy()
    handles, total = layout([int(s) for s in built_h], phases=True)
    out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    built2, status = block_build.index_block(E.keys, E.koff, bf, tb, dh, cmp, out, _dev(torch, handles))
    assert np.array_equal(built2.cpu().numpy(), built_h)
    img = out.cpu().numpy()
    blocks = [img[int(handles[2 * t]):int(handles[2 * t]) + int(built_h[t])].tobytes() for t in range(len(tbf) - 1)]
    check_image(img, handles, blocks, "index")
    return blocks, built_h, status.cpu().numpy()


# ---------------------------------------------------------------- GPU tests
@pytest.mark.gpu
def test_gpu_fixture_plan_build_index(torch_cuda, tables):
    """1. the reference's cuts, block bytes and index blocks for every fixture table."""
    torch = torch_cuda
    for r, f, t in tables:
        name, ri = r["name"], r["restart_interval"]
        E = Entries(torch, t["entries"])
        first, sizes, tbf, status = gpu_plan(torch, E, [0, E.n], r["block_size"], ri)
        nb = len(t["blocks"])
        assert list(status) == [0] and list(tbf) == [0, nb], name
        assert list(first[:nb + 1]) == (t["first"] if nb else [0]), name
        assert list(sizes[:nb]) == [len(b) for b in t["blocks"]], name
        handles, total = layout([len(b) for b in t["blocks"]], phases=True)
        img, built, st = gpu_build(torch, E, t["first"], ri, handles, total)
        assert not st.any() and list(built) == [len(b) for b in t["blocks"]], name
        check_image(img, handles, t["blocks"], name)
        blocks, built, st = gpu_index(torch, E, t["first"], [0, nb], t["handles"], r["cmp"])
        assert list(st) == [0] and blocks == [t["index"]], name


@pytest.mark.gpu
def test_gpu_fixture_separator_pairs(torch_cuda, fx):
    """1b. every separator / successor pair as a two-block (one-block) table's index key."""
    torch = torch_cuda
    for cmp in (0, 1):
        entries, first, tbf, want = [], [0], [0], []
        for r in fx["separators"]:
            if r["cmp"] == cmp:
                entries += [(bytes.fromhex(r["start"]), b""), (bytes.fromhex(r["limit"]), b"")]
                first += [len(entries) - 1, len(entries)]
                tbf.append(len(first) - 1)
                want.append(bytes.fromhex(r["out"]))
        n_sep = len(want)
        for r in fx["successors"]:
            if r["cmp"] == cmp:
                entries.append((bytes.fromhex(r["key"]), b""))
                first.append(len(entries))
                tbf.append(len(first) - 1)
                want.append(bytes.fromhex(r["out"]))
        E = Entries(torch, entries)
        handles = [(17 * b, 300 + b) for b in range(len(first) - 1)]
        blocks, _, st = gpu_index(torch, E, first, tbf, handles, cmp)
        assert not st.any()
        for t, blk in enumerate(blocks):
            st_, ents = bm.walk(blk)
            assert st_ == bm.OK and len(ents) == (2 if t < n_sep else 1)
            assert ents[0][0] == want[t], (cmp, t)
            assert blk[ents[0][1]:ents[0][1] + ents[0][2]] == bd.encode_handle(*handles[tbf[t]])


@pytest.mark.gpu
def test_gpu_real_table(torch_cuda, real):
    """2. decode(real_sst.bin) -> plan -> build -> seal == the file's first 96 regions."""
    torch = torch_cuda
    from lsbm_amd import block, block_build, table
    meta, sst, data, entries, first = real
    dimg = _dev(torch, sst)
    dh = _dev(torch, np.array([[b["offset"], b["size"]] for b in data], dtype=np.int64).reshape(-1))
    keys, koff, values, ebase, st = block.decode(dimg, dh)
    assert not st.cpu().numpy().any()
    n = koff.numel() - 1
    p = block_build.plan(keys, koff, values.reshape(-1), _dev(torch, np.array([0, n], dtype=np.int64)), 4096, 16)
    assert p.status.cpu().tolist() == [0] and p.table_block_first.cpu().tolist() == [0, 96]
    assert p.block_first[:97].cpu().tolist() == first
    sizes = p.block_bytes[:96].cpu().numpy()
    assert list(sizes) == [b["size"] for b in data]
    handles, total = table.layout_blocks(sizes)
    assert [int(h) for h in handles[0::2]] == [b["offset"] for b in data]
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_handles = _dev(torch, handles)
    built, st = block_build.build(keys, koff, values.reshape(-1), dimg, p.block_first[:97].contiguous(), out,
                                  d_handles, 16)
    assert not st.cpu().numpy().any() and built.cpu().tolist() == list(sizes)
    table.seal_blocks(out, d_handles, torch.zeros(96, dtype=torch.uint8, device="cuda"))
    assert np.array_equal(out.cpu().numpy(), sst[:total])
    file_handles = np.array([[b["file_offset"], b["size"]] for b in data], dtype=np.int64).reshape(-1)
    isz, ist = block_build.index_block(keys, koff, p.block_first[:97].contiguous(), p.table_block_first,
                                       _dev(torch, file_handles), block.INTERNAL_KEY)
    ih = _dev(torch, np.array([0, int(isz[0])], dtype=np.int64))
    iout = torch.zeros(int(isz[0]), dtype=torch.uint8, device="cuda")
    _, ist = block_build.index_block(keys, koff, p.block_first[:97].contiguous(), p.table_block_first,
                                     _dev(torch, file_handles), block.INTERNAL_KEY, iout, ih)
    assert ist.cpu().tolist() == [0]
    blk = iout.cpu().numpy().tobytes()
    st_, ents = bm.walk(blk)
    assert st_ == bm.OK and len(ents) == 96
    got = [(k, blk[vo:vo + vl]) for k, vo, vl, _ in ents]
    assert got[:95] == real_index_entries(meta, sst)[:95]


def shaped_entries(rng, n, klo=4, khi=20, vlo=0, vhi=40):
    ks = set()
    while len(ks) < n:
        ks.add(bytes(rng.choice(b"abcd") for _ in range(rng.randint(klo, khi))))
    return [(k, bytes(rng.randrange(256) for _ in range(rng.randint(vlo, vhi)))) for k in sorted(ks)]


def sized_block(rng, target, ri):
    """Entries whose block is exactly `target` bytes at restart interval ri."""
    ents = shaped_entries(rng, 20)
    base = len(bm.build_block(ents + [(b"zzzz", b"")], ri))
    for fill in range(target - base - 4, target - base + 1):
        e = ents + [(b"zzzz", b"\x77" * fill)]
        if len(bm.build_block(e, ri)) == target:
            return e
    raise AssertionError(target)


@pytest.mark.gpu
def test_gpu_build_kernel_shapes(torch_cuda):
    """3. entry counts around the wave width, sizes around the LDS tile, a
    block far above it, every 16-B window phase, an output that is itself off
    phase -- against the model."""
    import random
    torch = torch_cuda
    from lsbm_amd import block_build
    rng = random.Random(0x5AFE)
    for ri in (1, 16):
        groups = [shaped_entries(rng, n) for n in (1, 15, 16, 17, 33, 63, 64, 65, 129)]
        groups += [sized_block(rng, s, ri) for s in (8191, 8192, 8193)]
        big = shaped_entries(rng, 2, 30, 40)
        groups += [[big[0]], shaped_entries(rng, 1200, 60, 100, 100, 140), [big[1]]]
        groups += [[]]  # Finish() of a fresh builder
        groups += [shaped_entries(rng, 3) for _ in range(8)]  # (all 16 phases)
        entries, first = [], [0]
        for g in groups:
            entries += g
            first.append(len(entries))
        want = [bm.build_block(g, ri) for g in groups]
        assert [len(w) for w in want[9:12]] == [8191, 8192, 8193] and len(want[13]) > 200000
        E = Entries(torch, entries)
        handles, total = layout([len(w) for w in want], phases=True)
        for skew in (0, 3):
            img, built, st = gpu_build(torch, E, first, ri, handles, total, skew)
            assert not st.any() and list(built) == [len(w) for w in want]
            check_image(img, handles, want, (ri, skew))
    # nothing to build
    E0 = Entries(torch, [])
    img, built, st = gpu_build(torch, E0, [0], 16, np.zeros(0, dtype=np.int64), 32)
    assert built.size == 0 and np.all(img == GUARD)
    img, built, st = gpu_build(torch, E0, [0, 0], 16, np.array([3, 8], dtype=np.int64), 32)
    assert list(built) == [8] and list(st) == [0]
    check_image(img, [3, 8], [bm.build_block([], 16)])
    assert block_build.BUILD_TOO_LARGE == 3


@pytest.mark.gpu
def test_gpu_build_value_slices(torch_cuda):
    """3. value slices at odd phases of the image, overlapping and repeated."""
    import random
    torch = torch_cuda
    rng = random.Random(0x51CE)
    image = np.frombuffer(bytes(rng.randrange(256) for _ in range(4000)), np.uint8).copy()
    keys = [k for k, _ in shaped_entries(rng, 150)]
    values = []
    for i in range(len(keys)):
        off = rng.randrange(0, 3900) if i % 5 else 1001  # (repeated: the same slice again)
        values.append([off, rng.randint(0, 100) if i % 7 else 4000 - off])
    entries = [(k, image[o:o + n].tobytes()) for k, (o, n) in zip(keys, values)]
    E = Entries(torch, entries, values, image)
    first = [0, 40, 41, 150]
    want = [bm.build_block(entries[first[b]:first[b + 1]], 16) for b in range(3)]
    handles, total = layout([len(w) for w in want])
    img, built, st = gpu_build(torch, E, first, 16, handles, total)
    assert not st.any()
    check_image(img, handles, want)


@pytest.mark.gpu
def test_gpu_plan_tables_cap_and_too_large(torch_cuda):
    """3. five tables (one empty, one with a single entry), a cap one too
    small, and a value length of 2^32 that no memory backs."""
    import random
    torch = torch_cuda
    rng = random.Random(0x9A7)
    entries = shaped_entries(rng, 700, 4, 24, 0, 90)
    tf = [0, 300, 300, 301, 650, 700]
    for bs, ri in ((256, 3), (1024, 16), (4096, 1)):
        E = Entries(torch, entries)
        want_first, want_sizes, want_tbf = [], [], [0]
        for t in range(5):
            f, s = bd.plan([(k, len(v)) for k, v in entries[tf[t]:tf[t + 1]]], bs, ri)
            want_first += [tf[t] + x for x in f[:len(s)]]
            want_sizes += s
            want_tbf.append(len(want_sizes))
        nb = len(want_sizes)
        first, sizes, tbf, status = gpu_plan(torch, E, tf, bs, ri)
        assert not status.any() and list(tbf) == want_tbf
        assert list(first[:nb + 1]) == want_first + [700] and list(sizes[:nb]) == want_sizes
        # one slot too few: the true total, and nothing past the cap
        from lsbm_amd import block_build
        cap = nb - 1
        p = block_build.plan(E.keys, E.koff, E.values, _dev(torch, np.array(tf, dtype=np.int64)), bs, ri,
                             blocks_cap=cap)
        assert p.table_block_first.cpu().tolist() == want_tbf
        assert p.block_first.numel() == cap + 1 and p.block_bytes.numel() == cap
        assert p.block_first.cpu().tolist() == want_first[:cap + 1]
        assert p.block_bytes.cpu().tolist() == want_sizes[:cap]
    # no tables, no entries
    E0 = Entries(torch, [])
    first, sizes, tbf, status = gpu_plan(torch, E0, [0], 4096, 16)
    assert list(tbf) == [0] and list(first) == [0]
    first, sizes, tbf, status = gpu_plan(torch, E0, [0, 0], 4096, 16)
    assert list(tbf) == [0, 0] and list(status) == [0]
    # plan reads lengths only: a 2^32-byte value that does not exist
    small = entries[:40]
    E = Entries(torch, small)
    vals = E.values_host.copy()
    vals[25, 1] = 1 << 32
    E.values = _dev(torch, vals)
    first, sizes, tbf, status = gpu_plan(torch, E, [0, 20, 40], 1024, 16)
    assert list(status) == [0, 3]
    f, s = bd.plan([(k, len(v)) for k, v in small[:20]], 1024, 16)
    assert list(first[:len(s)]) == f[:len(s)] and list(sizes[:len(s)]) == s and tbf[1] == len(s)


@pytest.mark.gpu
def test_gpu_build_windows_and_bad_input(torch_cuda):
    """4. verdicts on checked input: a window one byte short, a value slice one
    byte past the image, a decreasing key offset, a 7-byte internal key --
    each for exactly its block or table, the neighbours built correctly, every
    guard byte outside the windows intact."""
    import random
    torch = torch_cuda
    from lsbm_amd import block_build
    rng = random.Random(0xBAD)
    entries = shaped_entries(rng, 120, 9, 20)
    first = [0, 30, 60, 90, 120]
    want = [bm.build_block(entries[first[b]:first[b + 1]], 16) for b in range(4)]
    sizes = [len(w) for w in want]
    # a window one byte too small
    E = Entries(torch, entries)
    handles, total = layout([sizes[0], sizes[1] - 1, sizes[2], sizes[3]])
    img, built, st = gpu_build(torch, E, first, 16, handles, total)
    assert list(st) == [0, block_build.BUILD_NO_ROOM, 0, 0] and list(built) == sizes
    check_image(img, handles, [want[0], None, want[2], want[3]])
    # a value slice that ends one byte past the image
    handles, total = layout(sizes)
    E = Entries(torch, entries)
    vals = E.values_host.copy()
    vals[70] = [E.image.numel() - 4, 5]
    E.values = _dev(torch, vals)
    img, built, st = gpu_build(torch, E, first, 16, handles, total)
    assert list(st) == [0, 0, block_build.BUILD_BAD_INPUT, 0] and list(built) == [sizes[0], sizes[1], 0, sizes[3]]
    check_image(img, handles, [want[0], want[1], None, want[3]])
    assert np.all(img[int(handles[4]):int(handles[4]) + sizes[2]] == GUARD)  # nothing written for it
    # a decreasing key offset: entries 40 and 41 are bad, both in block 1
    E = Entries(torch, entries)
    koff = E.koff_host.copy()
    koff[41] = koff[40] - 1
    E.koff = _dev(torch, koff)
    img, built, st = gpu_build(torch, E, first, 16, handles, total)
    assert list(st) == [0, block_build.BUILD_BAD_INPUT, 0, 0]
    check_image(img, handles, [want[0], None, want[2], want[3]])
    first_p, _, tbf, status = gpu_plan(torch, E, [0, 30, 60, 120], 4096, 16)
    assert list(status) == [0, block_build.BUILD_BAD_INPUT, 0]
    # block_first that decreases, or passes the entries
    E = Entries(torch, entries)
    img, built, st = gpu_build(torch, E, [0, 30, 20, 90, 121], 16, handles, total)
    assert list(st) == [0, 2, block_build.BUILD_NO_ROOM, 2]  # (block 2 now holds 70 entries)
    # a 7-byte key under the internal comparator: that table's index block alone
    ents = [(k, v) for k, v in entries]
    ents[59] = (b"7 bytes", b"")
    E = Entries(torch, ents)
    dh = [(100 * b, 90) for b in range(4)]
    blocks, built, st = gpu_index(torch, E, first, [0, 1, 2, 4], dh, 1)
    assert list(st) == [0, block_build.BUILD_BAD_INPUT, 0] and built[1] == 0
    keys = [k for k, _ in ents]
    assert blocks[0] == bd.index_block(keys[:30], [0, 30], dh[:1], 1)
    assert blocks[2] == bd.index_block(keys[60:], [0, 30, 60], dh[2:], 1)
    blocks, built, st = gpu_index(torch, E, first, [0, 1, 2, 4], dh, 0)
    assert not st.any() and blocks[1] == bd.index_block(keys[30:60], [0, 30], dh[1:2], 0)
    # an index window one byte too small
    bf, tb = _dev(torch, np.array(first, dtype=np.int64)), _dev(torch, np.array([0, 4], dtype=np.int64))
    d = _dev(torch, np.array(dh, dtype=np.int64).reshape(-1))
    size, _ = block_build.index_block(E.keys, E.koff, bf, tb, d, 0)
    out = torch.full((int(size[0]) + 20,), GUARD, dtype=torch.uint8, device="cuda")
    built, st = block_build.index_block(E.keys, E.koff, bf, tb, d, 0, out,
                                        _dev(torch, np.array([5, int(size[0]) - 1], dtype=np.int64)))
    assert st.cpu().tolist() == [block_build.BUILD_NO_ROOM] and built.cpu().tolist() == size.cpu().tolist()
    o = out.cpu().numpy()
    assert np.all(o[:5] == GUARD) and np.all(o[5 + int(size[0]) - 1:] == GUARD)


@pytest.mark.gpu
def test_gpu_round_trip_through_the_reader(torch_cuda, tables):
    """5. scan / decode of the built blocks return the entries; seek finds every key."""
    torch = torch_cuda
    from lsbm_amd import block, block_build
    for name in ("internal_bloom10_bs1024_ri16", "bytewise_bs256_ri3"):
        r, f, t = [x for x in tables if x[0]["name"] == name][0]
        cmp, ri = r["cmp"], r["restart_interval"]
        E = Entries(torch, t["entries"])
        p = block_build.plan(E.keys, E.koff, E.values, _dev(torch, np.array([0, E.n], dtype=np.int64)),
                             r["block_size"], ri)
        nb = int(p.table_block_first[-1])
        handles, total = layout([int(s) for s in p.block_bytes[:nb].cpu()], phases=True)
        out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
        dh = _dev(torch, handles)
        first = p.block_first[:nb + 1].contiguous()
        _, st = block_build.build(E.keys, E.koff, E.values, E.image, first, out, dh, ri)
        assert not st.cpu().numpy().any()
        counts, st = block.scan(out, dh)
        assert not st.cpu().numpy().any()
        assert counts[:, 0].cpu().tolist() == [t["first"][b + 1] - t["first"][b] for b in range(nb)]
        keys, koff, values, ebase, st = block.decode(out, dh)
        assert not st.cpu().numpy().any()
        keys, koff, values, img = keys.cpu().numpy(), koff.cpu().numpy(), values.cpu().numpy(), out.cpu().numpy()
        got = [(keys[int(koff[e]):int(koff[e + 1])].tobytes(),
                img[int(values[e, 0]):int(values[e, 0]) + int(values[e, 1])].tobytes()) for e in range(E.n)]
        assert got == t["entries"]
        # Seek(key e) in its block finds entry e
        block_of = np.repeat(np.arange(nb), np.diff(t["first"]))
        qh = _dev(torch, handles.reshape(-1, 2)[block_of].reshape(-1))
        res = block.seek(out, qh, E.keys, E.koff, cmp=cmp)
        assert not res.state.cpu().numpy().any()
        assert res.key_len.cpu().tolist() == [len(k) for k, _ in t["entries"]]
        assert np.array_equal(res.value.cpu().numpy(), values)


@pytest.mark.gpu
def test_gpu_table_build_whole_files(torch_cuda, tables):
    """6. table_build == the reference's table files, byte for byte; table_get
    over the built image finds every key."""
    torch = torch_cuda
    from lsbm_amd import block, block_build
    whole = ("internal_bloom10_bs1024_ri16", "bytewise_nofilter_bs256_ri3", "one_entry_internal_bloom10",
             "one_entry_bytewise", "empty_internal_bloom10", "empty_bytewise", "edges_bs4096_ri16")
    for r, f, t in tables:
        if r["name"] not in whole:
            continue
        E = Entries(torch, t["entries"])
        image, handles, index_h = block_build.table_build(
            E.keys, E.koff, E.values, E.image, cmp=r["cmp"], block_size=r["block_size"],
            restart_interval=r["restart_interval"], bits_per_key=r["bits_per_key"])
        assert image.cpu().numpy().tobytes() == f, r["name"]
        assert handles.cpu().tolist() == [x for h in t["handles"] for x in h]
        assert tuple(index_h) == t["index_h"]
        if r["name"] == "internal_bloom10_bs1024_ri16":
            metas = dict((k, t["meta"][vo:vo + vl]) for k, vo, vl, _ in bm.walk(t["meta"])[1])
            fh = bm.decode_handle(metas[bd.FILTER_KEY])
            res = block.table_get(image, index_h, E.keys, E.koff, filter=image[fh[0]:fh[0] + fh[1]].contiguous(),
                                  verify=True, cmp=block.INTERNAL_KEY, bits_per_key=10)
            assert not res.state.cpu().numpy().any()
            assert res.key_len.cpu().tolist() == [len(k) for k, _ in t["entries"]]
            img, val = image.cpu().numpy(), res.value.cpu().numpy()
            assert [img[int(o):int(o) + int(n)].tobytes() for o, n in val] == [v for _, v in t["entries"]]
    with pytest.raises(ValueError):
        block_build.table_build(E.keys, E.koff, E.values, E.image, compression=1)


def _blob(b):
    b = bytes(b)
    return struct.pack("<Q", len(b)) + b


@pytest.mark.gpu
def test_cpp_block_builder_layer(torch_cuda, tables, tmp_path):
    """7. include/lsbm/block_builder.h (PlanBlocks, BuildBlocks,
    BuildIndexBlocks) against the fixture, driven by tests/cpp/block_build_tool.cc."""
    exe = tmp_path / "block_build_tool"
    libdir = os.path.join(REPO, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"),
                    os.path.join(HERE, "cpp", "block_build_tool.cc"), "-L", libdir, "-llsbm_crc32c",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    r, f, t = [x for x in tables if x[0]["name"] == "internal_bloom10_bs1024_ri16"][0]
    entries, nb = t["entries"], len(t["blocks"])
    keys = b"".join(k for k, _ in entries)
    koff = np.zeros(len(entries) + 1, dtype=np.uint64)
    koff[1:] = np.cumsum([len(k) for k, _ in entries])
    image = b"".join(v for _, v in entries)
    voff = np.zeros(len(entries) + 1, dtype=np.uint64)
    voff[1:] = np.cumsum([len(v) for _, v in entries])
    values = np.stack([voff[:-1], np.diff(voff)], axis=1).astype(np.uint64)
    u64 = lambda a: np.array(a, dtype=np.uint64).tobytes()  # noqa: E731

    def run(mode, a, b=(), c=(), tweak=None):
        ko = koff.copy()
        if tweak:
            tweak(ko)
        cmd = (_blob(u64([mode, r["block_size"], r["restart_interval"], r["cmp"]])) + _blob(keys)
               + _blob(ko.tobytes()) + _blob(values.tobytes()) + _blob(image) + _blob(u64(a)) + _blob(u64(b))
               + _blob(u64(c)))
        fi, fo = tmp_path / "cmd.bin", tmp_path / "out.bin"
        fi.write_bytes(cmd)
        p = subprocess.run([str(exe), str(fi), str(fo)], check=True, capture_output=True, text=True, timeout=120)
        return p.stdout.strip(), fo.read_bytes()

    status, out = run(0, [0, len(entries)])
    assert status == "status OK"
    w = np.frombuffer(out, dtype=np.uint64)
    assert int(w[0]) == nb
    assert list(w[1:nb + 2]) == t["first"] and list(w[nb + 2:2 * nb + 2]) == [len(b) for b in t["blocks"]]
    assert list(w[2 * nb + 2:]) == [0, nb, 0]

    def blocks_of(out):
        n = struct.unpack_from("<Q", out, 0)[0]
        offs = np.frombuffer(out, dtype=np.uint64, count=n + 1, offset=8)
        st = np.frombuffer(out, dtype=np.uint64, count=n, offset=8 * (n + 2))
        body = out[8 * (2 * n + 2):]
        return [body[int(offs[i]):int(offs[i + 1])] for i in range(n)], list(st)

    status, out = run(1, t["first"])
    assert status == "status OK"
    blocks, st = blocks_of(out)
    assert blocks == t["blocks"] and not any(st)
    status, out = run(2, t["first"], [0, nb], [x for h in t["handles"] for x in h])
    assert status == "status OK"
    blocks, st = blocks_of(out)
    assert blocks == [t["index"]] and st == [0]

    def decreasing(ko):
        ko[11] = ko[10] - 1
    status, out = run(1, t["first"], tweak=decreasing)
    assert status == "status Invalid argument: bad block builder input"
    blocks, st = blocks_of(out)
    assert st[0] == 2 and not any(st[1:]) and blocks[1:] == t["blocks"][1:] and blocks[0] == b""
