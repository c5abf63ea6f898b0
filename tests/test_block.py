"""SSTable block reader (table/block.cc: Block, DecodeEntry, Block::Iter).

Parity is pinned by tests/golden/block_fixture.json, which the reference's own
BlockBuilder and Block::Iter produced (tests/golden/make_block_fixture.py),
built blocks and mutated ones, and by the blocks of a real db_bench SSTable
(tests/golden/real_sst.bin).  CPU tests: the plain-Python model
(tests/golden/blockmodel.py) against both, and the C ABI's argument checks.
GPU tests: every entry point of include/lsbm_block.h, lsbm_amd.block.table_get
and the C++ layer include/lsbm/block_reader.h against the fixture and the
model.  Every comparison is exact.
"""
import hashlib
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from golden import blockmodel as bm
from golden.make_real_fixture import block_entries

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
STATUS_CODE = {v: k for k, v in bm.MESSAGE.items()}
MAX_TAG = b"\xff" * 8


def apply_ops(block, ops):
    b = bytearray(block)
    for op in ops:
        if op[0] == "set":
            d = bytes.fromhex(op[2])
            b[op[1]:op[1] + len(d)] = d
        else:
            b = b[:op[1]]
    return bytes(b)


@pytest.fixture(scope="module")
def fixture_cases():
    """[(record, block bytes, the keys its Seek targets derive from)]."""
    fx = json.load(open(os.path.join(G, "block_fixture.json")))
    built = {r["name"]: bytes.fromhex(r["hex"]) for r in fx["built"]}
    cases = []
    for r in fx["built"]:
        b = built[r["name"]]
        cases.append((r, b, [e[0] for e in bm.walk(b)[1]]))
    for r in fx["mutated"]:
        base = built[r["base"]]
        cases.append((r, apply_ops(base, r["ops"]), [e[0] for e in bm.walk(base)[1]]))
    return cases


@pytest.fixture(scope="module")
def real_blocks():
    meta = json.load(open(os.path.join(G, "real_fixture.json")))
    sst = np.fromfile(os.path.join(G, "real_sst.bin"), dtype=np.uint8)
    return meta, sst


def model_probe_record(block, targets, cmp):
    rows, h = [], hashlib.sha256()
    for t in targets:
        r = bm.seek(block, t, cmp)
        rows.append([r["state"], r["pos"], len(r["key"]), r["value_offset"], r["value_length"]])
        h.update(struct.pack("<I", len(r["key"])) + r["key"])
    return {"rows": rows, "keys_sha256": h.hexdigest()}


# ---------------------------------------------------------------- CPU: the model pinned
def test_model_reproduces_fixture(fixture_cases):
    names = [r["name"] for r, _, _ in fixture_cases]
    assert len(names) == len(set(names)) >= 30
    for rec, block, keys in fixture_cases:
        status, ents = bm.walk(block)
        assert bm.MESSAGE[status] == rec["status"], rec["name"]
        assert len(ents) == rec["entries"], rec["name"]
        assert sum(len(e[0]) for e in ents) == rec["key_bytes"], rec["name"]
        assert sum(e[2] for e in ents) == rec["value_bytes"], rec["name"]
        assert bm.entries_sha(block, ents) == rec["sha256"], rec["name"]
        targets = bm.seek_targets(keys)
        assert model_probe_record(block, targets, bm.BYTEWISE) == rec["seek_bytewise"], rec["name"]
        if rec.get("internal"):
            t8 = [t for t in targets if len(t) >= 8]
            assert model_probe_record(block, t8, bm.INTERNAL_KEY) == rec["seek_internal"], rec["name"]


def test_fixture_covers_the_verdicts(fixture_cases):
    by = {r["name"]: r for r, _, _ in fixture_cases}
    for n in range(4):
        assert by[f"size_{n}"]["status"] == "Corruption: bad block contents"
    assert by["num_restarts_max_plus_1"]["status"] == "Corruption: bad block contents"
    assert (by["num_restarts_0"]["status"], by["num_restarts_0"]["entries"]) == ("OK", 0)
    # forward iteration passes a restart entry with shared != 0, Seek does not
    r = by["restart_entry_shared"]
    assert (r["status"], r["entries"]) == ("OK", 12)
    assert any(row[0] == bm.SEEK_BAD_ENTRY for row in r["seek_bytewise"]["rows"])
    assert by["shared_gt_prev_key"]["entries"] == 1
    for n in ("varint_into_limit", "varint5_high_bits_kept", "value_past_limit", "two_bytes_before_limit"):
        assert by[n]["status"] == "Corruption: bad entry in block", n
    assert by["varint5_high_bits_dropped"]["status"] == "OK"


def test_model_builder_reproduces_built_blocks(fixture_cases):
    for rec, block, _ in fixture_cases:
        if "hex" not in rec:
            continue
        ents = [(k, block[vo:vo + vl]) for k, vo, vl, _ in bm.walk(block)[1]]
        assert bm.build_block(ents, rec["restart_interval"]) == block, rec["name"]


def test_model_decodes_real_sstable_blocks(real_blocks):
    meta, sst = real_blocks
    kinds = [b["kind"] for b in meta["table_blocks"]]
    assert kinds.count("data") == 96 and "index" in kinds
    for b in meta["table_blocks"]:
        blk = sst[b["offset"]:b["offset"] + b["size"]].tobytes()
        status, ents = bm.walk(blk)
        assert status == bm.OK
        assert [(k, blk[vo:vo + vl]) for k, vo, vl, _ in ents] == block_entries(blk), b["kind"]
        if b["kind"] == "index":
            handles = [bm.decode_handle(blk[vo:vo + vl]) for _, vo, vl, _ in ents]
            want = [(d["file_offset"], d["size"]) for d in meta["table_blocks"] if d["kind"] == "data"]
            assert handles[:96] == want


def _declared():
    text = open(os.path.join(REPO, "include", "lsbm_block.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lsbm_\w+)\s*\(", text)))


def test_block_symbols_exported_and_declared(product_lib):
    from lsbm_amd import _lib
    names = _declared()
    assert names == ["lsbm_block_decode_dev", "lsbm_block_scan_dev", "lsbm_block_seek_dev"]
    assert sorted(_lib.BLOCK_SIGNATURES) == names
    out = subprocess.run(["nm", "-D", "--defined-only", product_lib._name], capture_output=True,
                         text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert not [n for n in names if n not in exported]


def _fake_args():
    z = np.zeros(16, dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint8)
    return z, buf, z.ctypes.data, buf.ctypes.data


def test_block_entry_points_check_arguments(product_lib):
    """A bad argument is LSBM_ERR_INVALID, with or without a device."""
    from lsbm_amd import _lib
    L = _lib.lib()
    z, buf, zp, bp = _fake_args()
    inv = _lib.LSBM_ERR_INVALID
    assert L.lsbm_block_scan_dev(None, 64, zp, 1, zp, zp, None) == inv
    assert L.lsbm_block_scan_dev(bp, 64, zp, 1, zp, None, None) == inv
    assert L.lsbm_block_decode_dev(bp, 64, zp, 1, None, zp, bp, 8, zp, zp, 1, None, zp, None) == inv
    assert L.lsbm_block_decode_dev(bp, 64, zp, 1, zp, zp, None, 8, zp, zp, 1, None, zp, None) == inv
    seek = lambda **kw: L.lsbm_block_seek_dev(  # noqa: E731
        kw.get("image", bp), 64, zp, bp, zp, 1, kw.get("cmp", 0), kw.get("flags", 0), zp, zp, zp, zp,
        kw.get("hout", zp), kw.get("found", None), kw.get("foff", None), 0, None)
    assert seek(image=None) == inv
    assert seek(cmp=2) == inv
    assert seek(flags=2) == inv
    assert seek(flags=1, hout=None) == inv
    assert seek(found=bp, foff=None) == inv
    # nothing to do is OK before anything is looked at
    assert L.lsbm_block_scan_dev(None, 0, None, 0, None, None, None) == _lib.LSBM_OK
    assert L.lsbm_block_seek_dev(None, 0, None, None, None, 0, 0, 0, None, None, None, None, None, None,
                                 None, 0, None) == _lib.LSBM_OK


def test_block_entry_points_fail_loudly_without_device(product_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    from lsbm_amd import _lib
    L = _lib.lib()
    z, buf, zp, bp = _fake_args()
    # host pointers are not device pointers, but with no device the calls
    # must refuse before touching anything
    nd = _lib.LSBM_ERR_NO_DEVICE
    assert L.lsbm_block_scan_dev(bp, 64, zp, 1, zp, zp, None) == nd
    assert L.lsbm_block_decode_dev(bp, 64, zp, 1, zp, zp, bp, 8, zp, zp, 1, None, zp, None) == nd
    assert L.lsbm_block_seek_dev(bp, 64, zp, bp, zp, 1, 0, 0, zp, zp, zp, zp, None, None, None, 0,
                                 None) == nd


# ---------------------------------------------------------------- GPU helpers
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pack_image(blocks, pad=0):
    """Blocks in one image, block i at an offset that is i mod 16: (image,
    handles int64[2n])."""
    img, handles = bytearray(), []
    for i, b in enumerate(blocks):
        while len(img) % 16 != i % 16:
            img.append(0xEE)
        handles += [len(img), len(b)]
        img += b
    img += b"\xee" * pad
    return np.frombuffer(bytes(img), np.uint8).copy(), np.array(handles, dtype=np.int64)


def pack_keys(keys):
    offs = np.zeros(len(keys) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(k) for k in keys])
    # (one pad byte: a batch of empty keys still has a buffer to point at)
    return np.frombuffer(b"".join(keys) + b"\0", np.uint8).copy(), offs


def gpu_scan_decode(torch, img, handles):
    """scan + decode of every block: (counts, status, per block [(key, value
    offset relative to the block, value length)], decode status)."""
    from lsbm_amd import block
    dimg, dh = _dev(torch, img), _dev(torch, handles)
    counts, status = block.scan(dimg, dh)
    keys, koff, values, ebase, dstatus = block.decode(dimg, dh)
    keys, koff, values, ebase = (t.cpu().numpy() for t in (keys, koff, values, ebase))
    out = []
    for i in range(handles.size // 2):
        ents = []
        for e in range(int(ebase[i]), int(ebase[i + 1])):
            ents.append((keys[int(koff[e]):int(koff[e + 1])].tobytes(),
                         int(values[e, 0]) - int(handles[2 * i]), int(values[e, 1])))
        out.append(ents)
    return counts.cpu().numpy(), status.cpu().numpy(), out, dstatus.cpu().numpy()


def gpu_seek(torch, img, handles, probes, cmp, value_is_handle=False, room=None):
    """probes: [(block index, target)].  Returns the rows [state, pos,
    key_len, value offset relative to the block (0 unless valid), value
    length], the found keys and the handles."""
    from lsbm_amd import block
    hq = np.array([[handles[2 * b], handles[2 * b + 1]] for b, _ in probes], dtype=np.int64).reshape(-1)
    kb, ko = pack_keys([t for _, t in probes])
    found = foff = None
    if room is not None:
        foff = np.zeros(len(probes) + 1, dtype=np.int64)
        foff[1:] = np.cumsum(room)
        found = torch.full((int(foff[-1]) + 32,), 0xAB, dtype=torch.uint8, device="cuda")
        foff = _dev(torch, foff)
    r = block.seek(_dev(torch, img), _dev(torch, hq), _dev(torch, kb), _dev(torch, ko), cmp=cmp,
                   value_is_handle=value_is_handle, found=found, found_offsets=foff)
    state, pos, klen, value = (t.cpu().numpy() for t in (r.state, r.pos, r.key_len, r.value))
    rows = []
    for q in range(len(probes)):
        vo = int(value[q, 0]) - int(hq[2 * q]) if state[q] in (bm.VALID, bm.SEEK_BAD_HANDLE) else int(value[q, 0])
        rows.append([int(state[q]), int(pos[q]), int(klen[q]), vo, int(value[q, 1])])
    fk = None
    if room is not None:
        f, fo = found.cpu().numpy(), foff.cpu().numpy()
        assert (f[int(fo[-1]):] == 0xAB).all()  # nothing past the last window
        fk = [f[int(fo[q]):int(fo[q + 1])].tobytes() for q in range(len(probes))]
    return rows, fk, (r.handle.cpu().numpy() if value_is_handle else None)


def model_rows(blocks, probes, cmp, value_is_handle=False):
    rows, keys, handles = [], [], []
    for b, t in probes:
        r = bm.seek(blocks[b], t, cmp, value_is_handle)
        rows.append([r["state"], r["pos"], len(r["key"]), r["value_offset"], r["value_length"]])
        keys.append(r["key"])
        handles.append(r["handle"])
    return rows, keys, handles


def model_walk_record(block):
    status, ents = bm.walk(block)
    return status, [(k, vo, vl) for k, vo, vl, _ in ents]


# ---------------------------------------------------------------- GPU: the fixture
@pytest.mark.gpu
def test_gpu_fixture_blocks_scan_decode_seek(torch_cuda, fixture_cases):
    torch = torch_cuda
    blocks = [b for _, b, _ in fixture_cases]
    img, handles = pack_image(blocks)
    assert {int(h) % 16 for h in handles[0::2]} == set(range(16))
    counts, status, decoded, dstatus = gpu_scan_decode(torch, img, handles)
    for i, (rec, block, _) in enumerate(fixture_cases):
        assert counts[i].tolist() == [rec["entries"], rec["key_bytes"], rec["value_bytes"]], rec["name"]
        assert status[i] == dstatus[i] == STATUS_CODE[rec["status"]], rec["name"]
        assert bm.entries_sha(block, [(k, vo, vl, 0) for k, vo, vl in decoded[i]]) == rec["sha256"], rec["name"]
    # every recorded probe in one launch per comparator
    for field, cmp in (("seek_bytewise", bm.BYTEWISE), ("seek_internal", bm.INTERNAL_KEY)):
        probes, want, spans = [], [], []
        for i, (rec, _, keys) in enumerate(fixture_cases):
            if field not in rec:
                continue
            t = bm.seek_targets(keys)
            if cmp == bm.INTERNAL_KEY:
                t = [x for x in t if len(x) >= 8]
            assert len(t) == len(rec[field]["rows"])
            spans.append((rec, len(probes), len(probes) + len(t)))
            probes += [(i, x) for x in t]
            want += rec[field]["rows"]
        assert probes
        rows, fk, _ = gpu_seek(torch, img, handles, probes, cmp, room=[w[2] for w in want])
        for rec, a, b in spans:
            assert rows[a:b] == want[a:b], (rec["name"], field)
            h = hashlib.sha256()
            for k in fk[a:b]:
                h.update(struct.pack("<I", len(k)) + k)
            assert h.hexdigest() == rec[field]["keys_sha256"], (rec["name"], field)


# ---------------------------------------------------------------- GPU: a real table
@pytest.mark.gpu
def test_gpu_real_sstable_blocks(torch_cuda, real_blocks):
    from test_bloom import real_table_keys
    from lsbm_amd import block
    torch = torch_cuda
    meta, sst = real_blocks
    handles = np.array([[b["offset"], b["size"]] for b in meta["table_blocks"]], dtype=np.int64).reshape(-1)
    assert handles.size == 2 * 98
    counts, status, decoded, dstatus = gpu_scan_decode(torch, sst, handles)
    for i, b in enumerate(meta["table_blocks"]):
        st, ents = model_walk_record(sst[b["offset"]:b["offset"] + b["size"]].tobytes())
        assert status[i] == dstatus[i] == st == bm.OK
        assert counts[i].tolist() == [len(ents), sum(len(e[0]) for e in ents), sum(e[2] for e in ents)]
        assert decoded[i] == ents, i
    # the data blocks' keys + key_offsets: the pair the host parse gives bloom.build_filters
    (kb, ko), _, _ = real_table_keys(meta, sst)
    keys, koff, _, ebase, _ = block.decode(_dev(torch, sst), _dev(torch, handles[:2 * 96]))
    assert int(ebase[-1]) == ko.size - 1
    assert np.array_equal(koff.cpu().numpy(), ko.astype(np.int64))
    assert keys.cpu().numpy().tobytes() == kb.tobytes()


# ---------------------------------------------------------------- GPU: kernel shapes
def shaped_blocks():
    """Blocks built by the model's builder at the sizes where the kernels take
    another path: 1 / 63 / 64 / 65 / 128 / 129 restart intervals (the 64-lane
    chunks), interval 1, and a 200 KB block (past the LDS tile) between two
    7-byte blocks."""
    def entries(n, klen=10, tag=False):
        out = []
        for i in range(n):
            k = (b"k%0*d" % (klen - 1, i)) + (struct.pack("<Q", (1000 - i % 7) << 8 | 1) if tag else b"")
            out.append((k, b"v" * (i % 9)))
        return out
    blocks = [bm.build_block(entries(2 * r - 1), 2) for r in (1, 63, 64, 65, 128, 129)]
    blocks.append(bm.build_block(entries(100, tag=True), 1))
    blocks.append(b"abc" + struct.pack("<I", 0))
    big = bm.build_block(entries(5200, klen=24, tag=True), 1)
    assert len(big) > 200_000
    blocks.append(big)
    blocks.append(b"xyz" + struct.pack("<I", 0))
    for b, r in zip(blocks, (1, 63, 64, 65, 128, 129, 100, 0, 5200, 0)):
        assert bm.block_layout(b)[1] == r
    return blocks


@pytest.fixture(scope="module")
def shaped():
    blocks = shaped_blocks()
    img, handles = pack_image(blocks)
    return blocks, img, handles, [model_walk_record(b) for b in blocks]


@pytest.mark.gpu
def test_gpu_kernel_shapes_scan_decode(torch_cuda, shaped):
    from lsbm_amd import block
    torch = torch_cuda
    blocks, img, handles, want = shaped
    counts, status, decoded, dstatus = gpu_scan_decode(torch, img, handles)
    for i, (st, ents) in enumerate(want):
        assert status[i] == dstatus[i] == st == bm.OK, i
        assert counts[i].tolist() == [len(ents), sum(len(e[0]) for e in ents), sum(e[2] for e in ents)], i
        assert decoded[i] == ents, i
    # n = 0
    dimg = _dev(torch, img)
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    c0, s0 = block.scan(dimg, none)
    assert c0.numel() == 0 and s0.numel() == 0
    k0, ko0, v0, eb0, st0 = block.decode(dimg, none)
    assert k0.numel() == 0 and ko0.cpu().tolist() == [0] and eb0.cpu().tolist() == [0] and st0.numel() == 0
    # a handle that ends 1 byte past the image; a size >= 2^32; an offset past the image
    last_off = int(handles[-2])
    odd = np.array([last_off, img.size - last_off + 1, 0, 1 << 32, img.size + 1, 0, img.size, 0,
                    int(handles[0]), int(handles[1])], dtype=np.int64)
    c, s = block.scan(dimg, _dev(torch, odd))
    assert s.cpu().tolist() == [bm.BAD_CONTENTS] * 4 + [bm.OK]
    assert c.cpu().numpy()[:4].tolist() == [[0, 0, 0]] * 4
    assert c.cpu().numpy()[4].tolist() == counts[0].tolist()
    _, _, _, eb, ds = block.decode(dimg, _dev(torch, odd))
    assert ds.cpu().tolist() == [bm.BAD_CONTENTS] * 4 + [bm.OK] and int(eb[-1]) == counts[0][0]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [1, 3, 6])
def test_gpu_decode_windows_too_small(torch_cuda, shaped, which):
    """A key window 1 byte too small and an entry window 1 entry too small
    give status 3, and the canary bytes after each window stay intact."""
    from lsbm_amd import block
    torch = torch_cuda
    blocks, img, handles, want = shaped
    ents = want[which][1]
    ne, nk = len(ents), sum(len(e[0]) for e in ents)
    dimg, dh = _dev(torch, img), _dev(torch, handles[2 * which:2 * which + 2])

    def run(ecap, kcap):
        keys = torch.full((nk + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        koff = torch.full((ne + 9,), -7, dtype=torch.int64, device="cuda")
        vals = torch.full((ne + 8, 2), -7, dtype=torch.int64, device="cuda")
        eb = _dev(torch, np.array([0, ecap], dtype=np.int64))
        kb = _dev(torch, np.array([0, kcap], dtype=np.int64))
        *_, st = block.decode(dimg, dh, entry_base=eb, key_base=kb, keys=keys, key_offsets=koff, values=vals)
        return int(st[0]), keys.cpu().numpy(), koff.cpu().numpy(), vals.cpu().numpy()

    st, keys, koff, vals = run(ne, nk)  # exact windows inside larger buffers
    assert st == bm.OK
    assert keys[:nk].tobytes() == b"".join(e[0] for e in ents) and (keys[nk:] == 0xAB).all()
    assert koff[0] == 0 and koff[ne] == nk and (koff[ne + 1:] == -7).all() and (vals[ne:] == -7).all()
    for ecap, kcap in ((ne, nk - 1), (ne - 1, nk)):
        st, keys, koff, vals = run(ecap, kcap)
        assert st == bm.NO_ROOM
        assert (keys[kcap:] == 0xAB).all()
        assert (koff[ecap + 1:] == -7).all() and (vals[ecap:] == -7).all()


def sampled_targets(keys, cap=60):
    step = max(1, len(keys) // cap)
    return bm.seek_targets(keys[::step] + keys[-1:])


@pytest.mark.gpu
def test_gpu_seek_shapes_and_real_blocks(torch_cuda, shaped, real_blocks):
    torch = torch_cuda
    blocks, img, handles, want = shaped
    meta, sst = real_blocks
    # the real table's blocks behind the shaped ones, in one image
    rb = [sst[b["offset"]:b["offset"] + b["size"]].tobytes() for b in meta["table_blocks"]]
    allb = blocks + rb
    img, handles = pack_image(allb)
    probes = []
    for i, b in enumerate(allb):
        keys = [e[0] for e in bm.walk(b)[1]]
        probes += [(i, t) for t in sampled_targets(keys, 60 if i < len(blocks) else 8)]
    # the internal comparator only where every key has its 8-byte tag
    tagged = {i for i, b in enumerate(allb) if all(len(e[0]) >= 8 for e in bm.walk(b)[1])}
    assert len(tagged) >= 98 + 2  # the real table's blocks and the tagged shaped ones
    for cmp in (bm.BYTEWISE, bm.INTERNAL_KEY):
        sel = [p for p in probes if cmp == bm.BYTEWISE or p[0] in tagged]
        wrows, wkeys, _ = model_rows(allb, sel, cmp)
        rows, fk, _ = gpu_seek(torch, img, handles, sel, cmp, room=[len(k) for k in wkeys])
        assert rows == wrows, cmp
        assert fk == wkeys, cmp
        assert {r[0] for r in wrows} >= {bm.VALID, bm.NOT_VALID}
    # a 5-byte key under the internal comparator: "bad entry in block"
    short = bm.build_block([(b"abcde", b"v"), (b"abcdefghijkl", b"w")], 16)
    simg, sh = pack_image([short])
    rows, _, _ = gpu_seek(torch, simg, sh, [(0, b"abcdefghijk0"), (0, b"abc")], bm.INTERNAL_KEY)
    assert [r[0] for r in rows] == [bm.SEEK_BAD_ENTRY] * 2
    assert rows == model_rows([short], [(0, b"abcdefghijk0"), (0, b"abc")], bm.INTERNAL_KEY)[0]


@pytest.mark.gpu
def test_gpu_seek_value_is_handle_and_found_window(torch_cuda, real_blocks):
    torch = torch_cuda
    meta, sst = real_blocks
    tb = meta["table_blocks"]
    rb = [sst[b["offset"]:b["offset"] + b["size"]].tobytes() for b in tb]
    handles = np.array([[b["offset"], b["size"]] for b in tb], dtype=np.int64).reshape(-1)
    index = next(i for i, b in enumerate(tb) if b["kind"] == "index")
    ikeys = [e[0] for e in bm.walk(rb[index])[1]]
    probes = [(index, k) for k in ikeys[:96]]
    rows, _, hout = gpu_seek(torch, sst, handles, probes, bm.INTERNAL_KEY, value_is_handle=True)
    assert [r[0] for r in rows] == [bm.VALID] * 96
    assert hout.tolist() == [[tb[i]["file_offset"], tb[i]["size"]] for i in range(96)]
    # on data blocks the values are not handles: state 4 wherever the model says so
    probes = [(b, t) for b in (0, 17, 95) for t in sampled_targets([e[0] for e in bm.walk(rb[b])[1]], 40)]
    wrows, _, whandles = model_rows(rb, probes, bm.INTERNAL_KEY, value_is_handle=True)
    rows, _, hout = gpu_seek(torch, sst, handles, probes, bm.INTERNAL_KEY, value_is_handle=True)
    assert rows == wrows
    assert [tuple(int(x) & 0xFFFFFFFFFFFFFFFF for x in h) for h in hout.tolist()] == whandles
    # crafted values: truncated varints, one varint only, 10-byte varints, trailing bytes
    vals = [b"\x80", b"\x01", b"", b"\x05\x07", b"\xff" * 9 + b"\x01" + b"\x80\x01", b"\x80" * 10 + b"\x01",
            b"\x02\x03junk"]
    crafted = bm.build_block([(b"k%d" % i, v) for i, v in enumerate(vals)], 2)
    cimg, ch = pack_image([crafted])
    cprobes = [(0, b"k%d" % i) for i in range(len(vals))]
    wrows, _, whandles = model_rows([crafted], cprobes, bm.BYTEWISE, value_is_handle=True)
    assert [r[0] for r in wrows] == [4, 4, 4, 0, 0, 4, 0] and whandles[3] == (5, 7)
    rows, _, hout = gpu_seek(torch, cimg, ch, cprobes, bm.BYTEWISE, value_is_handle=True)
    assert rows == wrows
    assert [tuple(int(x) & 0xFFFFFFFFFFFFFFFF for x in h) for h in hout.tolist()] == whandles
    # the found-key window, with room, with exactly enough, and 1 byte short
    probes = [(3, e[0]) for e in bm.walk(rb[3])[1][:12]]
    wrows, wkeys, _ = model_rows(rb, probes, bm.INTERNAL_KEY)
    for slack in (5, 0):
        rows, fk, _ = gpu_seek(torch, sst, handles, probes, bm.INTERNAL_KEY, room=[len(k) + slack for k in wkeys])
        assert rows == wrows
        assert [k[:len(w)] for k, w in zip(fk, wkeys)] == wkeys
        assert all(k[len(w):] == b"\xab" * slack for k, w in zip(fk, wkeys))
    room = [len(k) - (1 if q % 2 else 0) for q, k in enumerate(wkeys)]
    rows, fk, _ = gpu_seek(torch, sst, handles, probes, bm.INTERNAL_KEY, room=room)
    assert rows == wrows  # the true length is reported either way
    assert [k for q, k in enumerate(fk) if q % 2 == 0] == [k for q, k in enumerate(wkeys) if q % 2 == 0]


# ---------------------------------------------------------------- GPU: Table::InternalGet
def real_filter_block(meta):
    """The table's filter block cut down to the filters the fixture holds
    (real_filter.bin): those filters, their offsets, array offset, base_lg."""
    f = meta["filter"]
    blob = np.fromfile(os.path.join(G, "real_filter.bin"), dtype=np.uint8).tobytes()
    assert len(blob) == f["prefix_bytes"]
    n = f["offsets"].index(f["prefix_bytes"]) if f["prefix_bytes"] in f["offsets"] else len(f["offsets"])
    tail = b"".join(struct.pack("<I", o) for o in f["offsets"][:n])
    return blob + tail + struct.pack("<I", len(blob)) + bytes([f["base_lg"]])


def model_table_get(image, index_block, key, cmp=bm.INTERNAL_KEY):
    """(state, key length, value offset, value length) of InternalGet without
    filter and checksum, blocks of type kNoCompression."""
    r = bm.seek(index_block, key, cmp, value_is_handle=True)
    if r["state"] != bm.VALID:
        return r["state"], 0, 0, 0
    off, size = r["handle"]
    if off > len(image) or size > len(image) - off:
        return bm.SEEK_BAD_CONTENTS, 0, 0, 0
    d = bm.seek(image[off:off + size], key, cmp)
    if d["state"] != bm.VALID:
        return d["state"], 0, 0, 0
    return bm.VALID, len(d["key"]), off + d["value_offset"], d["value_length"]


@pytest.mark.gpu
def test_gpu_table_get_real_sstable(torch_cuda, real_blocks):
    """The 96 data blocks lie at their file offsets and the index block at its
    own in a sparse image (the bytes between are zero).  Index entries past
    block 95 point into that gap: zero bytes parse as a block without restart
    points (not valid), and fail ReadBlock's checksum under verify.  Handles
    past the image need an image that ends before them: the same blocks with
    the index block placed right behind block 95's trailer."""
    from lsbm_amd import block
    torch = torch_cuda
    meta, sst = real_blocks
    tb = meta["table_blocks"]
    data = [b for b in tb if b["kind"] == "data"]
    assert all(b["file_offset"] == b["offset"] for b in data) and data[0]["offset"] == 0
    ix = next(b for b in tb if b["kind"] == "index")
    data_end = data[-1]["offset"] + data[-1]["size"] + 5
    image = np.zeros(ix["file_offset"] + ix["size"] + 5, dtype=np.uint8)
    image[:data_end] = sst[:data_end]
    image[ix["file_offset"]:] = sst[ix["offset"]:ix["offset"] + ix["size"] + 5]
    index_block = sst[ix["offset"]:ix["offset"] + ix["size"]].tobytes()
    index_handle = (ix["file_offset"], ix["size"])
    dimg = _dev(torch, image)
    host = image.tobytes()

    by_block = []  # (key, absolute value offset, value length) of every entry of the 96 blocks
    for b in data:
        blk = sst[b["offset"]:b["offset"] + b["size"]].tobytes()
        by_block.append([(k, b["offset"] + vo, vl) for k, vo, vl, _ in bm.walk(blk)[1]])
    ents = [e for es in by_block for e in es]
    keys = [e[0] for e in ents]

    def get(qkeys, **kw):
        kb, ko = pack_keys(qkeys)
        r = block.table_get(dimg, index_handle, _dev(torch, kb), _dev(torch, ko), **kw)
        return (r.state.cpu().numpy().tolist(), r.key_len.cpu().numpy().tolist(),
                r.value.cpu().numpy().tolist())

    # every key returns its value, with and without the trailer check
    for verify in (True, False):
        state, klen, value = get(keys, verify=verify)
        assert state == [block.SEEK_VALID] * len(keys)
        assert klen == [len(k) for k in keys]
        assert value == [[vo, vl] for _, vo, vl in ents]
    # the same user keys with tag 0 and with the maximum tag land where the model says
    users = sorted({k[:-8] for k in keys})[::5]
    edge = [u + bytes(8) for u in users] + [u + MAX_TAG for u in users]
    want = [model_table_get(host, index_block, k) for k in edge]
    state, klen, value = get(edge, verify=False)
    assert [(s, kl, v[0], v[1]) for s, kl, v in zip(state, klen, value)] == want
    assert state.count(block.SEEK_VALID) >= len(users)
    # (under verify the last user key's tag 0 passes block 95 into the zero gap: a checksum failure)
    state, klen, value = get(edge, verify=True)
    got = [(s, kl, v[0], v[1]) for s, kl, v in zip(state, klen, value)]
    assert got == [w if w[0] == bm.VALID else (block.GET_BAD_CHECKSUM, 0, 0, 0) for w in want]
    # keys of later blocks: their handles point into the zero gap
    later = [e[0] for e in bm.walk(index_block)[1][200:240]]
    state, _, _ = get(later, verify=False)
    assert state == [model_table_get(host, index_block, k)[0] for k in later] == [block.SEEK_NOT_VALID] * 40
    state, _, _ = get(later, verify=True)
    assert state == [block.GET_BAD_CHECKSUM] * 40
    # ... and past the image: "bad block contents", no fault
    compact = np.concatenate([sst[:data_end], sst[ix["offset"]:ix["offset"] + ix["size"] + 5]])
    kb, ko = pack_keys(later + keys[:50])
    for verify in (True, False):
        r = block.table_get(_dev(torch, compact), (data_end, ix["size"]), _dev(torch, kb), _dev(torch, ko),
                            verify=verify)
        assert r.state.cpu().tolist() == [block.SEEK_BAD_CONTENTS] * 40 + [block.SEEK_VALID] * 50
    # a corrupted block fails the checksum only under verify; a compressed type asks for snappy
    bad = image.copy()
    bad[data[2]["offset"] + 100] ^= 1
    bad[data[4]["offset"] + data[4]["size"]] = 1
    kb, ko = pack_keys([e[0] for e in by_block[2][:3] + by_block[4][:3]])
    r = block.table_get(_dev(torch, bad), index_handle, _dev(torch, kb), _dev(torch, ko), verify=True)
    assert r.state.cpu().tolist() == [block.GET_BAD_CHECKSUM] * 6
    r = block.table_get(_dev(torch, bad), index_handle, _dev(torch, kb), _dev(torch, ko), verify=False)
    assert r.state.cpu().tolist()[3:] == [block.GET_NEEDS_UNCOMPRESS] * 3
    # with the table's filter block no present key is filtered out; absent user keys mostly are
    filt = _dev(torch, np.frombuffer(real_filter_block(meta), np.uint8).copy())
    state, klen, value = get(keys, filter=filt, bits_per_key=20)
    assert state == [block.SEEK_VALID] * len(keys) and value == [[vo, vl] for _, vo, vl in ents]
    absent = [k[:-9] + b"~" + k[-8:] for k in keys[:400]]
    state, _, _ = get(absent, filter=filt, bits_per_key=20)
    assert state.count(block.GET_FILTERED) > 300


# ---------------------------------------------------------------- GPU: the C++ layer
@pytest.mark.gpu
def test_cpp_block_reader_layer(torch_cuda, fixture_cases, tmp_path):
    """include/lsbm/block_reader.h: ScanBlocks / DecodeBlocks / SeekBlocks over
    the fixture image, driven by tests/cpp/block_tool.cc."""
    exe = tmp_path / "block_tool"
    libdir = os.path.join(REPO, "lsbm_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"),
                    os.path.join(HERE, "cpp", "block_tool.cc"), "-L", libdir, "-llsbm_crc32c",
                    "-Wl,-rpath," + libdir, "-o", str(exe)], check=True)
    blocks = [b for _, b, _ in fixture_cases]
    img, handles = pack_image(blocks)
    fi, fh = tmp_path / "img", tmp_path / "handles"
    img.tofile(fi)
    handles.astype("<u8").tofile(fh)
    first_bad = next(r["status"] for r, _, _ in fixture_cases if r["status"] != "OK")

    # scan: "<entries> <key bytes> <value bytes> <status>" per block, then the first failure
    r = subprocess.run([str(exe), "scan", str(fi), str(fh)], check=True, capture_output=True, text=True,
                       timeout=120)
    lines = r.stdout.split("\n")
    for i, (rec, _, _) in enumerate(fixture_cases):
        assert lines[i] == "%d %d %d %d" % (rec["entries"], rec["key_bytes"], rec["value_bytes"],
                                            STATUS_CODE[rec["status"]]), rec["name"]
    assert lines[len(blocks)] == "status " + first_bad

    # decode: per block the SHA-256 input is rebuilt here from the tool's dump
    fo = tmp_path / "decoded"
    r = subprocess.run([str(exe), "decode", str(fi), str(fh), str(fo)], check=True, capture_output=True,
                       text=True, timeout=120)
    assert r.stdout.strip() == "status " + first_bad
    buf, p = open(fo, "rb").read(), 0
    for i, (rec, block, _) in enumerate(fixture_cases):
        n = struct.unpack_from("<Q", buf, p)[0]
        p += 8
        ents = []
        for _ in range(n):
            kl, vo, vl = struct.unpack_from("<QQQ", buf, p)
            p += 24
            ents.append((buf[p:p + kl], vo - int(handles[2 * i]), vl, 0))
            p += kl
        assert n == rec["entries"] and bm.entries_sha(block, ents) == rec["sha256"], rec["name"]
    assert p == len(buf)

    # seek: the recorded probes under both comparators, found keys included
    for field, cmp in (("seek_bytewise", 0), ("seek_internal", 1)):
        probes, want = [], []
        for i, (rec, _, keys) in enumerate(fixture_cases):
            if field not in rec:
                continue
            t = bm.seek_targets(keys)
            if cmp:
                t = [x for x in t if len(x) >= 8]
            probes += [(i, x) for x in t]
            want += rec[field]["rows"]
        hq = np.array([[handles[2 * b], handles[2 * b + 1]] for b, _ in probes], dtype="<u8").reshape(-1)
        kb, ko = pack_keys([t for _, t in probes])
        fq, fk, fko, fr = (tmp_path / f"{n}{cmp}" for n in ("hq", "tk", "to", "res"))
        hq.tofile(fq)
        kb.tofile(fk)
        ko.astype("<u8").tofile(fko)
        r = subprocess.run([str(exe), "seek", str(fi), str(fq), str(fk), str(fko), str(cmp), str(fr)],
                           check=True, capture_output=True, text=True, timeout=120)
        bad = [w[0] for w in want if w[0] >= 2]
        msg = bm.SEEK_MESSAGE[bad[0]] if bad else "OK"
        assert r.stdout.strip() == "status " + msg
        buf, p, rows, found = open(fr, "rb").read(), 0, [], []
        for q in range(len(probes)):
            st, pos, kl, vo, vl = struct.unpack_from("<QQQQQ", buf, p)
            p += 40
            found.append(buf[p:p + kl])
            p += kl
            rows.append([st, pos, kl, vo - int(hq[2 * q]) if st == 0 else vo, vl])
        assert rows == want
        assert found == [bm.seek(blocks[b], t, cmp)["key"] for b, t in probes]
