"""Every engine since the CRC one at offsets past 4 GiB.

Small existing cases of each engine are rebased into a sparse arena of
2^32 + 2^26 bytes (tests/high_offsets.py): the payload is copied to
arena[B, B + len) and B is added to every offset that addresses it.  The
expectation is the plain-Python model's output at base 0, moved by B where the
header says an output is an absolute offset and identical everywhere else.
For every B >= 2^32 a decoy of the same layout lies at B - 2^32, so a kernel
that drops the high half of an offset returns a valid, wrong answer.  Writes
that the caller places go to a second arena between 0xEE guards, at the
position itself and at the position minus 2^32.

CPU part: the rebasing helper, the models' position independence under the
per-output shift tables, and the decoy-differs assertions.

Bases.  Each input buffer of a case moves in turn over 2^32 + 4099, 2^32,
2^32 - len and 2^32 - c for the cuts c named in its test, while the case's
other buffers stay parked at 2^32 + k * 2 MiB + 4099 + 2 (k - 1); the first
of these placements passes base + len as the buffer's size.  Entry points and
what reaches them at 2^32 or more (in: offsets read, out: positions written):

    lsbm_block_scan_dev              in: handles
    lsbm_block_decode_dev            in: handles; out: key windows (d_key_base) at 2^32 + 36867, 2^32,
                                     2^32 - nk / 2, 2^32 - nk, 2^32 - 5
    lsbm_block_seek_dev              in: handles, target offsets; out: found-key windows (d_found_offsets) from
                                     2^32 + 45065, 2^32, 2^32 - nf / 2, 2^32 - nf, 2^32 - 3
    lsbm_block_plan_dev              in: key offsets, value slices
    lsbm_block_build_dev             in: key offsets, value slices; out: block windows from 2^32 + 20483,
                                     2^32 - size / 2, 2^32 - size - 3, 2^32 - 5000, 2^32
    lsbm_index_block_build_dev       in: key offsets, data handles; out: windows behind the blocks'
    lsbm_merge_plan_dev              in: key offsets
    lsbm_merge_gather_dev            in: key offsets, value slices (2^32 + 2^25 + 1 as well)
    lsbm_block_pack_plan_dev         in: first_offset 2^32 - 1, - 16, - 2000, 2^32, 2^32 + 4099
    lsbm_block_pack_dev              in: raw offsets from 2^32 + 2 MiB, compressed offsets across the line;
                                     out: 2^32 - 2048 + p and 2^32 - 16 + p for the 16 phases p, 2^32 + 12288 + p
    lsbm_snappy_compress_dev         in: block offsets; out: 2^32 + 8197, 2^32 - n0 / 2, 2^32 - n0 - n1 / 2,
                                     2^32 - n0 - 20, 2^32 - 1, 2^32
    lsbm_snappy_uncompressed_length_dev  in: stream offsets
    lsbm_snappy_uncompress_dev       in: stream offsets; out: as compress
    lsbm_bloom_build_dev             in: key offsets; out (filter_out): 2^32 + 12295, 2^32 - f2 - 20, 2^32 - 1, 2^32
    lsbm_bloom_may_match_dev         in: filter handles, key offsets
    lsbm_filter_block_may_match_dev  in: block handles, key offsets
    lsbm_wb_scan_dev                 in: record pairs
    lsbm_wb_decode_dev               in: record pairs; out: key windows at 2^32 + 12293, 2^32 - 20,
                                     2^32 - nk / 2, 2^32 - nk, 2^32
    lsbm_memtable_sort_dev           in: key offsets
    lsbm_lookup_keys_dev             in: user offsets; out: the same offsets + 8q of the output arena
    lsbm_memtable_get_dev            in: memtable key offsets, lookup key offsets, value slices
    lsbm_find_file_dev               in: bound offsets, lookup key offsets
    lsbm_save_value_dev              in: found-window offsets, lookup key offsets, value slices
    lsbm_slices_gather_dev           in: slices; out: 2^32 + 28673, 2^32 - 100
    lsbm_dbiter_plan_dev             in: key offsets
    lsbm_dbiter_range_dev            in: key offsets, lo offsets, hi offsets
    lsbm_dbiter_emit_dev             in: live value slices into the image

Rejections (an offset of x + 2^32 over a buffer of a few KiB): block reader,
builder, merge, pack, memtable (scan and sort), Get (slices_gather,
lookup_keys) and scans (plan, range).  The snappy and bloom entry points take
no buffer size, so they have nothing to reject.
"""
import os

import numpy as np
import pytest

import high_offsets as ho
from golden import blockmodel as bm
from high_offsets import ARENA_BYTES, FILL, GUARD, LINE

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")


# --------------------------------------------------------------------------- the cases
@pytest.fixture(scope="module")
def block_case():
    return ho.fixture_block_case()


BLOCK_MODES = ((bm.BYTEWISE, False), (bm.INTERNAL_KEY, False), (bm.BYTEWISE, True))


def block_cuts(case):
    """Inside an entry's three-varint header, inside a key's non-shared bytes,
    inside the restart array, between two blocks."""
    h = case.arrays["handles"]
    blk = case.bufs["image"][int(h[0]):int(h[0]) + int(h[1])]
    _, ents = bm.walk(blk)
    key, vo, vl, p = ents[5]
    e = bm.decode_entry(blk, p, len(blk))
    return [int(h[0]) + p + 1, int(h[0]) + e[3] + 1, int(h[0]) + int(h[1]) - 6, int(h[2])]


@pytest.fixture(scope="module")
def snappy_case(snappy_oracle, snappy_golden):
    return ho.fixture_snappy_case(snappy_oracle, snappy_golden)


@pytest.fixture(scope="module")
def bloom_case(bloom_oracle):
    return ho.fixture_bloom_case(bloom_oracle)


@pytest.fixture(scope="module")
def merge_case():
    return ho.merge_case()


# --------------------------------------------------------------------------- CPU: the helper
def test_rebase_then_unrebase_gives_the_case_back(block_case, merge_case):
    for case in (block_case, merge_case):
        bases = {name: LINE + 4099 + 16 * i for i, name in enumerate(sorted(case.bufs))}
        moved = ho.rebase(case, bases)
        for name, (buf, how) in case.addr.items():
            flat, was = moved[name].reshape(-1), case.arrays[name].reshape(-1)
            idx = slice(0, None, 2) if how == "pairs" else slice(None)
            assert (flat[idx] == was[idx] + bases[buf]).all() and flat[idx].min() >= LINE
            if how == "pairs":
                assert (flat[1::2] == was[1::2]).all()
        back = ho.rebase(ho.Case(case.bufs, case.decoy, moved, case.addr), {k: -v for k, v in bases.items()})
        assert set(back) == set(case.arrays)
        for name in back:
            assert back[name].dtype == np.int64 and ho.same(back[name], case.arrays[name]), name
        imgs = ho.host_images(case, {k: 37 for k in case.bufs})
        assert all(imgs[k] == bytes([FILL]) * 37 + case.bufs[k] for k in case.bufs)


def test_bases_cover_the_line():
    b = ho.bases_for(1000, [1, 500, 999, 1000, 0])
    assert b == [LINE + 4099, LINE, LINE - 1000, LINE - 1, LINE - 500, LINE - 999]
    assert (LINE + 4099) % 16 == 3 and (LINE + 4099) % 2 == 1


def small_bases(case):
    return {name: 37 + 64 * i for i, name in enumerate(sorted(case.bufs))}


def check_position_independent(case, model, shifts, note):
    """The model on host buffers with every payload at a small nonzero base
    equals its base-0 outputs moved by the shift table: the expectations of
    the GPU tests are the model's, wherever the bytes lie."""
    base0 = model(case.bufs, case.arrays)
    bases = small_bases(case)
    moved = model(ho.host_images(case, bases), ho.rebase(case, bases))
    ho.assert_same(moved, ho.shift_outputs(base0, shifts, bases), note)
    return base0


def differ_but(base0, decoy, layout_only, note):
    ho.assert_all_differ({k: v for k, v in base0.items() if k not in layout_only},
                         {k: v for k, v in decoy.items() if k not in layout_only}, note)


def test_block_model_is_position_independent_and_decoy_differs(block_case):
    for cmp, vih in BLOCK_MODES:
        model = lambda im, ar: ho.block_model(im, ar, cmp, vih)  # noqa: E731
        base0 = check_position_independent(block_case, model, ho.BLOCK_SHIFTS, (cmp, vih))
        decoy = model(block_case.decoy, block_case.arrays)
        differ_but(base0, decoy, () if vih else ho.BLOCK_LAYOUT_ONLY_WITHOUT_FLAG, (cmp, vih))


def test_snappy_model_is_position_independent_and_decoy_differs(snappy_case, snappy_oracle):
    model = lambda im, ar: ho.snappy_model(im, ar, snappy_oracle)  # noqa: E731
    base0 = check_position_independent(snappy_case, model, ho.SNAPPY_SHIFTS, "snappy")
    decoy = model(snappy_case.decoy, snappy_case.arrays)
    assert base0["ok"].tolist() == [1, 1, 1]
    differ_but(base0, decoy, ho.SNAPPY_LAYOUT_ONLY, "snappy")
    for name in ("compressed", "plain"):  # (both non-empty blocks, not one of them)
        assert all(a != b for a, b in zip(base0[name][:2], decoy[name][:2])), name


def test_bloom_model_is_position_independent_and_decoy_differs(bloom_case, bloom_oracle):
    model = lambda im, ar: ho.bloom_model(im, ar, bloom_oracle, 10)  # noqa: E731
    base0 = check_position_independent(bloom_case, model, ho.BLOOM_SHIFTS, "bloom")
    ho.assert_all_differ(base0, model(bloom_case.decoy, bloom_case.arrays), "bloom")
    assert base0["may"][:40].all() and base0["block_may"][:40].all() and base0["may"][40:].sum() < 10


def test_merge_model_is_position_independent_and_decoy_differs(merge_case):
    for drop in (False, True):
        model = lambda im, ar: ho.merge_model(im, ar, drop)  # noqa: E731
        base0 = check_position_independent(merge_case, model, ho.MERGE_SHIFTS, drop)
        decoy = model(merge_case.decoy, merge_case.arrays)
        differ_but(base0, decoy, ho.MERGE_LAYOUT_ONLY if drop else ho.MERGE_LAYOUT_ONLY_WITHOUT_DROP, drop)
    assert base0["counts"][0] < 257  # the drop rule drops


def test_pack_plan_model_moves_with_first_offset():
    raw, comp = [1, 15, 4097, 300, 64, 17], [-1, 9, 2000, 290, 20, -1]
    a = ho.pack_plan_model(raw, comp, 0, 5)
    b = ho.pack_plan_model(raw, comp, LINE - 100, 5)
    ho.assert_same(b, ho.shift_outputs(a, ho.PACK_PLAN_SHIFTS, {"out": LINE - 100}))
    assert a["types"].tolist() == [0, 1, 1, 0, 1, 0]


def test_pack_mover_decoy_differs():
    sizes, types, data, decoy, src_off, img, dimg = ho.pack_mover_case()
    assert sorted(sizes)[:2] == [1, 15] and 4097 in sizes and set(types) == {0, 1}
    for d, dd, o, t in zip(data, decoy, src_off, types):  # what a truncated source offset would move
        assert len(d) == len(dd) and all(x != y for x, y in zip(d, dd))
        assert bytes(img[t][o:o + len(d)]) == d and bytes(dimg[t][o:o + len(d)]) == dd


# --------------------------------------------------------------------------- GPU: the arena
class Arena:
    """ARENA_BYTES of device memory that nothing fills: only what a case uses
    is written."""

    def __init__(self, torch):
        self.torch = torch
        self.t = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")

    def put(self, off, data):
        a = np.frombuffer(bytes(data), np.uint8)
        assert 0 <= off and off + a.size <= ARENA_BYTES
        if a.size:
            self.t[off:off + a.size].copy_(self.torch.from_numpy(a.copy()))

    def get(self, off, n):
        return self.t[off:off + n].cpu().numpy().tobytes()

    def image(self, size=ARENA_BYTES):
        return self.t[:size]

    def place(self, case, bases):
        """Every payload at its base, and below every base >= 2^32 the decoy."""
        for name, b in bases.items():
            self.put(b, case.bufs[name])
            if b >= LINE:
                self.put(b - LINE, case.decoy[name])

    def size_for(self, case, bases, name, exact):
        return bases[name] + len(case.bufs[name]) if exact else ARENA_BYTES


class Guarded:
    """Writes into the output arena: 4 KiB of 0xEE on either side of every
    window, and the same around the window minus 2^32, where a store through
    a truncated address would land."""

    def __init__(self, arena):
        self.arena, self.windows = arena, []

    def window(self, pos, n):
        assert pos - GUARD >= 0 and pos + n + GUARD <= ARENA_BYTES
        self.windows.append((int(pos), int(n)))

    def _regions(self):
        spans = []
        for pos, n in self.windows:
            spans.append((pos - GUARD, pos + n + GUARD))
            if pos + n > LINE:
                spans.append((max(0, pos - LINE - GUARD), pos + n - LINE + GUARD))
        spans.sort()
        merged = []
        for a, b in spans:
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        return merged

    def prefill(self):
        for a, b in self._regions():
            self.arena.t[a:b].fill_(FILL)

    def verify(self, writes, note=""):
        """writes: [(pos, bytes)] that must be there; bytes of a window that no
        write names are the call's own; everything else is still 0xEE."""
        for a, b in self._regions():
            got = np.frombuffer(self.arena.get(a, b - a), np.uint8)
            want = np.full(b - a, FILL, dtype=np.uint8)
            care = np.ones(b - a, dtype=bool)
            for pos, n in self.windows:
                lo, hi = max(pos, a), min(pos + n, b)
                if lo < hi:
                    care[lo - a:hi - a] = False
            for pos, data in writes:
                lo, hi = max(pos, a), min(pos + len(data), b)
                if lo < hi:
                    want[lo - a:hi - a] = np.frombuffer(data, np.uint8)[lo - pos:hi - pos]
                    care[lo - a:hi - a] = True
            bad = np.nonzero(care & (got != want))[0]
            assert bad.size == 0, (note, "first wrong byte at", a + int(bad[0]))


@pytest.fixture(scope="module")
def arenas(torch_cuda):
    torch = torch_cuda
    pair = [Arena(torch), Arena(torch)]
    yield pair[0], pair[1]
    for a in pair:
        a.t = None
    pair.clear()
    torch.cuda.empty_cache()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).cuda()


def _np(t):
    return t.cpu().numpy().astype(np.int64)


def parked(case, moving):
    """Bases of the buffers that are not the one under test: wholly above the
    line, 2 MiB apart, each at another odd phase."""
    return {name: LINE + (i + 1) * (1 << 21) + 4099 + 2 * i
            for i, name in enumerate(sorted(case.bufs)) if name != moving}


def placements(case, cuts):
    """Each buffer in turn over its bases, the others parked high; the
    first placement of every buffer ends its image just past the payload."""
    for name in sorted(case.bufs):
        for i, b in enumerate(ho.bases_for(len(case.bufs[name]), cuts.get(name, []))):
            bases = parked(case, name)
            bases[name] = b
            yield name, bases, i == 0


# --------------------------------------------------------------------------- GPU: block reader
FOUND_HIGH = LINE + 11 * 4096 + 9


def gpu_block(torch, arena, out, case, bases, arrays, cmp, vih, want, exact, fout=FOUND_HIGH):
    """scan, decode and seek.  The found keys go to windows of the output arena
    from `fout` on (d_found_offsets are the caller's), each exactly as long
    as its key."""
    from lsbm_amd import block
    img = arena.image(arena.size_for(case, bases, "image", exact))
    dh = _dev(torch, arrays["handles"])
    counts, status = block.scan(img, dh)
    keys, koff, values, _, dstatus = block.decode(img, dh)
    assert _np(dstatus).tolist() == _np(status).tolist()
    room = want["key_len"]
    foff = fout + np.concatenate([[0], np.cumsum(room)])
    nf = int(foff[-1]) - fout
    g = Guarded(out)
    g.window(fout, nf)
    g.prefill()
    r = block.seek(img, _dev(torch, arrays["seek_handles"]), arena.t, _dev(torch, arrays["target_offsets"]),
                   cmp=cmp, value_is_handle=vih, found=out.image(fout + nf if exact else ARENA_BYTES),
                   found_offsets=_dev(torch, foff))
    g.verify([(fout, want["found"])], ("found", hex(fout)))
    return {"counts": _np(counts), "status": _np(status), "keys": keys.cpu().numpy().tobytes(),
            "key_offsets": _np(koff), "values": _np(values), "state": _np(r.state), "pos": _np(r.pos),
            "key_len": _np(r.key_len), "value": _np(r.value),
            "handle": _np(r.handle) if vih else np.zeros((room.size, 2), dtype=np.int64),
            "found": out.get(fout, nf)}


@pytest.mark.gpu
def test_gpu_block_reader_past_4gib(torch_cuda, arenas, block_case):
    torch, (arena, out) = torch_cuda, arenas
    case = block_case
    base0 = {m: ho.block_model(case.bufs, case.arrays, *m) for m in BLOCK_MODES}
    cuts = {"image": block_cuts(case), "targets": [len(case.bufs["targets"]) // 2]}
    n = 0
    for name, bases, exact in placements(case, cuts):
        arena.place(case, bases)
        arrays = ho.rebase(case, bases)
        for mode in BLOCK_MODES if name == "image" else BLOCK_MODES[1:2]:
            want = ho.shift_outputs(base0[mode], ho.BLOCK_SHIFTS, bases)
            got = gpu_block(torch, arena, out, case, bases, arrays, mode[0], mode[1], want, exact)
            ho.assert_same(got, want, (name, hex(bases[name]), mode, exact))
            n += 1
    assert n >= 3 * 7
    # seek's found-key windows across the line: inside a key, ending on it, starting on it
    bases = parked(case, None)
    arena.place(case, bases)
    arrays = ho.rebase(case, bases)
    for mode in BLOCK_MODES[:2]:
        want = ho.shift_outputs(base0[mode], ho.BLOCK_SHIFTS, bases)
        nf = len(want["found"])
        assert nf > 100
        for fout in (LINE, LINE - nf // 2, LINE - nf, LINE - 3):
            got = gpu_block(torch, arena, out, case, bases, arrays, mode[0], mode[1], want, fout == LINE - nf, fout)
            ho.assert_same(got, want, ("found", hex(fout), mode))
    # decode's key windows are the caller's (d_key_base): past 4 GiB and across the line in the output arena
    from lsbm_amd import block
    bases = parked(case, None)
    arena.place(case, bases)
    arrays = ho.rebase(case, bases)
    want = ho.shift_outputs(base0[BLOCK_MODES[0]], ho.BLOCK_SHIFTS, bases)
    c = want["counts"]
    ne, nk = int(c[:, 0].sum()), int(c[:, 1].sum())
    for kout in (LINE + 9 * 4096 + 3, LINE, LINE - nk // 2, LINE - nk, LINE - 5):
        g = Guarded(out)
        g.window(kout, nk)
        g.prefill()
        koff = torch.full((ne + 1,), -2, dtype=torch.int64, device="cuda")
        *_, st = block.decode(arena.image(), _dev(torch, arrays["handles"]),
                              entry_base=_dev(torch, np.concatenate([[0], np.cumsum(c[:, 0])])),
                              key_base=_dev(torch, kout + np.concatenate([[0], np.cumsum(c[:, 1])])),
                              keys=out.image(kout + nk), key_offsets=koff,
                              values=torch.zeros((ne, 2), dtype=torch.int64, device="cuda"))
        assert _np(st).tolist() == want["status"].tolist()
        g.verify([(kout, want["keys"])], ("key window", hex(kout)))
        assert _np(koff).tolist() == (want["key_offsets"] + kout).tolist(), hex(kout)


@pytest.mark.gpu
def test_gpu_block_reader_rejects_offset_past_small_image(torch_cuda, arenas, block_case):
    """A handle at x + 2^32 over an image of a few KiB is "bad block contents";
    a bounds check on the low half alone would read block x."""
    from lsbm_amd import block
    torch, (arena, _) = torch_cuda, arenas
    case = block_case
    arena.put(0, case.bufs["image"])
    n_img = len(case.bufs["image"])
    h = case.arrays["handles"].copy()
    want = ho.block_model(case.bufs, case.arrays, bm.BYTEWISE, False)
    h[2] += LINE
    img = arena.image(n_img)
    counts, status = block.scan(img, _dev(torch, h))
    assert _np(status).tolist() == [bm.OK, bm.BAD_CONTENTS, bm.OK]
    assert _np(counts)[[0, 2]].tolist() == want["counts"][[0, 2]].tolist() and _np(counts)[1].tolist() == [0, 0, 0]
    *_, dstatus = block.decode(img, _dev(torch, h))
    assert _np(dstatus).tolist() == [bm.OK, bm.BAD_CONTENTS, bm.OK]
    qh = case.arrays["seek_handles"].copy()
    hit = np.nonzero(qh[0::2] == case.arrays["handles"][2])[0]
    qh[2 * hit] += LINE
    arena.put(1 << 20, case.bufs["targets"])
    to = case.arrays["target_offsets"] + (1 << 20)
    r = block.seek(img, _dev(torch, qh), arena.t, _dev(torch, to))
    state = _np(r.state)
    assert (state[hit] == bm.SEEK_BAD_CONTENTS).all() and hit.size
    keep = np.setdiff1d(np.arange(state.size), hit)
    assert state[keep].tolist() == want["state"][keep].tolist()
    assert _np(r.value)[keep].tolist() == want["value"][keep].tolist()


# --------------------------------------------------------------------------- GPU: snappy
def gpu_snappy(torch, arena, out, case, bases, arrays, want, out_pos, note):
    """compress and uncompress into the output arena from out_pos on."""
    from lsbm_amd import snappy
    n = arrays["raw_offsets"].size - 1
    lens = np.diff(arrays["raw_offsets"])
    caps = np.array([snappy.max_compressed_length(int(x)) for x in lens], dtype=np.int64)
    coff = out_pos + np.concatenate([[0], np.cumsum(caps + 24)[:-1]])  # (windows 24 bytes apart)
    g = Guarded(out)
    for p, c in zip(coff, caps):
        g.window(p, c)
    g.prefill()
    _, _, clen = snappy.compress(arena.t, _dev(torch, arrays["raw_offsets"]), out=out.t,
                                 out_offsets=_dev(torch, np.concatenate([coff, coff[-1:] + caps[-1:]])))
    clen = _np(clen)
    g.verify([(int(p), s) for p, s in zip(coff, want["compressed"])], note + ("compress",))
    got = {"compressed": [out.get(int(coff[i]), int(clen[i])) for i in range(n)], "compressed_len": clen}
    ulen, lok = snappy.uncompressed_length(arena.t, _dev(torch, arrays["comp_offsets"]))
    got["ulen"], got["len_ok"] = _np(ulen), _np(lok)
    uoff = out_pos + np.concatenate([[0], np.cumsum(want["ulen"])])
    g = Guarded(out)
    g.window(int(uoff[0]), int(uoff[-1] - uoff[0]))
    g.prefill()
    _, _, ok, n_bad = snappy.uncompress(arena.t, _dev(torch, arrays["comp_offsets"]), out=out.t,
                                        out_offsets=_dev(torch, uoff))
    assert int(n_bad.item()) == 0
    g.verify([(int(uoff[0]), b"".join(want["plain"]))], note + ("uncompress",))
    got["ok"] = _np(ok)
    got["plain"] = [out.get(int(uoff[i]), int(uoff[i + 1] - uoff[i])) for i in range(n)]
    return got


@pytest.mark.gpu
def test_gpu_snappy_past_4gib(torch_cuda, arenas, snappy_case, snappy_oracle):
    torch, (arena, out) = torch_cuda, arenas
    case = snappy_case
    want = ho.snappy_model(case.bufs, case.arrays, snappy_oracle)
    ro, co = case.arrays["raw_offsets"], case.arrays["comp_offsets"]
    # inside a literal run (the incompressible block), inside a copy's source
    # window (the periodic block), in the input and in the stream
    cuts = {"raw": [int(ro[1]) // 2, int(ro[1] + (ro[2] - ro[1]) // 2), int(ro[1]) + 20],
            "comp": [int(co[1]) // 2, int(co[1] + (co[2] - co[1]) // 2)]}
    for name, bases, _ in placements(case, cuts):
        arena.place(case, bases)
        got = gpu_snappy(torch, arena, out, case, bases, ho.rebase(case, bases), want, LINE + 8192 + 5,
                         (name, hex(bases[name])))
        ho.assert_same(got, want, (name, hex(bases[name])))
    # the outputs across the line: inside the literal run, and inside the
    # periodic block's output, whose copies then read their source across it
    bases = parked(case, None)
    arena.place(case, bases)
    arrays = ho.rebase(case, bases)
    n0 = int(want["ulen"][0])
    for pos in (LINE - n0 // 2, LINE - n0 - int(want["ulen"][1]) // 2, LINE - n0 - 20, LINE - 1, LINE):
        got = gpu_snappy(torch, arena, out, case, bases, arrays, want, pos, ("out", hex(pos)))
        ho.assert_same(got, want, ("out", hex(pos)))


# --------------------------------------------------------------------------- GPU: bloom
def gpu_bloom(torch, arena, out, case, bases, arrays, want, out_pos, note):
    from lsbm_amd import bloom
    bits = case.extra["bits_per_key"]
    sizes = case.extra["filter_bytes"]
    fout = out_pos + case.arrays["filter_out"] + 3 * np.arange(len(sizes))  # (3 bytes apart)
    g = Guarded(out)
    for p, n in zip(fout, sizes):
        g.window(int(p), n)
    g.prefill()
    bloom.build_filters(arena.t, _dev(torch, arrays["key_offsets"]), _dev(torch, arrays["filter_first"]),
                        _dev(torch, fout), out.t, bits)
    torch.cuda.synchronize()
    g.verify([(int(p), f) for p, f in zip(fout, want["built"])], note)
    got = {"built": [out.get(int(p), n) for p, n in zip(fout, sizes)]}
    po = _dev(torch, arrays["probe_offsets"])
    may, n_may = bloom.may_match(arena.t, _dev(torch, arrays["filter_handles"]), arena.t, po, bits)
    got["may"] = _np(may)
    assert int(n_may.item()) == int(got["may"].sum())
    may, _ = bloom.filter_block_may_match(arena.t, _dev(torch, arrays["fblock_handles"]),
                                          _dev(torch, arrays["data_offsets"]), arena.t, po, bits)
    got["block_may"] = _np(may)
    return got


@pytest.mark.gpu
def test_gpu_bloom_past_4gib(torch_cuda, arenas, bloom_case, bloom_oracle):
    torch, (arena, out) = torch_cuda, arenas
    case = bloom_case
    want = ho.bloom_model(case.bufs, case.arrays, bloom_oracle, 10)
    ko, fo = case.arrays["key_offsets"], case.arrays["filter_out"]
    cuts = {"keys": [int(ko[31]) + 3], "probes": [int(case.arrays["probe_offsets"][17]) + 2],
            "filters": [int(fo[2]) + 20, int(fo[1]) + 5], "fblock": [int(fo[2]) + 20]}
    for name, bases, _ in placements(case, cuts):
        arena.place(case, bases)
        got = gpu_bloom(torch, arena, out, case, bases, ho.rebase(case, bases), want, LINE + 4096 * 3 + 7,
                        (name, hex(bases[name])))
        ho.assert_same(got, want, (name, hex(bases[name])))
    bases = parked(case, None)
    arena.place(case, bases)
    for pos in (LINE - int(fo[2]) - 20, LINE - 1, LINE):  # the line inside a filter's bit array as it is built
        got = gpu_bloom(torch, arena, out, case, bases, ho.rebase(case, bases), want, pos, ("out", hex(pos)))
        ho.assert_same(got, want, ("out", hex(pos)))


# --------------------------------------------------------------------------- GPU: pack
PACK_RAW = [1, 15, 4097, 300, 64, 17]
PACK_COMP = [-1, 9, 2000, 290, 20, -1]


@pytest.mark.gpu
def test_gpu_pack_plan_across_the_line(torch_cuda):
    from lsbm_amd import sstable
    torch = torch_cuda
    base0 = ho.pack_plan_model(PACK_RAW, PACK_COMP, 0, 5)
    for first in (LINE - 1, LINE - 16, LINE - 2000, LINE, LINE + 4099):
        for gap in (5, 0):
            want = ho.pack_plan_model(PACK_RAW, PACK_COMP, first, gap)
            if gap == 5:
                ho.assert_same(want, ho.shift_outputs(base0, ho.PACK_PLAN_SHIFTS, {"out": first}))
            types, handles, end = sstable.pack_plan(_dev(torch, PACK_RAW), _dev(torch, PACK_COMP), first, gap)
            ho.assert_same({"types": _np(types), "handles": _np(handles), "end": _np(end)}, want, (hex(first), gap))
            assert first >= LINE or want["handles"][0] < LINE <= want["end"][0]


@pytest.mark.gpu
def test_gpu_pack_mover_past_4gib(torch_cuda, arenas):
    """Blocks of 1, 15 and 4097 bytes among others, raw and compressed sources
    past 4 GiB, destinations across the line at all 16 phases with a source
    phase that is the same and one that is 5 off."""
    from lsbm_amd import sstable
    torch, (arena, out) = torch_cuda, arenas
    sizes, types, data, decoy, src_off, img, dimg = ho.pack_mover_case()
    ran = 0
    for phase in range(16):
        for diff in (0, 5):
            for straddler in (0, 1):  # the 4097-byte block, the 15-byte block
                if straddler == 1 and (phase < 2 or diff != (0 if phase % 2 else 5)):
                    continue
                d0 = (LINE - 2048 if straddler == 0 else LINE - 16) + phase
                dest = [0] * 6
                dest[straddler] = d0
                nxt = LINE + 3 * 4096 + phase
                for i in range(6):
                    if i != straddler:
                        dest[i] = nxt
                        nxt += sizes[i] + 16
                # the sources: the raw image above the line, the compressed one across it
                sb = {0: LINE + (1 << 21) + ((d0 + diff - src_off[0]) % 16),
                      1: LINE - 112 + ((d0 + diff - src_off[1]) % 16)}
                if straddler == 1:
                    sb = {0: sb[0], 1: LINE - 32 + ((d0 + diff - src_off[1]) % 16)}
                assert (sb[types[straddler]] + src_off[straddler] - d0) % 16 == diff
                for t in (0, 1):
                    arena.put(sb[t], img[t])
                    if sb[t] >= LINE:
                        arena.put(sb[t] - LINE, dimg[t])
                rh = np.array([[sb[0] + o, n] if t == 0 else [0, 0] for o, n, t in zip(src_off, sizes, types)])
                co = np.array([sb[1] + o if t == 1 else 0 for o, t in zip(src_off, types)])
                handles = np.array([[d, n] for d, n in zip(dest, sizes)]).reshape(-1)
                g = Guarded(out)
                for d, n in zip(dest, sizes):
                    g.window(d, n)
                g.prefill()
                exact = phase == 3
                st = sstable.pack(arena.image(sb[0] + len(img[0]) if exact else ARENA_BYTES), _dev(torch, rh.reshape(-1)),
                                  arena.image(sb[1] + len(img[1]) if exact else ARENA_BYTES), _dev(torch, co),
                                  torch.tensor(types, dtype=torch.uint8, device="cuda"), _dev(torch, handles),
                                  out.image(max(dest[i] + sizes[i] for i in range(6)) if exact else ARENA_BYTES),
                                  gap=0)
                assert _np(st).tolist() == [0] * 6, (phase, diff, straddler)
                g.verify(list(zip(dest, data)), (phase, diff, straddler))
                ran += 1
    assert ran >= 32 + 14


@pytest.mark.gpu
def test_gpu_pack_rejects_offsets_past_small_images(torch_cuda, arenas):
    from lsbm_amd import sstable
    torch, (arena, out) = torch_cuda, arenas
    data = bytes(range(200))
    arena.put(0, data)
    g = Guarded(out)
    g.window(GUARD, 600)
    g.prefill()
    rh = np.array([0, 50, 60 + LINE, 50, 120, 50, 10, 50], dtype=np.int64)
    handles = np.array([GUARD, 50, GUARD + 100, 50, GUARD + 200, 50, GUARD + 300 + LINE, 50], dtype=np.int64)
    st = sstable.pack(arena.image(200), _dev(torch, rh), None, None, torch.zeros(4, dtype=torch.uint8, device="cuda"),
                      _dev(torch, handles), out.image(GUARD + 600), gap=0)
    assert _np(st).tolist() == [0, 2, 0, 1]  # LSBM_BUILD_BAD_INPUT, LSBM_BUILD_NO_ROOM
    got = out.get(GUARD, 600)
    assert got[:50] == data[:50] and got[200:250] == data[120:170]
    assert got[50:200] == bytes([FILL]) * 150 and got[250:] == bytes([FILL]) * 350


# --------------------------------------------------------------------------- GPU: merge
def gpu_merge(torch, arena, case, bases, arrays, drop, exact):
    from lsbm_amd import merge
    keys = arena.image(arena.size_for(case, bases, "keys", exact))
    ko = _dev(torch, arrays["key_offsets"])
    p = merge.plan(keys, ko, _dev(torch, arrays["run_first"]), cmp=bm.INTERNAL_KEY, drop=drop,
                   smallest_snapshot=15 if drop else None, bottom_level=True)
    n = ko.numel() - 1
    out_keys = torch.full((len(case.bufs["keys"]) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    g = merge.gather(keys, ko, _dev(torch, arrays["values"]), p, out_keys=out_keys[:len(case.bufs["keys"]) - 1])
    n_out, nbytes = (int(x) for x in p.counts.cpu())
    ok = out_keys.cpu().numpy()
    assert (ok[nbytes:] == 0xAB).all() and g.key_offsets.numel() == n + 1
    assert _np(g.key_offsets)[:n_out + 1].tolist() == _np(p.out_key_offsets)[:n_out + 1].tolist()
    return {"source": _np(p.source)[:n_out], "out_key_offsets": _np(p.out_key_offsets)[:n_out + 1],
            "counts": _np(p.counts), "run_status": _np(p.run_status), "out_keys": ok[:nbytes].tobytes(),
            "out_values": _np(g.values).reshape(-1, 2)[:n_out], "gather_status": _np(g.status)}


@pytest.mark.gpu
def test_gpu_merge_past_4gib(torch_cuda, arenas, merge_case):
    torch, (arena, _) = torch_cuda, arenas
    case = merge_case
    ko = case.arrays["key_offsets"]
    # inside a user key; inside 8-byte tags, so that the tag's load straddles
    # the line (at entry 130, and at 3 of 8 bytes into the first run's last tag)
    cuts = {"keys": [int(ko[40]) + 2, int(ko[131]) - 4, int(ko[100]) - 5, int(ko[257]) - 1]}
    base0 = {d: ho.merge_model(case.bufs, case.arrays, d) for d in (False, True)}
    for name, bases, exact in placements(case, cuts):
        if name == "vimage":  # no value byte is read: the slices only pass through
            bases = {"keys": LINE + 4099, "vimage": LINE + (1 << 25) + 1}
        arena.place(case, {"keys": bases["keys"]})
        arrays = ho.rebase(case, bases)
        for drop in (False, True):
            want = ho.shift_outputs(base0[drop], ho.MERGE_SHIFTS, bases)
            got = gpu_merge(torch, arena, case, bases, arrays, drop, exact)
            ho.assert_same(got, want, (name, hex(bases[name]), drop, exact))
        if name == "vimage":
            break


@pytest.mark.gpu
def test_gpu_merge_rejects_offset_past_small_buffer(torch_cuda, arenas, merge_case):
    """The last key offset at x + 2^32 over a key buffer of a few KiB: the run
    that holds it is LSBM_MERGE_BAD_INPUT, the others are not."""
    from lsbm_amd import merge
    torch, (arena, _) = torch_cuda, arenas
    case = merge_case
    arena.put(0, case.bufs["keys"])
    ko = case.arrays["key_offsets"].copy()
    ko[-1] += LINE
    p = merge.plan(arena.image(len(case.bufs["keys"])), _dev(torch, ko), _dev(torch, case.arrays["run_first"]))
    assert _np(p.run_status).tolist() == [0, 0, merge.MERGE_BAD_INPUT]
    assert _np(p.counts).tolist()[0] == 0


# --------------------------------------------------------------------------- the later engines' cases
@pytest.fixture(scope="module")
def memtable_case():
    return ho.memtable_case()


@pytest.fixture(scope="module")
def sort_case():
    return ho.sort_case()


@pytest.fixture(scope="module")
def build_case():
    return ho.build_case()


@pytest.fixture(scope="module")
def get_case():
    return ho.get_case()


@pytest.fixture(scope="module")
def scan_case():
    from test_scan_gpu import tile_edge_history
    return ho.scan_case(tile_edge_history())


def test_memtable_models_are_position_independent_and_decoy_differs(memtable_case, sort_case):
    case = memtable_case
    base0 = ho.memtable_model(case.bufs, case.arrays)
    bases = {"image": 37, "kout": 1000}
    moved = ho.memtable_model(ho.host_images(case, bases), ho.rebase(case, bases))
    moved["key_offsets"] = moved["key_offsets"] + bases["kout"]  # (the window's start: the caller's key_base[0])
    ho.assert_same(moved, ho.shift_outputs(base0, ho.MEMTABLE_SHIFTS, bases), "memtable")
    ho.assert_all_differ(base0, ho.memtable_model(case.decoy, case.arrays), "memtable")
    assert base0["status"].tolist() == [ho.mt.OK, ho.mt.BAD_PUT, ho.mt.WRONG_COUNT, ho.mt.OK]
    base0 = check_position_independent(sort_case, ho.sort_model, ho.SORT_SHIFTS, "sort")
    differ_but(base0, ho.sort_model(sort_case.decoy, sort_case.arrays), ho.SORT_LAYOUT_ONLY, "sort")


def test_build_model_is_position_independent_and_decoy_differs(build_case):
    base0 = check_position_independent(build_case, ho.build_model, ho.BUILD_SHIFTS, "build")
    differ_but(base0, ho.build_model(build_case.decoy, build_case.arrays), ho.BUILD_LAYOUT_ONLY, "build")
    assert len(base0["blocks"]) == 16 and base0["table_block_first"].tolist() == [0, 8, 16]


def test_get_model_is_position_independent_and_decoy_differs(get_case):
    base0 = check_position_independent(get_case, ho.get_model, ho.GET_SHIFTS, "get")
    differ_but(base0, ho.get_model(get_case.decoy, get_case.arrays), ho.GET_LAYOUT_ONLY, "get")
    gm = ho.gm
    assert {gm.FOUND, gm.DELETED, gm.UNDECIDED} <= set(base0["mem_verdict"].tolist())
    assert {gm.FOUND, gm.DELETED, gm.UNDECIDED, gm.CORRUPT, gm.ERROR + gm.BAD_CHECKSUM} <= set(
        base0["save_verdict"].tolist())
    assert (base0["file"] >= 0).any(axis=0).all() and (base0["file"] < 0).any()


def test_scan_model_is_position_independent_and_decoy_differs(scan_case):
    for s in ho.SCAN_SNAPSHOTS:
        model = lambda im, ar: ho.scan_model(im, ar, s)  # noqa: E731
        base0 = check_position_independent(scan_case, model, ho.SCAN_SHIFTS, s)
        differ_but(base0, model(scan_case.decoy, scan_case.arrays), ho.SCAN_LAYOUT_ONLY, s)
        assert base0["forward_status"].any() and base0["counts"][0] > 100


# --------------------------------------------------------------------------- GPU: memtable
def gpu_memtable(torch, arena, out, case, bases, arrays, want, exact, note):
    from lsbm_amd import memtable
    img = arena.image(arena.size_for(case, bases, "image", exact))
    rec = _dev(torch, arrays["records"])
    counts, status = memtable.scan(img, rec)
    c, kout = want["counts"], bases["kout"]
    entry_base = np.concatenate([[0], np.cumsum(c[:, 0])])
    key_base = kout + np.concatenate([[0], np.cumsum(c[:, 1] + 8 * c[:, 0])])
    ne, nk = int(entry_base[-1]), int(key_base[-1] - kout)
    g = Guarded(out)
    g.window(kout, nk)
    g.prefill()
    koff = torch.full((ne + 1 + 16,), -2, dtype=torch.int64, device="cuda")
    vals = torch.full((2 * ne + 32,), -2, dtype=torch.int64, device="cuda")
    d = memtable.decode(img, rec, _dev(torch, entry_base), _dev(torch, key_base),
                        keys=out.image(kout + nk if exact else ARENA_BYTES), key_offsets=koff[8:8 + ne + 1],
                        values=vals[16:16 + 2 * ne])
    assert _np(d.status).tolist() == _np(status).tolist()
    g.verify([(kout, want["keys"])], note)
    kh, vh = koff.cpu().numpy(), vals.cpu().numpy()
    assert (kh[:8] == -2).all() and (kh[8 + ne + 1:] == -2).all()
    assert (vh[:16] == -2).all() and (vh[16 + 2 * ne:] == -2).all()
    return {"counts": _np(counts), "status": _np(status), "keys": out.get(kout, nk), "key_offsets": kh[8:8 + ne + 1],
            "values": vh[16:16 + 2 * ne].reshape(-1, 2),
            "max_sequence": np.array([memtable.max_sequence_of(d.max_sequence)], dtype=np.int64)}


@pytest.mark.gpu
def test_gpu_memtable_scan_decode_past_4gib(torch_cuda, arenas, memtable_case):
    torch, (arena, out) = torch_cuda, arenas
    case = memtable_case
    base0 = ho.memtable_model(case.bufs, case.arrays)
    rec = case.arrays["records"]
    _, calls = ho.mt.walk(case.bufs["image"], int(rec[0]), int(rec[1]))
    # inside the 12-byte batch header; inside a key that is copied by 8-byte
    # words; inside the record with the bad Put
    cuts = [int(rec[0]) + 5, calls[1][1] + 3, int(rec[2]) + 20, int(rec[6]) + 1]
    nk = len(base0["keys"])
    runs = [({"image": b, "kout": LINE + 3 * 4096 + 5}, i == 0)
            for i, b in enumerate(ho.bases_for(len(case.bufs["image"]), cuts))]
    # the key windows across the line in the output arena: inside a copied key
    runs += [({"image": LINE + 4099, "kout": k}, k == LINE - nk) for k in (LINE - 20, LINE - nk // 2, LINE - nk, LINE)]
    for bases, exact in runs:
        arena.place(case, {"image": bases["image"]})
        want = ho.shift_outputs(base0, ho.MEMTABLE_SHIFTS, bases)
        got = gpu_memtable(torch, arena, out, case, bases, ho.rebase(case, bases), want, exact,
                           (hex(bases["image"]), hex(bases["kout"])))
        ho.assert_same(got, want, (hex(bases["image"]), hex(bases["kout"]), exact))
    assert len(runs) >= 10


@pytest.mark.gpu
def test_gpu_memtable_sort_past_4gib(torch_cuda, arenas, sort_case):
    from lsbm_amd import memtable
    torch, (arena, _) = torch_cuda, arenas
    case = sort_case
    want = ho.sort_model(case.bufs, case.arrays)
    ko = case.arrays["key_offsets"]
    # inside the first 8-byte word of a user key, inside a tag, one byte before the end
    cuts = {"keys": [int(ko[50]) + 3, int(ko[200]) - 5, int(ko[128]) + 7, int(ko[257]) - 1]}
    for name, bases, exact in placements(case, cuts):
        arena.place(case, bases)
        arrays = ho.rebase(case, bases)
        p = memtable.sort(arena.image(arena.size_for(case, bases, "keys", exact)), _dev(torch, arrays["key_offsets"]))
        got = {"source": _np(p.source), "out_key_offsets": _np(p.out_key_offsets), "counts": _np(p.counts),
               "status": _np(p.run_status)}
        ho.assert_same(got, want, (hex(bases["keys"]), exact))


@pytest.mark.gpu
def test_gpu_memtable_rejects_offsets_past_small_images(torch_cuda, arenas, memtable_case, sort_case):
    from lsbm_amd import memtable, merge
    torch, (arena, _) = torch_cuda, arenas
    case = memtable_case
    arena.put(0, case.bufs["image"])
    want = ho.memtable_model(case.bufs, case.arrays)
    rec = case.arrays["records"].copy()
    rec[6] += LINE
    counts, status = memtable.scan(arena.image(len(case.bufs["image"])), _dev(torch, rec))
    assert _np(status).tolist() == want["status"].tolist()[:3] + [ho.mt.BAD_INPUT]
    assert _np(counts)[:3].tolist() == want["counts"][:3].tolist() and _np(counts)[3].tolist() == [0, 0]
    case = sort_case
    arena.put(0, case.bufs["keys"])
    ko = case.arrays["key_offsets"].copy()
    ko[-1] += LINE
    p = memtable.sort(arena.image(len(case.bufs["keys"])), _dev(torch, ko))
    assert _np(p.run_status).tolist() == [merge.MERGE_BAD_INPUT] and _np(p.counts).tolist() == [0, 0]


# --------------------------------------------------------------------------- GPU: block and index builder
def gpu_build(torch, arena, out, case, bases, arrays, base0, out_pos, exact, note):
    from lsbm_amd import block_build
    keys = arena.image(arena.size_for(case, bases, "keys", exact))
    vimage = arena.image(arena.size_for(case, bases, "vimage", exact))
    ko, values = _dev(torch, arrays["key_offsets"]), _dev(torch, arrays["values"])
    p = block_build.plan(keys, ko, values, _dev(torch, arrays["table_first"]), ho.BUILD_BLOCK_SIZE, ho.BUILD_RESTART)
    nb = int(base0["table_block_first"][-1])
    got = {"block_first": _np(p.block_first)[:nb + 1], "block_bytes": _np(p.block_bytes)[:nb],
           "table_block_first": _np(p.table_block_first), "plan_status": _np(p.status)}
    sizes = base0["block_bytes"]
    pos = out_pos + np.concatenate([[0], np.cumsum(sizes + 7)[:-1]])  # (windows 7 bytes apart)
    handles = np.stack([pos, sizes], 1).reshape(-1)
    # the index entries name these windows: handles past 4 GiB in the varints
    want = ho.build_model(case.bufs, case.arrays, data_handles=handles)
    ipos = int(pos[-1] + sizes[-1]) + 9 + np.array([0, int(want["index_bytes"][0]) + 5])
    ihandles = np.stack([ipos, want["index_bytes"]], 1).reshape(-1)
    g = Guarded(out)
    for a, n in list(zip(pos, sizes)) + list(zip(ipos, want["index_bytes"])):
        g.window(int(a), int(n))
    g.prefill()
    size = int(ipos[-1] + want["index_bytes"][-1]) if exact else ARENA_BYTES
    built, st = block_build.build(keys, ko, values, vimage, p.block_first[:nb + 1].contiguous(), out.image(size),
                                  _dev(torch, handles), ho.BUILD_RESTART)
    ibuilt, ist = block_build.index_block(keys, ko, p.block_first[:nb + 1].contiguous(), p.table_block_first,
                                          _dev(torch, handles), cmp=bm.INTERNAL_KEY, out=out.image(size),
                                          out_handles=_dev(torch, ihandles))
    torch.cuda.synchronize()
    g.verify([(int(a), b) for a, b in zip(pos, want["blocks"])] +
             [(int(a), b) for a, b in zip(ipos, want["index_blocks"])], note)
    got.update({"blocks": [out.get(int(a), int(n)) for a, n in zip(pos, sizes)], "built_bytes": _np(built),
                "build_status": _np(st),
                "index_blocks": [out.get(int(a), int(n)) for a, n in zip(ipos, want["index_bytes"])],
                "index_bytes": _np(ibuilt), "index_status": _np(ist)})
    return got, want


@pytest.mark.gpu
def test_gpu_block_builder_past_4gib(torch_cuda, arenas, build_case):
    torch, (arena, out) = torch_cuda, arenas
    case = build_case
    base0 = ho.build_model(case.bufs, case.arrays)
    ko, v = case.arrays["key_offsets"], case.arrays["values"].reshape(-1, 2)
    # inside a key, between two keys of one block; inside a value (the 150-byte one of entry 9)
    cuts = {"keys": [int(ko[20]) + 5, int(ko[21]), int(ko[140]) + 9], "vimage": [int(v[9, 0]) + 70, int(v[30, 0]) + 1]}
    for name, bases, exact in placements(case, cuts):
        arena.place(case, bases)
        got, want = gpu_build(torch, arena, out, case, bases, ho.rebase(case, bases), base0, LINE + 5 * 4096 + 3, exact,
                              (name, hex(bases[name])))
        ho.assert_same(got, want, (name, hex(bases[name]), exact))
        for k in ("blocks", "block_first", "block_bytes", "built_bytes"):  # byte-identical to base 0
            assert ho.same(got[k], base0[k]), k
    bases = parked(case, None)
    arena.place(case, bases)
    first = int(base0["block_bytes"][0])
    for pos in (LINE - first // 2, LINE - first - 3, LINE - 5000, LINE):  # the line inside a block as it is written
        got, want = gpu_build(torch, arena, out, case, bases, ho.rebase(case, bases), base0, pos, False, ("out", hex(pos)))
        ho.assert_same(got, want, ("out", hex(pos)))


@pytest.mark.gpu
def test_gpu_block_builder_rejects_offsets_past_small_images(torch_cuda, arenas, build_case):
    from lsbm_amd import block_build
    torch, (arena, out) = torch_cuda, arenas
    case = build_case
    arena.put(0, case.bufs["keys"])
    arena.put(1 << 20, case.bufs["vimage"])
    base0 = ho.build_model(case.bufs, case.arrays)
    keys = arena.image(len(case.bufs["keys"]))
    ko = _dev(torch, case.arrays["key_offsets"])
    v = case.arrays["values"].copy()
    v[0::2] += 1 << 20
    v[2 * 20] += LINE  # entry 20, in block 1: its value slice is x + 2^32
    sizes = base0["block_bytes"]
    pos = GUARD + np.concatenate([[0], np.cumsum(sizes + 7)[:-1]])
    handles = np.stack([pos, sizes], 1).reshape(-1)
    handles[2 * 3] += LINE  # block 3's window is x + 2^32
    g = Guarded(out)
    g.window(GUARD, int(pos[-1] + sizes[-1]) - GUARD)
    g.prefill()
    built, st = block_build.build(keys, ko, _dev(torch, v), arena.image((1 << 20) + len(case.bufs["vimage"])),
                                  _dev(torch, base0["block_first"]), out.image(int(pos[-1] + sizes[-1])),
                                  _dev(torch, handles), ho.BUILD_RESTART)
    want = [0] * 16
    want[1] = want[3] = 2  # LSBM_BUILD_BAD_INPUT: "a value slice is not wholly inside the value image", "a window is not wholly inside the output"
    assert _np(st).tolist() == want
    for b in (0, 2, 4, 15):
        assert out.get(int(pos[b]), int(sizes[b])) == base0["blocks"][b]
    for b in (1, 3):  # "Nothing is written for that block"
        assert out.get(int(pos[b]), int(sizes[b])) == bytes([FILL]) * int(sizes[b])
    ko2 = case.arrays["key_offsets"].copy()
    ko2[-1] += LINE
    p = block_build.plan(keys, _dev(torch, ko2), _dev(torch, case.arrays["values"]),
                         _dev(torch, case.arrays["table_first"]), ho.BUILD_BLOCK_SIZE, ho.BUILD_RESTART)
    assert _np(p.status).tolist() == [0, 2]
    assert _np(p.block_first)[:8].tolist() == base0["block_first"][:8].tolist()


# --------------------------------------------------------------------------- GPU: Get
def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def gpu_get(torch, arena, out, case, bases, arrays, want, exact, note):
    from lsbm_amd import _lib, db
    gm = ho.gm
    L = _lib.lib()
    stream = _ptr_stream(torch)
    n = arrays["user_offsets"].size - 1
    size = lambda name: arena.size_for(case, bases, name, exact)  # noqa: E731
    uo = arrays["user_offsets"]
    # LookupKey: key q lands at d_user_offsets[q] + 8q of the output, so past 4 GiB by construction
    start, cap = int(uo[0]), int(uo[-1]) + 8 * n
    g = Guarded(out)
    g.window(start, cap - start)
    g.prefill()
    d_uo = _dev(torch, uo)
    lk_off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = L.lsbm_lookup_keys_dev(_ptr(arena.t), size("users"), _ptr(d_uo), n, ho.GET_SNAPSHOT, None, _ptr(out.t),
                                cap - 1, _ptr(lk_off), _ptr(st), stream)
    assert rc == 0 and _np(st).tolist() == [2] and (_np(lk_off) == -7).all()  # one byte short: nothing is written
    g.verify([], note + ("short",))
    rc = L.lsbm_lookup_keys_dev(_ptr(arena.t), size("users"), _ptr(d_uo), n, ho.GET_SNAPSHOT, None, _ptr(out.t),
                                cap, _ptr(lk_off), _ptr(st), stream)
    assert rc == 0
    g.verify([(start, want["lookup_keys"])], note + ("lookup",))
    got = {"lookup_keys": out.get(start, cap - start), "lookup_offsets": _np(lk_off), "lookup_status": _np(st)}
    if start >= LINE:  # the calls below read these keys at offsets past 4 GiB: their decoy, 2^32 lower
        decoy_users = ho.split_keys(case.decoy["users"], case.arrays["user_offsets"])
        out.put(start - LINE, b"".join(gm.lookup_key(u, ho.GET_SNAPSHOT) for u in decoy_users))
    lkeys = out.image(cap)
    # MemTable::Get
    from collections import namedtuple
    mem = namedtuple("Mem", "keys key_offsets values")(arena.image(size("mem")), _dev(torch, arrays["mem_offsets"]),
                                                       _dev(torch, arrays["mem_values"]))
    verdict, value, where = db.new_verdicts(n, "cuda")
    st = db.memtable_probe(mem, lkeys, lk_off, ho.GET_SOURCE, verdict, value, where)
    assert _np(st).tolist() == [0]
    got.update({"mem_verdict": _np(verdict), "mem_value": _np(value), "mem_where": _np(where)})
    # the file pick
    file, st = db.find_file(arena.image(size("bounds")), _dev(torch, arrays["bound_offsets"]),
                            _dev(torch, ho.GET_RUN_FIRST), torch.tensor(ho.GET_RUN_FLAGS, dtype=torch.int32, device="cuda"),
                            torch.tensor([1, 1, 0, 1, 1, 1, 1, 0], dtype=torch.uint8, device="cuda"), lkeys, lk_off)
    assert _np(st).tolist() == [0]
    got["file"] = _np(file)
    # SaveValue over one round of reads, from fresh verdicts
    verdict, value, where = db.new_verdicts(n, "cuda")
    st = db.save_value(torch.tensor(arrays["state"], dtype=torch.int32, device="cuda"), _dev(torch, arrays["key_len"]),
                       arena.image(size("found")), _dev(torch, arrays["found_offsets"]), _dev(torch, arrays["value_in"]),
                       lkeys, lk_off, ho.GET_SOURCE + 1, verdict, value, where)
    assert _np(st).tolist() == [0]
    got.update({"save_verdict": _np(verdict), "save_value": _np(value), "save_where": _np(where)})
    # the values, gathered to windows past 4 GiB in the output arena
    lens = [len(b) for b in want["gathered"]]
    opos = bases["gather_out"] + np.concatenate([[0], np.cumsum(lens)])
    g = Guarded(out)
    g.window(int(opos[0]), int(opos[-1] - opos[0]))
    g.prefill()
    st = db.slices_gather(arena.image(size("vimage")), value.reshape(-1), where, ho.GET_SOURCE + 1, ho.GET_SOURCE + 2,
                          out.image(int(opos[-1]) if exact else ARENA_BYTES), _dev(torch, opos))
    assert _np(st).tolist() == [0]
    g.verify([(int(opos[0]), b"".join(want["gathered"]))], note + ("gather",))
    got["gathered"] = [out.get(int(opos[q]), lens[q]) for q in range(n)]
    return got


def _ptr_stream(torch):
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.gpu
def test_gpu_get_past_4gib(torch_cuda, arenas, get_case):
    torch, (arena, out) = torch_cuda, arenas
    case = get_case
    base0 = ho.get_model(case.bufs, case.arrays)
    a = case.arrays
    cuts = {"users": [int(a["user_offsets"][30]) + 3], "mem": [int(a["mem_offsets"][45]) + 2, int(a["mem_offsets"][46]) - 4],
            "bounds": [int(a["bound_offsets"][7]) - 3], "found": [int(a["found_offsets"][33]) + 5],
            "vimage": [1200]}
    n = 0
    for name, bases, exact in placements(case, cuts):
        arena.place(case, bases)
        bases = dict(bases, gather_out=LINE - 100 if name == "vimage" else LINE + 7 * 4096 + 1)
        want = ho.shift_outputs(base0, ho.GET_SHIFTS, bases)
        got = gpu_get(torch, arena, out, case, bases, ho.rebase(case, bases), want, exact, (name, hex(bases[name])))
        ho.assert_same(got, want, (name, hex(bases[name]), exact))
        n += 1
    assert n >= 5 * 4


@pytest.mark.gpu
def test_gpu_get_rejects_offsets_past_small_buffers(torch_cuda, arenas, get_case):
    from lsbm_amd import db
    torch, (arena, out) = torch_cuda, arenas
    case = get_case
    a = case.arrays
    base0 = ho.get_model(case.bufs, case.arrays)
    n = a["user_offsets"].size - 1
    arena.put(0, case.bufs["vimage"])
    arena.put(1 << 20, case.bufs["users"])
    # slices_gather: "a selected slice that is not inside the image ... such a query is not copied, the others are"
    where = torch.tensor(base0["save_where"], dtype=torch.int32, device="cuda")
    slices = base0["save_value"].copy()
    hit = int(np.nonzero((base0["save_where"] >= 0) & (slices[:, 1] > 0))[0][2])
    slices[hit, 0] += LINE
    lens = [len(b) for b in base0["gathered"]]
    opos = GUARD + np.concatenate([[0], np.cumsum(lens)])
    g = Guarded(out)
    g.window(GUARD, int(opos[-1]) - GUARD)
    g.prefill()
    st = db.slices_gather(arena.image(len(case.bufs["vimage"])), _dev(torch, slices.reshape(-1)), where,
                          ho.GET_SOURCE + 1, ho.GET_SOURCE + 2, out.image(int(opos[-1])), _dev(torch, opos))
    assert _np(st).tolist() == [2]  # LSBM_MERGE_BAD_INPUT
    for q in range(n):
        want = base0["gathered"][q] if q != hit else bytes([FILL]) * lens[q]
        assert out.get(int(opos[q]), lens[q]) == want, q
    # the key-offset checks: the last user offset at x + 2^32 over a buffer of a few hundred bytes
    uo = a["user_offsets"] + (1 << 20)
    uo[-1] += LINE
    from lsbm_amd import _lib
    cap = int(uo[-1]) + 8 * n  # (inside the output arena: whatever a wrong check lets through lands in it)
    g = Guarded(out)
    g.window(1 << 20, len(case.bufs["users"]) + 8 * n)
    g.prefill()
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = _lib.lib().lsbm_lookup_keys_dev(_ptr(arena.t), (1 << 20) + len(case.bufs["users"]), _ptr(_dev(torch, uo)), n,
                                         ho.GET_SNAPSHOT, None, _ptr(out.t), cap, _ptr(off), _ptr(st),
                                         _ptr_stream(torch))
    assert rc == 0 and _np(st).tolist() == [2] and (_np(off) == -7).all()
    assert out.get((1 << 20) - GUARD, len(case.bufs["users"]) + 8 * n + 2 * GUARD).count(FILL) == \
        len(case.bufs["users"]) + 8 * n + 2 * GUARD


# --------------------------------------------------------------------------- GPU: scans
def gpu_scan(torch, arena, case, bases, arrays, snapshot, exact):
    from lsbm_amd import scan
    size = lambda name: arena.size_for(case, bases, name, exact)  # noqa: E731
    v = scan.view(arena.image(size("keys")), _dev(torch, arrays["key_offsets"]), _dev(torch, arrays["values"]),
                  arena.image(size("vimage")), snapshot)
    ny = v.n_yield
    p = v.plan
    got = {"live": _np(p.source)[:ny], "yield_rank": _np(p.yield_rank), "corrupt_rank": _np(p.corrupt_rank),
           "first": _np(p.first)[:ny], "back": _np(p.back)[:ny], "counts": _np(p.counts),
           "live_values": _np(v.live_values).reshape(-1, 2)}
    u8 = lambda x: torch.tensor(np.asarray(x, dtype=np.uint8), device="cuda")  # noqa: E731
    for reverse in (False, True):
        r = v.scan(arena.image(size("lo")), _dev(torch, arrays["lo_offsets"]), arena.image(size("hi")),
                   _dev(torch, arrays["hi_offsets"]), limit=_dev(torch, arrays["limits"]), reverse=reverse,
                   lo_present=u8(arrays["lo_present"]), hi_present=u8(arrays["hi_present"]))
        tag = "reverse" if reverse else "forward"
        got.update({tag + "_status": _np(r.status), tag + "_entry_first": _np(r.entry_first),
                    tag + "_keys": r.keys.cpu().numpy().tobytes(), tag + "_key_offsets": _np(r.key_offsets),
                    tag + "_values": r.values.cpu().numpy().tobytes(), tag + "_value_offsets": _np(r.value_offsets)})
    return got


@pytest.mark.gpu
def test_gpu_scans_past_4gib(torch_cuda, arenas, scan_case):
    torch, (arena, _) = torch_cuda, arenas
    case = scan_case
    base0 = {s: ho.scan_model(case.bufs, case.arrays, s) for s in ho.SCAN_SNAPSHOTS}
    ko, v = case.arrays["key_offsets"], case.arrays["values"].reshape(-1, 2)
    # inside a user key, inside tags at the tile edges (entries 255 | 256, 511 | 512), inside an emitted value
    cuts = {"keys": [int(ko[50]) + 2, int(ko[256]) - 4, int(ko[512]) - 3],
            "vimage": [int(v[40, 0]) + 1, int(v[768, 0])], "lo": [int(case.arrays["lo_offsets"][4]) + 1],
            "hi": [int(case.arrays["hi_offsets"][1]) + 1]}
    for name, bases, exact in placements(case, cuts):
        arena.place(case, bases)
        arrays = ho.rebase(case, bases)
        for s in ho.SCAN_SNAPSHOTS if name == "keys" else ho.SCAN_SNAPSHOTS[:1]:
            want = ho.shift_outputs(base0[s], ho.SCAN_SHIFTS, bases)
            ho.assert_same(gpu_scan(torch, arena, case, bases, arrays, s, exact), want, (name, hex(bases[name]), s, exact))


@pytest.mark.gpu
def test_gpu_scans_reject_offset_past_small_buffer(torch_cuda, arenas, scan_case):
    from lsbm_amd import merge, scan
    torch, (arena, _) = torch_cuda, arenas
    case = scan_case
    arena.put(0, case.bufs["keys"])
    ko = case.arrays["key_offsets"].copy()
    ko[-1] += LINE
    p = scan.plan(arena.image(len(case.bufs["keys"])), _dev(torch, ko), 3)
    assert _np(p.status).tolist() == [merge.MERGE_BAD_INPUT] and _np(p.counts).tolist() == [0, 0, 0]
    # a query's bound at x + 2^32 over a bound buffer of a few dozen bytes
    arena.put(1 << 20, case.bufs["vimage"])
    values = case.arrays["values"].copy()
    values[0::2] += 1 << 20
    v = scan.view(arena.image(len(case.bufs["keys"])), _dev(torch, case.arrays["key_offsets"]), _dev(torch, values),
                  arena.image((1 << 20) + len(case.bufs["vimage"])), 3)
    arena.put(2 << 20, case.bufs["lo"])
    lo_off = case.arrays["lo_offsets"] + (2 << 20)
    lo_off[-1] += LINE
    r = v.range(arena.image((2 << 20) + len(case.bufs["lo"])), _dev(torch, lo_off))
    assert _np(r.call_status).tolist() == [merge.MERGE_BAD_INPUT]


# --------------------------------------------------------------------------- GPU: what a dropped high half reads
@pytest.mark.gpu
def test_gpu_truncated_offsets_read_the_decoy(torch_cuda, arenas, block_case, merge_case):
    """The placement does what it is for: offsets with their high half dropped
    on purpose (B - 2^32 in place of B) read the decoy, whose answer is
    well-formed and no array of which equals the payload's."""
    torch, (arena, out) = torch_cuda, arenas
    mode = BLOCK_MODES[1]
    for case, model, run, shifts, skip in (
            (block_case, lambda im, ar: ho.block_model(im, ar, *mode),
             lambda c, b, ar, w: gpu_block(torch, arena, out, c, b, ar, mode[0], mode[1], w, False), ho.BLOCK_SHIFTS,
             ho.BLOCK_LAYOUT_ONLY_WITHOUT_FLAG),
            (merge_case, lambda im, ar: ho.merge_model(im, ar, True),
             lambda c, b, ar, w: gpu_merge(torch, arena, c, b, ar, True, False), ho.MERGE_SHIFTS,
             ho.MERGE_LAYOUT_ONLY)):
        bases = parked(case, None)
        arena.place(case, bases)
        low = {k: v - LINE for k, v in bases.items()}
        want_decoy = ho.shift_outputs(model(case.decoy, case.arrays), shifts, low)
        got = run(case, low, ho.rebase(case, low), want_decoy)
        ho.assert_same(got, want_decoy, "decoy")
        differ_but(got, ho.shift_outputs(model(case.bufs, case.arrays), shifts, bases), skip, "payload")
