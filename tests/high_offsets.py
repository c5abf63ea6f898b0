"""Rebasing helper of tests/test_high_offsets.py: small cases of every engine,
placed at offsets past 4 GiB in a sparse arena.

A Case is a handful of input buffers (a few hundred bytes to a few KiB each),
the int64 offset arrays that point into them, and a decoy: a second
well-formed set of buffers of the same sizes with different contents.  A
kernel that drops the high half of an offset at base B reads the decoy at
B - 2^32 and so returns a valid, wrong answer.

    rebase(case, bases)        the offset arrays with bases[buffer] added
    host_images(case, bases)   the buffers behind `bases[buffer]` filler bytes:
                               what a model reads to prove that it is
                               position-independent
    shift_outputs(...)         base-0 outputs moved by the per-output table

The per-output tables (SHIFTS) say, per entry point and output array, which
input buffer's base the output moves by, or None where it must be identical
to the base-0 run.  They are taken from the headers' wording:

    lsbm_block.h       d_values / d_value: "{absolute offset in the image,
                       length}" -> the image's base on the offset slot of
                       entries that were found; d_pos is "the found entry's
                       offset in the block", counts / status / key lengths /
                       decoded handles / found keys do not move
    lsbm_snappy.h      lengths, ok flags and bytes only: nothing moves
    lsbm_bloom.h       may bytes and filter bytes only: nothing moves
    lsbm_table_pack.h  d_handles "offset[i] = first_offset + ..." and d_end
                       move with first_offset; types and moved bytes do not
    lsbm_merge.h       d_source, counts, statuses and the output's own key
                       offsets do not move; gather's d_out_values are "copied
                       from the source entry": they move with the value
                       image's base
    lsbm_block_build.h entry numbers, sizes, statuses and block bytes: nothing
                       moves (the index entries encode the d_data_handles the
                       caller passes, which are inputs)
    lsbm_memtable.h    d_values "{offset of the value bytes in the image,
                       length}; for a deletion length 0 and the offset just
                       past the key" move with the image on every offset slot;
                       d_key_offsets index d_keys from d_key_base[0] on, so
                       they move with the key window the caller chose, not
                       with the image; sort's outputs do not move
    lsbm_get.h         "d_key_offsets[q] = d_user_offsets[q] + 8q" moves with
                       the user keys' base; a found query's value slice is the
                       entry's or the read's, so its offset moves with the
                       value image ({0, 0} of a deletion does not); verdicts,
                       where words, file indices and gathered bytes do not
    lsbm_iter.h        positions, ranks, counts, statuses and the emitted
                       bytes with their running offsets do not move; the live
                       value slices are lsbm_merge_gather_dev's

An output that the offset arrays alone decide (a count of entries, a status
that is OK for any well-formed input, a running sum of key lengths) is the
same for every decoy of the same layout; the *_LAYOUT_ONLY tuples name them,
and the decoy-differs assertions leave exactly those out.
"""
import numpy as np

from golden import blockmodel as bm
from golden import buildmodel as bd
from golden import getmodel as gm
from golden import memtable_cases as mc
from golden import memtablemodel as mt
from golden import mergemodel as mm
from golden import scanmodel as sm

LINE = 1 << 32
ARENA_BYTES = LINE + (1 << 26)
GUARD = 4096
FILL = 0xEE


class Case:
    """bufs / decoy: name -> bytes (same lengths); arrays: name -> int64 numpy
    array; addr: array name -> (buffer name, "all" | "pairs"): every slot, or
    the even slots ({offset, size} pairs), holds an offset into that buffer."""

    def __init__(self, bufs, decoy, arrays, addr, extra=None):
        assert set(bufs) == set(decoy) and all(len(bufs[k]) == len(decoy[k]) for k in bufs)
        assert all(bufs[k] != decoy[k] for k in bufs if len(bufs[k]))
        self.bufs, self.decoy, self.addr = dict(bufs), dict(decoy), dict(addr)
        self.arrays = {k: np.asarray(v, dtype=np.int64).copy() for k, v in arrays.items()}
        self.extra = dict(extra or {})


def _moved(a, how, delta):
    a = a.copy()
    if how == "all":
        a += delta
    elif how == "pairs":
        a.reshape(-1)[0::2] += delta
    else:
        raise ValueError(how)
    return a


def rebase(case, bases):
    """The case's offset arrays with bases[buffer] added wherever they address
    that buffer (a negative base undoes it)."""
    out = {}
    for name, a in case.arrays.items():
        if name in case.addr:
            buf, how = case.addr[name]
            a = _moved(a, how, int(bases.get(buf, 0)))
        out[name] = a.copy()
    return out


def host_images(case, bases, decoy=False):
    src = case.decoy if decoy else case.bufs
    return {k: bytes([FILL]) * int(bases.get(k, 0)) + v for k, v in src.items()}


def shift_outputs(outputs, shifts, bases):
    """Base-0 outputs moved by the table: shifts[name] is None, or (buffer,
    selector) where selector(outputs) is a boolean mask of the slots that hold
    an offset into that buffer."""
    assert set(shifts) == set(outputs), (sorted(shifts), sorted(outputs))
    out = {}
    for name, v in outputs.items():
        rule = shifts[name]
        if rule is None:
            out[name] = v
            continue
        buf, sel = rule
        v = np.asarray(v, dtype=np.int64).copy()
        v[sel(outputs)] += int(bases.get(buf, 0))
        out[name] = v
    return out


def same(a, b):
    if isinstance(a, (bytes, bytearray)) or isinstance(b, (bytes, bytearray)):
        return bytes(a) == bytes(b)
    if isinstance(a, list) or isinstance(b, list):
        return list(a) == list(b)
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((a == b).all())


def assert_same(got, want, note=""):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name in want:
        assert same(got[name], want[name]), (note, name)


def assert_all_differ(a, b, note=""):
    """No compared array is equal between the payload's and the decoy's model
    outputs: a kernel that reads the decoy fails every comparison."""
    assert set(a) == set(b)
    for name in a:
        assert not same(a[name], b[name]), (note, name)


def bases_for(length, cuts):
    """The bases of one buffer: wholly above the line at an odd phase (3 mod
    16), exactly on it, ending on it, and with the line `c` bytes in."""
    out = [LINE + 4099, LINE, LINE - length]
    out += [LINE - int(c) for c in cuts if 0 < int(c) < length]
    seen, uniq = set(), []
    for b in out:
        if b not in seen:
            seen.add(b)
            uniq.append(b)
    return uniq


def keys_buffer(keys):
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(k) for k in keys])
    return b"".join(keys) + b"\0", off


def split_keys(buf, off):
    return [bytes(buf[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


# --------------------------------------------------------------------------- block reader
def _sized_block(size, seed, tagged):
    """A well-formed block of exactly `size` bytes whose entries differ from
    any fixture block's: the last value takes up the slack."""
    rng = np.random.default_rng(seed)
    for n in range(max(1, size // 40), 0, -1):
        ents = []
        for i in range(n):
            k = b"decoy%05d" % (i * 3 + seed % 7)
            if tagged:
                k += ((900 + i) << 8 | 1).to_bytes(8, "little")
            ents.append((k, bytes(rng.integers(65, 91, 5, dtype=np.uint8))))
        for slack_adj in (0, 1, 2):
            base = len(bm.build_block(ents, 4))
            pad = size - base - slack_adj
            if pad < 0:
                break
            trial = ents[:-1] + [(ents[-1][0], ents[-1][1] + b"z" * pad)]
            b = bm.build_block(trial, 4)
            if len(b) == size:
                assert bm.walk(b)[0] == bm.OK
                return b
    raise AssertionError("no decoy block of %d bytes" % size)


def block_case(blocks, tagged, probes):
    """blocks: [bytes]; probes: [(block index, target)].  Buffers: image (the
    blocks back to back at phases 0, 1, 2, ...) and targets."""
    img, dec, handles = bytearray(), bytearray(), []
    for i, b in enumerate(blocks):
        pad = b"\xee" * (1 if i else 0)  # an odd gap: the blocks' phases differ
        img += pad
        dec += pad
        handles += [len(img), len(b)]
        img += b
        dec += _sized_block(len(b), 11 + i, tagged[i])
    tk = b"".join(t for _, t in probes) + b"\0"
    dk = bytes((x + 1) & 255 for x in tk)
    toff = np.zeros(len(probes) + 1, dtype=np.int64)
    toff[1:] = np.cumsum([len(t) for _, t in probes])
    qh = np.array([[handles[2 * b], handles[2 * b + 1]] for b, _ in probes], dtype=np.int64).reshape(-1)
    return Case({"image": bytes(img), "targets": tk}, {"image": bytes(dec), "targets": dk},
                {"handles": handles, "seek_handles": qh, "target_offsets": toff},
                {"handles": ("image", "pairs"), "seek_handles": ("image", "pairs"),
                 "target_offsets": ("targets", "all")})


def block_model(images, arrays, cmp, value_is_handle):
    """scan, decode and seek of include/lsbm_block.h from tests/golden/blockmodel.py."""
    img, tk = images["image"], images["targets"]
    h = arrays["handles"]
    counts, status, keys, koff, values = [], [], b"", [0], []
    for i in range(len(h) // 2):
        blk = img[int(h[2 * i]):int(h[2 * i]) + int(h[2 * i + 1])]
        st, ents = bm.walk(blk)
        counts.append([len(ents), sum(len(e[0]) for e in ents), sum(e[2] for e in ents)])
        status.append(st)
        for k, vo, vl, _ in ents:
            keys += k
            koff.append(len(keys))
            values.append([int(h[2 * i]) + vo, vl])
    qh, to = arrays["seek_handles"], arrays["target_offsets"]
    state, pos, klen, value, handle, found = [], [], [], [], [], []
    for q in range(len(to) - 1):
        blk = img[int(qh[2 * q]):int(qh[2 * q]) + int(qh[2 * q + 1])]
        r = bm.seek(blk, tk[int(to[q]):int(to[q + 1])], cmp, value_is_handle)
        hit = r["state"] in (bm.VALID, bm.SEEK_BAD_HANDLE)
        state.append(r["state"])
        pos.append(r["pos"])
        klen.append(len(r["key"]))
        value.append([int(qh[2 * q]) + r["value_offset"] if hit else 0, r["value_length"]])
        handle.append([x - (1 << 64) if x >= 1 << 63 else x for x in r["handle"]])
        found.append(r["key"])
    return {"counts": np.array(counts, dtype=np.int64).reshape(-1, 3), "status": np.array(status, dtype=np.int64),
            "keys": keys, "key_offsets": np.array(koff, dtype=np.int64),
            "values": np.array(values, dtype=np.int64).reshape(-1, 2),
            "state": np.array(state, dtype=np.int64), "pos": np.array(pos, dtype=np.int64),
            "key_len": np.array(klen, dtype=np.int64), "value": np.array(value, dtype=np.int64).reshape(-1, 2),
            "handle": np.array(handle, dtype=np.int64).reshape(-1, 2), "found": b"".join(found)}


def _offset_slot(name):
    def sel(o):
        m = np.zeros(np.asarray(o[name]).shape, dtype=bool)
        m[:, 0] = True
        return m
    return sel


def _found_offset_slot(o):
    m = np.zeros(np.asarray(o["value"]).shape, dtype=bool)
    m[:, 0] = np.isin(o["state"], (bm.VALID, bm.SEEK_BAD_HANDLE))
    return m


# without LSBM_SEEK_VALUE_IS_HANDLE every d_handle_out pair is {0, 0}, for any block
BLOCK_LAYOUT_ONLY_WITHOUT_FLAG = ("handle",)
BLOCK_SHIFTS = {"counts": None, "status": None, "keys": None, "key_offsets": None,
                "values": ("image", _offset_slot("values")),
                "state": None, "pos": None, "key_len": None, "value": ("image", _found_offset_slot),
                "handle": None, "found": None}


def fixture_block_case():
    """One good block (internal keys), one with a bad entry, one with long
    shared prefixes, from block_fixture.json, and six probes of each."""
    import json
    import os
    from test_block import apply_ops, sampled_targets
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_fixture.json")))
    built = {r["name"]: bytes.fromhex(r["hex"]) for r in fx["built"]}
    mut = {r["name"]: r for r in fx["mutated"]}
    bad = mut["varint5_high_bits_kept"]
    blocks = [built["internal_i3"], apply_ops(built[bad["base"]], bad["ops"]), built["i16_200"]]
    assert [bm.walk(b)[0] for b in blocks] == [bm.OK, bm.BAD_ENTRY, bm.OK]
    probes = []
    for i, b in enumerate(blocks):
        keys = [e[0] for e in bm.walk(built[bad["base"]] if i == 1 else b)[1]]
        probes += [(i, t) for t in sampled_targets(keys, 6)]
    return block_case(blocks, [True, False, False], probes)


# --------------------------------------------------------------------------- snappy
def fixture_snappy_case(snappy_oracle, snappy_golden):
    """An incompressible block, one of long copies and an empty one, from
    snappy_fixture.json's specs."""
    from golden.snappy_inputs import block as snappy_block

    def pick(kind):
        return next(c for c in snappy_golden["cases"] if c["kind"] == kind and 600 <= c["n"] <= 5000)
    rnd, per = pick("random"), pick("period")
    blocks = [snappy_block("random", rnd["n"], rnd["seed"]), snappy_block("period", per["n"], per["seed"]), b""]
    streams = [snappy_oracle.compress(b) for b in blocks]
    assert len(streams[0]) > rnd["n"] and len(streams[1]) < per["n"] // 8
    d_rnd = snappy_block("random", rnd["n"], rnd["seed"] + 1)
    for x in range(1, 256):  # the same copy structure over other bytes: the same compressed length
        d_per = bytes(c ^ x for c in blocks[1])
        if len(snappy_oracle.compress(d_per)) == len(streams[1]):
            break
    dblocks = [d_rnd, d_per, b""]
    return snappy_case(blocks, streams, dblocks, [snappy_oracle.compress(b) for b in dblocks])


def snappy_case(blocks, streams, decoy_blocks, decoy_streams):
    """raw: the blocks to compress; comp: their compressed streams.  The decoy
    has other blocks of the same raw and compressed lengths."""
    assert [len(b) for b in blocks] == [len(b) for b in decoy_blocks]
    assert [len(s) for s in streams] == [len(s) for s in decoy_streams]
    ro = np.zeros(len(blocks) + 1, dtype=np.int64)
    ro[1:] = np.cumsum([len(b) for b in blocks])
    co = np.zeros(len(streams) + 1, dtype=np.int64)
    co[1:] = np.cumsum([len(s) for s in streams])
    return Case({"raw": b"".join(blocks) + b"\0", "comp": b"".join(streams) + b"\0"},
                {"raw": b"".join(decoy_blocks) + b"\1", "comp": b"".join(decoy_streams) + b"\1"},
                {"raw_offsets": ro, "comp_offsets": co},
                {"raw_offsets": ("raw", "all"), "comp_offsets": ("comp", "all")})


def snappy_model(images, arrays, oracle):
    raw, comp = images["raw"], images["comp"]
    ro, co = arrays["raw_offsets"], arrays["comp_offsets"]
    packed = [oracle.compress(raw[int(ro[i]):int(ro[i + 1])]) for i in range(len(ro) - 1)]
    ulen, ok, plain = [], [], []
    for i in range(len(co) - 1):
        s = comp[int(co[i]):int(co[i + 1])]
        good, n = oracle.uncompressed_length(s)
        ulen.append(n)
        ok.append(int(good))
        g2, out = oracle.uncompress(s)
        assert g2 == good
        plain.append(out)
    return {"compressed": packed, "compressed_len": np.array([len(p) for p in packed], dtype=np.int64),
            "ulen": np.array(ulen, dtype=np.int64), "len_ok": np.array(ok, dtype=np.int64),
            "ok": np.array(ok, dtype=np.int64), "plain": plain}


# the lengths are the layout's (a decoy of other lengths would not fit the
# offsets), and every block of payload and decoy is well formed: the bytes are
# what tells the two apart
SNAPPY_LAYOUT_ONLY = ("compressed_len", "ulen", "len_ok", "ok")
SNAPPY_SHIFTS = {"compressed": None, "compressed_len": None, "ulen": None, "len_ok": None, "ok": None,
                 "plain": None}


# --------------------------------------------------------------------------- bloom
def fixture_bloom_case(bloom_oracle):
    def keys(tag, n):
        return [b"%s%04d" % (tag, i * 7) + b"k" * (i % 5) for i in range(n)]
    built, absent = keys(b"in", 70), keys(b"no", 70)
    d_built, d_absent = keys(b"IN", 70), keys(b"NO", 70)
    # probes: the payload asks for its own keys first, the decoy for them last
    return bloom_case(built, d_built, built[:40] + absent[:40], d_absent[:40] + d_built[:40],
                      [0, 1, 30, 70], 10, bloom_oracle)


def bloom_case(keys, decoy_keys, probes, decoy_probes, filter_first, bits_per_key, oracle):
    """keys: what the filters are built from (filter f holds keys
    [filter_first[f], filter_first[f+1])); probes: the lookups; filters: the
    oracle's filters back to back; fblock: the filter block FilterBlockBuilder
    makes of them, one filter per 2 KiB of data offsets."""
    assert [len(k) for k in keys] == [len(k) for k in decoy_keys]
    assert [len(k) for k in probes] == [len(k) for k in decoy_probes]
    n_f = len(filter_first) - 1

    def build(ks):
        kb, ko = keys_buffer(ks)
        fs = []
        for f in range(n_f):
            a, b = int(filter_first[f]), int(filter_first[f + 1])
            fs.append(oracle.create_filter((kb[int(ko[a]):int(ko[b])] + b"\0", ko[a:b + 1] - ko[a]), bits_per_key))
        fblock = oracle.filter_block_build((kb, ko), [2048 * f for f in range(n_f)], filter_first, bits_per_key)
        return kb, ko, fs, fblock

    kb, ko, fs, fblock = build(keys)
    dkb, _, dfs, dfblock = build(decoy_keys)
    offs = np.cumsum([0] + [len(f) for f in fs])
    assert [len(f) for f in fs] == [len(f) for f in dfs] and len(fblock) == len(dfblock)
    pb, po = keys_buffer(probes)
    dpb, _ = keys_buffer(decoy_probes)
    # the filter each probe is put to: that of key q mod half, which holds the
    # payload's first half of the probes and the decoy's second half
    half = len(probes) // 2
    which = [int(np.searchsorted(np.asarray(filter_first), q % half, side="right")) - 1 for q in range(len(probes))]
    fh = [x for f in which for x in (int(offs[f]), len(fs[f]))]
    # FilterBlockReader picks filter block_offset >> 11; the last probe asks past the offset array
    data_offsets = [2048 * f + 100 * (q % 20) for q, f in enumerate(which)]
    data_offsets[-1] = 2048 * (n_f + 3)
    return Case({"keys": kb, "probes": pb, "filters": b"".join(fs) + b"\0", "fblock": fblock},
                {"keys": dkb, "probes": dpb, "filters": b"".join(dfs) + b"\1", "fblock": dfblock},
                {"key_offsets": ko, "probe_offsets": po, "filter_handles": fh,
                 "fblock_handles": [0, len(fblock)] * len(probes), "filter_first": filter_first,
                 "filter_out": offs[:-1], "data_offsets": data_offsets},
                {"key_offsets": ("keys", "all"), "probe_offsets": ("probes", "all"),
                 "filter_handles": ("filters", "pairs"), "fblock_handles": ("fblock", "pairs")},
                {"bits_per_key": bits_per_key, "filter_bytes": [len(f) for f in fs]})


def bloom_model(images, arrays, oracle, bits_per_key):
    keys = split_keys(images["keys"], arrays["key_offsets"])
    probes = split_keys(images["probes"], arrays["probe_offsets"])
    ff = arrays["filter_first"]
    built = [oracle.create_filter(keys_buffer(keys[int(ff[f]):int(ff[f + 1])]), bits_per_key)
             for f in range(len(ff) - 1)]
    fh, bh = arrays["filter_handles"], arrays["fblock_handles"]
    may, bmay = [], []
    for q, k in enumerate(probes):
        flt = images["filters"][int(fh[2 * q]):int(fh[2 * q]) + int(fh[2 * q + 1])]
        may.append(oracle.key_may_match(k, flt, bits_per_key))
        blk = images["fblock"][int(bh[2 * q]):int(bh[2 * q]) + int(bh[2 * q + 1])]
        bmay.append(oracle.filter_block_may_match(blk, int(arrays["data_offsets"][q]), k, bits_per_key))
    return {"built": built, "may": np.array(may, dtype=np.int64), "block_may": np.array(bmay, dtype=np.int64)}


BLOOM_SHIFTS = {"built": None, "may": None, "block_may": None}


# --------------------------------------------------------------------------- pack
def pack_plan_model(raw_len, comp_len, first_offset, gap):
    """lsbm_block_pack_plan_dev's rule (include/lsbm_table_pack.h), plain."""
    types, handles, off = [], [], int(first_offset)
    for r, c in zip(raw_len, comp_len):
        r, c = int(r), int(c)
        t = 1 if (c != -1 and c < r - r // 8) else 0
        size = c if t else r
        types.append(t)
        handles += [off, size]
        off += size + gap
    return {"types": np.array(types, dtype=np.int64), "handles": np.array(handles, dtype=np.int64),
            "end": np.array([off], dtype=np.int64)}


def _pairs_offset(name):
    def sel(o):
        m = np.zeros(np.asarray(o[name]).shape, dtype=bool)
        m.reshape(-1)[0::2] = True
        return m
    return sel


PACK_PLAN_SHIFTS = {"types": None, "handles": ("out", _pairs_offset("handles")),
                    "end": ("out", lambda o: np.ones(1, dtype=bool))}


def pack_mover_case():
    """Blocks of 4097, 15 and 1 bytes among others, alternately raw and
    compressed, 3 bytes apart in their source image; the decoy's blocks have
    other bytes in the same places.  Returns (sizes, types, blocks, decoy
    blocks, source offsets, {type: image}, {type: decoy image})."""
    sizes, types = [4097, 15, 1, 300, 64, 17], [0, 1, 0, 1, 0, 1]
    rng = np.random.default_rng(77)
    data = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in sizes]
    decoy = [bytes(255 - x for x in d) for d in data]
    src_off, pos = [], {0: 0, 1: 0}
    for n, t in zip(sizes, types):
        src_off.append(pos[t])
        pos[t] += n + 3
    img = {t: bytearray(pos[t]) for t in (0, 1)}
    dimg = {t: bytearray(pos[t]) for t in (0, 1)}
    for d, dd, o, t in zip(data, decoy, src_off, types):
        img[t][o:o + len(d)] = d
        dimg[t][o:o + len(d)] = dd
    return sizes, types, data, decoy, src_off, img, dimg


# --------------------------------------------------------------------------- merge
def merge_case(seed=5):
    """3 runs, 257 entries in all, user keys shared across the runs (equal user
    keys at different and at equal sequences), some deletions."""
    def build(salt):
        pick, rng = np.random.default_rng(seed), np.random.default_rng(seed + 1 + salt)
        runs, n_in = [], (100, 90, 67)
        for r, n in enumerate(n_in):
            users = sorted(pick.choice(120, n, replace=False).tolist())
            run = []
            for u in users:
                seq = int(rng.integers(1, 40)) if (u + salt) % 5 else 20  # equal internal keys across runs
                typ = 0 if int(rng.integers(0, 6)) == 0 else 1
                run.append(mm.internal_key((b"u%c%05d" % (65 + salt, u)) + b"x" * (u % 4), seq, typ))
            runs.append(run)  # (distinct users in ascending order: sorted)
        return runs
    runs, druns = build(0), build(1)
    keys = [k for run in runs for k in run]
    dkeys = [k for run in druns for k in run]
    assert len(keys) == 257 and [len(k) for k in keys] == [len(k) for k in dkeys]
    kb, ko = keys_buffer(keys)
    dkb, _ = keys_buffer(dkeys)
    run_first = np.cumsum([0] + [len(r) for r in runs])
    values = np.array([[1000 + 7 * i, i % 11] for i in range(len(keys))], dtype=np.int64).reshape(-1)
    vimage = bytes(range(256)) * 12
    return Case({"keys": kb, "vimage": vimage}, {"keys": dkb, "vimage": vimage[::-1]},
                {"key_offsets": ko, "run_first": run_first, "values": values},
                {"key_offsets": ("keys", "all"), "values": ("vimage", "pairs")})


def merge_model(images, arrays, drop, smallest_snapshot=15, bottom_level=True):
    keys = split_keys(images["keys"], arrays["key_offsets"])
    v = arrays["values"].reshape(-1, 2)
    rf = arrays["run_first"]
    runs = [[(keys[i], (int(v[i, 0]), int(v[i, 1]))) for i in range(int(rf[r]), int(rf[r + 1]))]
            for r in range(len(rf) - 1)]
    out, source = mm.merge_entries(runs, mm.INTERNAL_KEY, drop, smallest_snapshot, bottom_level)
    okeys = [k for k, _ in out]
    ooff = np.cumsum([0] + [len(k) for k in okeys])
    return {"source": np.array(source, dtype=np.int64), "out_key_offsets": ooff.astype(np.int64),
            "counts": np.array([len(out), int(ooff[-1])], dtype=np.int64),
            "run_status": np.array([mm.run_status([k for k, _ in run], mm.INTERNAL_KEY) for run in runs],
                                   dtype=np.int64),
            "out_keys": b"".join(okeys),
            "out_values": np.array([list(s) for _, s in out], dtype=np.int64).reshape(-1, 2),
            "gather_status": np.array([0], dtype=np.int64)}


MERGE_SHIFTS = {"source": None, "out_key_offsets": None, "counts": None, "run_status": None, "out_keys": None,
                "out_values": ("vimage", _offset_slot("out_values")), "gather_status": None}
# outputs that the offset arrays alone decide (a well-formed decoy of the same
# layout has the same ones): not part of the decoy-differs assertion
MERGE_LAYOUT_ONLY = ("run_status", "gather_status")
# without the drop rule every entry comes out, and payload and decoy hold keys
# of the same lengths under the same user-key order: the count and the running
# sum of the merged keys' lengths are the layout's too
MERGE_LAYOUT_ONLY_WITHOUT_DROP = MERGE_LAYOUT_ONLY + ("counts", "out_key_offsets")


# --------------------------------------------------------------------------- memtable
def memtable_case():
    """Four WriteBatch records: puts and deletions with keys of 8 bytes and
    more (copied by 8-byte words), one with a value that runs past the record
    (bad Put), one with a wrong count.  The decoy's records have the same
    lengths and other operations."""
    def put(k, v):
        return (1, k, v)

    def dele(k):
        return (0, k, b"")
    recs = [mc.batch(1000, [put(b"alpha-key-%04d" % i, b"value%d" % i * 3) for i in range(5)] + [dele(b"alpha-key-0002")]),
            mc.batch(2000, [put(b"bravo-key-000001", b"v" * 40), put(b"bravo-key-000002", b"w" * 9)])[:-4],
            mc.batch(3000, [put(b"charlie-key-%02d" % i, b"") for i in range(3)], count=7),
            mc.batch(4000, [dele(b"delta-key-0123456789"), put(b"delta-key-1", b"x" * 130)])]
    # the same lengths: a put of (k, v) takes 3 + k + v bytes, a deletion of k' 2 + k'
    def sized(seq, ops, n):
        """The batch with its last operation's last field grown to n bytes in all."""
        for fill in range(n):
            tag, k, v = ops[-1]
            last = (tag, k, v + b"z" * fill) if tag else (tag, k + b"z" * fill, v)
            r = mc.batch(seq, ops[:-1] + [last])
            if len(r) == n:
                return r
        raise AssertionError(n)
    drecs = [sized(77, [dele(b"A" * 9)], len(recs[0])),
             sized(88, [put(b"B" * 20, b"b")], len(recs[1])),
             sized(99, [dele(b"D" * 10), put(b"C" * 9, b"c")], len(recs[2])),
             sized(66, [put(b"E" * 12, b"e" * 30), put(b"F" * 8, b"f")], len(recs[3]))]
    assert [len(r) for r in recs] == [len(r) for r in drecs], ([len(r) for r in recs], [len(r) for r in drecs])
    buf, dbuf, pairs = bytearray(), bytearray(), []
    for r, d in zip(recs, drecs):
        buf += b"\xaa" * 3
        dbuf += b"\xaa" * 3
        pairs += [len(buf), len(r)]
        buf += r
        dbuf += d
    return Case({"image": bytes(buf)}, {"image": bytes(dbuf)}, {"records": pairs}, {"records": ("image", "pairs")})


def memtable_model(images, arrays):
    buf = images["image"]
    recs = [(int(a), int(b)) for a, b in arrays["records"].reshape(-1, 2)]
    want = [mt.insert_into(buf, off, ln) for off, ln in recs]
    flat = [e for _, es in want for e in es]
    return {"counts": np.array([[len(es), sum(len(k) - 8 for k, _, _ in es)] for _, es in want], dtype=np.int64),
            "status": np.array([st for st, _ in want], dtype=np.int64),
            "keys": b"".join(k for k, _, _ in flat),
            "key_offsets": np.cumsum([0] + [len(k) for k, _, _ in flat]).astype(np.int64),
            "values": np.array([[vo, len(v)] for _, v, vo in flat], dtype=np.int64).reshape(-1, 2),
            "max_sequence": np.array([mt.max_sequence(buf, recs)], dtype=np.int64)}


# lsbm_memtable.h: d_values = "{offset of the value bytes in the image,
# length}; for a deletion length 0 and the offset just past the key": every
# offset slot moves with the image.  d_key_offsets index d_keys, whose windows
# start at d_key_base[0]: they move with the key window ("kout"), not the image.
MEMTABLE_SHIFTS = {"counts": None, "status": None, "keys": None,
                   "key_offsets": ("kout", lambda o: np.ones(np.asarray(o["key_offsets"]).shape, dtype=bool)),
                   "values": ("image", _offset_slot("values")), "max_sequence": None}


def sort_case():
    """The merge case's 257 internal keys in arrival order (the three runs back
    to back): equal user keys and equal internal keys among them."""
    c = merge_case()
    return Case({"keys": c.bufs["keys"]}, {"keys": c.decoy["keys"]}, {"key_offsets": c.arrays["key_offsets"]},
                {"key_offsets": ("keys", "all")})


def sort_model(images, arrays):
    keys = split_keys(images["keys"], arrays["key_offsets"])
    order = mt.order(keys)
    return {"source": np.array(order, dtype=np.int64),
            "out_key_offsets": np.cumsum([0] + [len(keys[i]) for i in order]).astype(np.int64),
            "counts": np.array([len(keys), sum(len(k) for k in keys)], dtype=np.int64),
            "status": np.array([0], dtype=np.int64)}


SORT_SHIFTS = {"source": None, "out_key_offsets": None, "counts": None, "status": None}
SORT_LAYOUT_ONLY = ("counts", "status", "out_key_offsets")  # (the same user-key order: the same running sum)


# --------------------------------------------------------------------------- block and index builder
BUILD_BLOCK_SIZE, BUILD_RESTART = 600, 4


def build_case():
    """The merge case's 257 entries in merged order as two tables, with real
    value bytes: blocks of about 600 bytes, a restart every 4 entries."""
    def entries(keys, salt):
        keys = sorted(keys, key=lambda k: (k[:-8], -mm.tag_of(k)))
        rng = np.random.default_rng(900 + salt)
        vimage = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
        return keys, vimage
    c = merge_case()
    keys, vimage = entries(split_keys(c.bufs["keys"], c.arrays["key_offsets"]), 0)
    # the decoy: other keys of the same lengths in the same places, other value bytes
    dkeys = [bytes(b ^ 1 if i < len(k) - 8 else b for i, b in enumerate(k)) for k in keys]
    dvimage = bytes(255 - b for b in vimage)
    kb, ko = keys_buffer(keys)
    dkb, _ = keys_buffer(dkeys)
    values = np.array([[(37 * i) % 2800, (i * 5) % 23 if i % 9 else 150] for i in range(len(keys))],
                      dtype=np.int64).reshape(-1)
    return Case({"keys": kb, "vimage": vimage}, {"keys": dkb, "vimage": dvimage},
                {"key_offsets": ko, "values": values, "table_first": [0, 130, 257]},
                {"key_offsets": ("keys", "all"), "values": ("vimage", "pairs")})


def build_model(images, arrays, data_handles=None, cmp=bm.INTERNAL_KEY):
    """plan, build and index block of include/lsbm_block_build.h.  data_handles:
    the {offset, size} the index entries name (default: the blocks back to back
    from 0 with 5-byte trailers)."""
    keys = split_keys(images["keys"], arrays["key_offsets"])
    v = arrays["values"].reshape(-1, 2)
    vals = [images["vimage"][int(o):int(o) + int(n)] for o, n in v]
    tf = [int(x) for x in arrays["table_first"]]
    block_first, block_bytes, tbf, blocks = [], [], [0], []
    for t in range(len(tf) - 1):
        first, sizes = bd.plan([(keys[i], len(vals[i])) for i in range(tf[t], tf[t + 1])], BUILD_BLOCK_SIZE,
                               BUILD_RESTART)
        block_first += [tf[t] + f for f in first[:-1]]
        block_bytes += sizes
        tbf.append(len(block_first))
    block_first.append(tf[-1])
    for b in range(len(block_bytes)):
        blk = bm.build_block([(keys[i], vals[i]) for i in range(block_first[b], block_first[b + 1])], BUILD_RESTART)
        assert len(blk) == block_bytes[b]
        blocks.append(blk)
    if data_handles is None:
        data_handles, off = [], 0
        for n in block_bytes:
            data_handles += [off, n]
            off += n + 5
    dh = [(int(data_handles[2 * b]), int(data_handles[2 * b + 1])) for b in range(len(block_bytes))]
    index = [bd.index_block(keys, block_first[tbf[t]:tbf[t + 1] + 1], dh[tbf[t]:tbf[t + 1]], cmp)
             for t in range(len(tf) - 1)]
    return {"block_first": np.array(block_first, dtype=np.int64), "block_bytes": np.array(block_bytes, dtype=np.int64),
            "table_block_first": np.array(tbf, dtype=np.int64), "plan_status": np.zeros(len(tf) - 1, dtype=np.int64),
            "blocks": blocks, "built_bytes": np.array(block_bytes, dtype=np.int64),
            "build_status": np.zeros(len(block_bytes), dtype=np.int64), "index_blocks": index,
            "index_bytes": np.array([len(x) for x in index], dtype=np.int64),
            "index_status": np.zeros(len(index), dtype=np.int64)}


# lsbm_block_build.h: entry numbers, sizes, statuses and block bytes: nothing
# is an offset into an input buffer
BUILD_SHIFTS = {k: None for k in ("block_first", "block_bytes", "table_block_first", "plan_status", "blocks",
                                  "built_bytes", "build_status", "index_blocks", "index_bytes", "index_status")}
# what the key offsets and value lengths alone decide, or is OK for any
# well-formed input
BUILD_LAYOUT_ONLY = ("block_first", "block_bytes", "table_block_first", "plan_status", "built_bytes", "build_status",
                     "index_status")


# --------------------------------------------------------------------------- Get
GET_SNAPSHOT, GET_SOURCE = 50, 3
GET_RUN_FLAGS = [0, gm.RUN_LEVEL0, 0]
GET_RUN_FIRST = [0, 4, 5, 8]


def get_case(seed=21):
    """70 queries over a sorted memtable of 90 entries, 8 files in 3 runs (the
    middle one a Level-0 file), one round of table reads for SaveValue, and a
    value image.  The decoy holds other keys of the same lengths."""
    def build(prefix, salt):
        rng = np.random.default_rng(seed + salt)
        name = lambda u: prefix + b"%04d" % u + b"q" * (u % 3)  # noqa: E731
        users = [name(int(u)) for u in rng.integers(0, 120, 70)]
        ents = []
        for u in sorted(rng.choice(120, 60, replace=False).tolist()):
            for s in sorted(rng.choice(np.arange(1, 100), 1 + u % 2, replace=False).tolist(), reverse=True):
                ents.append(mm.internal_key(name(u), int(s), int(rng.integers(0, 4) != 0)))
        ents = ents[:90]
        cuts = sorted(rng.choice(np.arange(5, 115), 9, replace=False).tolist())
        bounds = []
        for f in range(8):  # (runs 0 and 2 ascend; the Level-0 file in between overlaps them)
            lo, hi = (cuts[f], cuts[f + 1] - 1) if f != 4 else (cuts[0] + 20, cuts[0] + 60)
            bounds += [mm.internal_key(name(lo), 90, 1), mm.internal_key(name(hi), 5, 1)]
        # one round of table reads: the state, the found key, its value slice
        state, found = [], []
        for q, u in enumerate(users):
            kind = int(rng.integers(0, 8))
            state.append({0: gm.NOT_VALID, 1: gm.FILTERED, 2: gm.BAD_CHECKSUM}.get(kind, gm.VALID))
            key = u if kind < 6 else name((q * 7) % 120)  # (kind 6, 7: another user's key is found)
            tag = int(rng.integers(1, 60)) << 8 | (int(rng.integers(0, 3) != 0) if kind != 5 else 2)
            found.append(key + tag.to_bytes(8, "little"))
        vimage = bytes(rng.integers(0, 256, 2500, dtype=np.uint8))
        return users, ents, bounds, state, found, vimage
    users, ents, bounds, state, found, vimage = build(b"user", 0)
    d_users, _, d_bounds, _, d_found, d_vimage = build(b"USER", 1)

    def fit(mine, theirs):
        """theirs, each cut or padded to the length of mine's: the layout is the payload's."""
        return [(t[:-8] + b"qqq")[:len(m) - 8] + t[-8:] for m, t in zip(mine, theirs)]
    d_users = [(t + b"qqq")[:len(m)] for m, t in zip(users, d_users)]
    d_ents = _sorted_with_lengths([len(k) for k in ents], seed)
    d_bounds, d_found = fit(bounds, d_bounds), fit(found, d_found)
    ub, uo = keys_buffer(users)
    mb, mo = keys_buffer(ents)
    bb, bo = keys_buffer(bounds)
    fb, fo = keys_buffer(found)
    n = len(users)
    mem_values = np.array([[(53 * i) % 2300, i % 40] for i in range(len(ents))], dtype=np.int64).reshape(-1)
    value_in = np.array([[(91 * q) % 2300 + 1, (q * 3) % 50] for q in range(n)], dtype=np.int64).reshape(-1)
    return Case({"users": ub, "mem": mb, "bounds": bb, "found": fb, "vimage": vimage},
                {"users": keys_buffer(d_users)[0], "mem": keys_buffer(d_ents)[0], "bounds": keys_buffer(d_bounds)[0],
                 "found": keys_buffer(d_found)[0], "vimage": d_vimage},
                {"user_offsets": uo, "mem_offsets": mo, "mem_values": mem_values, "bound_offsets": bo,
                 "found_offsets": fo, "value_in": value_in, "state": state,
                 "key_len": [len(k) for k in found]},
                {"user_offsets": ("users", "all"), "mem_offsets": ("mem", "all"), "mem_values": ("vimage", "pairs"),
                 "bound_offsets": ("bounds", "all"), "found_offsets": ("found", "all"),
                 "value_in": ("vimage", "pairs")})


def _sorted_with_lengths(lengths, seed):
    """Internal keys "USER....", sorted as a memtable is, whose i-th key has
    lengths[i] bytes: the decoy of a memtable of that layout."""
    rng = np.random.default_rng(seed + 1000)
    out, u = [], 0
    for i, n in enumerate(lengths):
        pad = n - 16
        assert 0 <= pad <= 2
        if not (i and int(rng.integers(0, 3)) == 0 and len(out[-1]) == n and mm.tag_of(out[-1]) >> 8 > 1):
            u += 1 + int(rng.integers(0, 2))
            seq = int(rng.integers(40, 99))
        else:
            seq = (mm.tag_of(out[-1]) >> 8) - 1
        out.append(mm.internal_key(b"USER%04d" % u + b"q" * pad, seq, int(rng.integers(0, 3) != 0)))
    assert out == sorted(out, key=lambda k: (k[:-8], -mm.tag_of(k)))
    return out


def get_model(images, arrays):
    """lookup keys, MemTable::Get, the file pick, SaveValue (from fresh
    verdicts) and the gathered values, from tests/golden/getmodel.py."""
    users = split_keys(images["users"], arrays["user_offsets"])
    n = len(users)
    lkeys = [gm.lookup_key(u, GET_SNAPSHOT) for u in users]
    mv = arrays["mem_values"].reshape(-1, 2)
    ents = [(k, (int(mv[i, 0]), int(mv[i, 1]))) for i, k in
            enumerate(split_keys(images["mem"], arrays["mem_offsets"]))]
    m_verdict, m_value, m_where = [], [], []
    for u in users:
        v, val = gm.memtable_get(ents, u, GET_SNAPSHOT)
        m_verdict.append(v)
        m_value.append(list(val) if v == gm.FOUND else [0, 0])
        m_where.append(GET_SOURCE if v != gm.UNDECIDED else -1)
    b = split_keys(images["bounds"], arrays["bound_offsets"])
    files = [(b[2 * f], b[2 * f + 1]) for f in range(len(b) // 2)]
    visible = [1, 1, 0, 1, 1, 1, 1, 0]
    pick = []
    for k in lkeys:
        row = []
        for r, flags in enumerate(GET_RUN_FLAGS):
            lo, hi = GET_RUN_FIRST[r], GET_RUN_FIRST[r + 1]
            i = gm.pick(files[lo:hi], flags, k, visible[lo:hi])
            row.append(lo + i if i >= 0 else -1)
        pick.append(row)
    found = split_keys(images["found"], arrays["found_offsets"])
    vin = arrays["value_in"].reshape(-1, 2)
    state = arrays["state"]
    s_verdict, s_value, s_where = [], [], []
    for q, u in enumerate(users):
        v, val = gm.save_value(int(state[q]), found[q], (int(vin[q, 0]), int(vin[q, 1])), u)
        s_verdict.append(v)
        s_value.append(list(val) if v == gm.FOUND else [0, 0])
        s_where.append(GET_SOURCE + 1 if v != gm.UNDECIDED else -1)
    vimage = images["vimage"]
    gathered = [vimage[o:o + ln] if w == GET_SOURCE + 1 else b"" for (o, ln), w in zip(s_value, s_where)]
    uo = arrays["user_offsets"]
    return {"lookup_keys": b"".join(lkeys), "lookup_offsets": (uo + 8 * np.arange(n + 1)).astype(np.int64),
            "lookup_status": np.array([0], dtype=np.int64),
            "mem_verdict": np.array(m_verdict, dtype=np.int64), "mem_value": np.array(m_value, dtype=np.int64),
            "mem_where": np.array(m_where, dtype=np.int64), "file": np.array(pick, dtype=np.int64),
            "save_verdict": np.array(s_verdict, dtype=np.int64), "save_value": np.array(s_value, dtype=np.int64),
            "save_where": np.array(s_where, dtype=np.int64), "gathered": gathered}


def _found_slot(value, verdict):
    def sel(o):
        m = np.zeros(np.asarray(o[value]).shape, dtype=bool)
        m[:, 0] = np.asarray(o[verdict]) == gm.FOUND
        return m
    return sel


# lsbm_get.h: "d_key_offsets[q] = d_user_offsets[q] + 8q" moves with the user
# keys' base; "d_value[2q], [2q+1] = the entry's slice" / "= the slice" pass a
# slice through, so a found query's offset moves with the value image and the
# {0, 0} of a deletion does not; verdicts, where words and file indices do not.
GET_SHIFTS = {"lookup_keys": None,
              "lookup_offsets": ("users", lambda o: np.ones(np.asarray(o["lookup_offsets"]).shape, dtype=bool)),
              "lookup_status": None, "mem_verdict": None, "mem_value": ("vimage", _found_slot("mem_value", "mem_verdict")),
              "mem_where": None, "file": None, "save_verdict": None,
              "save_value": ("vimage", _found_slot("save_value", "save_verdict")), "save_where": None,
              "gathered": None}
GET_LAYOUT_ONLY = ("lookup_status", "lookup_offsets")


# --------------------------------------------------------------------------- scans
SCAN_SNAPSHOTS = (3, 1995)


def scan_case(history):
    """history: the 769 sorted (internal key, value) entries of
    test_scan_gpu.tile_edge_history().  Queries: windows inside and across the
    tiles, absent bounds, limits.  The decoy: the same user keys with every
    entry's type flipped between value and deletion, other value bytes, and
    other bounds of the same lengths."""
    keys = [k for k, _ in history]
    vals = [v for _, v in history]
    dkeys = [k[:-8] + bytes([k[-8] ^ 1 if k[-8] < 2 else k[-8]]) + k[-7:] for k in keys]
    assert dkeys == sorted(dkeys, key=lambda k: (k[:-8], -sm.tag_of(k)))
    dvals = [bytes(255 - b for b in v) for v in vals]
    queries = [(b"a000", b"a050", 1 << 40), (b"a090", b"n", 1 << 40), (None, b"p", 7), (b"m", None, 1 << 40),
               (b"a04", b"q", 300), (None, None, 1 << 40), (b"n000", b"n001", 1), (b"p", b"r", 1 << 40),
               (b"a099", b"m", 0), (b"zz", None, 5), (b"a010", b"a011", 1 << 40), (b"n", b"pz", 2)]
    dqueries = [(b"a030", b"a070", 0), (b"a001", b"q", 0), (None, b"b", 0), (b"a", None, 0), (b"a99", b"m", 0),
                (None, None, 0), (b"a000", b"a001", 0), (b"q", b"z", 0), (b"a000", b"n", 0), (b"aa", None, 0),
                (b"a050", b"a090", 0), (b"a", b"a9", 0)]
    kb, ko = keys_buffer(keys)
    vb, vo = keys_buffer(vals)
    lo, lo_off = keys_buffer([q[0] or b"" for q in queries])
    hi, hi_off = keys_buffer([q[1] or b"" for q in queries])
    dlo, dlo_off = keys_buffer([q[0] or b"" for q in dqueries])
    dhi, dhi_off = keys_buffer([q[1] or b"" for q in dqueries])
    assert (lo_off == dlo_off).all() and (hi_off == dhi_off).all()
    values = np.stack([vo[:-1], np.diff(vo)], 1).reshape(-1)
    return Case({"keys": kb, "vimage": vb, "lo": lo, "hi": hi},
                {"keys": keys_buffer(dkeys)[0], "vimage": keys_buffer(dvals)[0], "lo": dlo, "hi": dhi},
                {"key_offsets": ko, "values": values, "lo_offsets": lo_off, "hi_offsets": hi_off,
                 "lo_present": [q[0] is not None for q in queries], "hi_present": [q[1] is not None for q in queries],
                 "limits": [q[2] for q in queries]},
                {"key_offsets": ("keys", "all"), "values": ("vimage", "pairs"), "lo_offsets": ("lo", "all"),
                 "hi_offsets": ("hi", "all")})


def scan_model(images, arrays, snapshot):
    """The snapshot view (lsbm_dbiter_plan_dev's arrays, the gathered live
    slices) and every query forward and reverse, from tests/golden/scanmodel.py."""
    keys = split_keys(images["keys"], arrays["key_offsets"])
    v = arrays["values"].reshape(-1, 2)
    entries = [(k, images["vimage"][int(o):int(o) + int(n)]) for k, (o, n) in zip(keys, v)]
    view = sm.View(entries, snapshot)
    los = split_keys(images["lo"], arrays["lo_offsets"])
    his = split_keys(images["hi"], arrays["hi_offsets"])
    out = {"live": np.array(view.live, dtype=np.int64), "yield_rank": np.array(view.yield_rank, dtype=np.int64),
           "corrupt_rank": np.array(view.corrupt_rank, dtype=np.int64), "first": np.array(view.first, dtype=np.int64),
           "back": np.array(view.back, dtype=np.int64),
           "counts": np.array([view.n_yield, sum(len(keys[j]) for j in view.live), view.corrupt_rank[-1]],
                              dtype=np.int64),
           "live_values": v[view.live].astype(np.int64).reshape(-1, 2)}
    for reverse in (False, True):
        got = [sm.scan_port(entries, snapshot, lo if p else None, hi if h else None, int(lim), reverse)[:2]
               for lo, hi, p, h, lim in zip(los, his, arrays["lo_present"], arrays["hi_present"], arrays["limits"])]
        flat = [e for es, _ in got for e in es]
        tag = "reverse" if reverse else "forward"
        out[tag + "_status"] = np.array([st for _, st in got], dtype=np.int64)
        out[tag + "_entry_first"] = np.cumsum([0] + [len(es) for es, _ in got]).astype(np.int64)
        out[tag + "_keys"] = b"".join(k for k, _ in flat)
        out[tag + "_key_offsets"] = np.cumsum([0] + [len(k) for k, _ in flat]).astype(np.int64)
        out[tag + "_values"] = b"".join(x for _, x in flat)
        out[tag + "_value_offsets"] = np.cumsum([0] + [len(x) for _, x in flat]).astype(np.int64)
    return out


# lsbm_iter.h: positions, ranks, counts, statuses and the emitted bytes with
# their own running offsets; the live entries' value slices are
# lsbm_merge_gather_dev's, "copied from the source entry": they move with the
# value image
SCAN_SHIFTS = {k: None for k in ("live", "yield_rank", "corrupt_rank", "first", "back", "counts")}
SCAN_SHIFTS["live_values"] = ("vimage", _offset_slot("live_values"))
for _tag in ("forward", "reverse"):
    for _name in ("status", "entry_first", "keys", "key_offsets", "values", "value_offsets"):
        SCAN_SHIFTS["%s_%s" % (_tag, _name)] = None
# the same for any entries with these user keys and corrupt positions
SCAN_LAYOUT_ONLY = ("corrupt_rank",)
