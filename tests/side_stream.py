"""Every callable of lsbm_amd that takes `stream`, with the smallest input the
suite has for it and the answer of the plain models.

REGISTRY maps "module.function" or "module.Class.method" to an Entry:

    make(torch)          the device inputs (for a method, the object too), all
                         built on the default stream; output windows that the
                         caller passes are part of the inputs, filled with 0xEE
    call(inputs, stream) the wrapper with that `stream`; returns read(), which
                         copies the results to the host (after the caller has
                         synchronised: call itself reads nothing back that the
                         wrapper does not) as a dict of output name to numpy
                         array, bytes, list or number
    want()               the same dict from the models under tests/golden and
                         the CRC, bloom and snappy oracles: no GPU
    own                  the outputs the wrapper creates (and fills) itself; an
                         entry's want() has at least one of them not all zeros,
                         so that a zero-fill ordered after the kernel shows.
                         Empty only with `creates_nothing`, the reason.

A wrapper whose only own output is a status word that is 0 on good input makes
a second call in `call` with the smallest input its header refuses (a window one
byte short, a key under 8 bytes, ...): that status is not 0, and the outputs the
refused call must leave alone are compared too.

tests/test_stream_wrappers.py holds the registry against the package;
tests/test_side_stream_gpu.py runs every entry on a side stream.
"""
import functools
import json
import os
import random
import struct
from collections import namedtuple

import numpy as np

import high_offsets as ho
from golden import blockmodel as bm
from golden import buffered_cases as bc
from golden import buffermodel as bfm
from golden import buildmodel as bd
from golden import getmodel as gm
from golden import logreadmodel as lrm
from golden import manifest_cases as mfc
from golden import manifestmodel as mfm
from golden import memcutmodel as mcm
from golden import memtable_cases as mtc
from golden import memtablemodel as mt
from golden import mergemodel as mm
from golden import scanmodel as sm
from golden import snappy_table_cases as tc
from golden import snappytablemodel as stm
from golden import tablewritemodel as tw
from golden import write_cases as wc
from golden import writemodel as wm

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
FILL = 0xEE
LINE = ho.LINE

Entry = namedtuple("Entry", "name make call want own creates_nothing")
REGISTRY = {}


def reg(name, own, make, call, want, creates_nothing=None):
    assert name not in REGISTRY, name
    REGISTRY[name] = Entry(name, make, call, want, tuple(own), creates_nothing)


cached = functools.lru_cache(maxsize=None)


# ---------------------------------------------------------------- oracles and helpers
@cached
def oracles():
    """(crc, bloom, snappy): tests/conftest.py's views of the oracle libraries."""
    import conftest
    return (conftest.Oracle(conftest._build("oracle", "liboracle_crc32c.so")),
            conftest.BloomOracle(conftest._build("oracle", "liboracle_bloom.so")),
            conftest.SnappyOracle(conftest._build("oracle", "liboracle_snappy.so")))


def crc():
    return oracles()[0]


def masked_crc(data):
    """The masked CRC a log header or a block trailer holds."""
    return crc().mask(crc().value(data))


def compress(data):
    return oracles()[2].compress(data)


def uncompress(data):
    ok, out = oracles()[2].uncompress(data)
    return out if ok else None


def stream_positions():
    """{name: index of its stream argument} of every *_dev function of the C
    ABI, from lsbm_amd/_lib.py's signature tables: by the headers' convention
    the trailing void* (tests/test_stream_wrappers.py holds the tables against
    the headers' parameter lists)."""
    import ctypes
    from lsbm_amd import _lib
    out = {}
    for table in (getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES")):
        for name, (_, args) in table.items():
            if name.endswith("_dev"):
                assert args and args[-1] is ctypes.c_void_p, name
                out[name] = len(args) - 1
    return out


def u8(torch, data):
    """bytes -> a uint8 device tensor with an address even when empty."""
    a = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    return torch.from_numpy(a.copy()).cuda()[:a.size - 1]


def dev(torch, a, dtype=np.int64):
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    if a.size == 0:
        return torch.zeros(1, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")[:0].reshape(a.shape)
    return torch.from_numpy(a.copy()).cuda()


def filled(torch, n, dtype=None, fill=FILL):
    return torch.full((max(n, 1),), fill, dtype=dtype or torch.uint8, device="cuda")[:n]


def ints(t):
    return t.cpu().numpy().astype(np.int64)


def byts(t):
    return t.cpu().numpy().tobytes()


def arr(a):
    return np.asarray(a, dtype=np.int64)


def pick(d, *names, **renamed):
    out = {n: d[n] for n in names}
    out.update({new: d[old] for new, old in renamed.items()})
    return out


def cut(buf, pairs):
    """[bytes] of {offset, length} pairs of a buffer."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return [bytes(buf[int(o):int(o) + int(n)]) for o, n in pairs]


def split(buf, offsets):
    return ho.split_keys(buf, np.asarray(offsets, dtype=np.int64))


def packed(items):
    """(bytes back to back, int64 offsets)."""
    off = np.zeros(len(items) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(k) for k in items])
    return b"".join(items), off


def nonzero(v):
    """Whether an output holds anything but zeros."""
    if v is None:
        return False
    if isinstance(v, (bytes, bytearray)):
        return any(v)
    if isinstance(v, str):
        return bool(v)
    if isinstance(v, dict):
        return any(nonzero(x) for x in v.values()) or any(nonzero(k) for k in v)
    if isinstance(v, (list, tuple)):
        return any(nonzero(x) for x in v)
    return bool(np.asarray(v).any())


def same(a, b):
    """Equality of two outputs, to the byte: arrays by shape and value, lists
    item by item."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and bool((a == b).all())
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (bytes, bytearray)) and isinstance(b, (bytes, bytearray)):
        return bytes(a) == bytes(b)
    return type(a) is type(b) and a == b or (isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer))
                                              and int(a) == int(b))


def assert_same(got, want, note=""):
    assert sorted(got) == sorted(want), (note, sorted(got), sorted(want))
    for name in want:
        assert same(got[name], want[name]), (note, name)


# ---------------------------------------------------------------- engine: CRC-32C
CRC_BLOCKS, CRC_BLOCK = 64, 4096  # far below kTailMinRows x waves: the cross-XCC queue is never entered
CRC_OFFSETS = [0, 1, 16, 4097, 5000, 70000, 70000, CRC_BLOCKS * CRC_BLOCK]
CRC_EXTENTS = [3, 100, 4096, 4096, 100000, 0, 200001, 62143]


@cached
def crc_data():
    return crc().fill_splitmix64(0, CRC_BLOCKS * CRC_BLOCK, 0x51DE57)


def _crc_make(torch):
    return {"data": u8(torch, crc_data().tobytes()), "offsets": dev(torch, CRC_OFFSETS),
            "extents": dev(torch, CRC_EXTENTS),
            "expect": dev(torch, _crc_expect().view(np.int32), np.int32)}


@cached
def _crc_expect():
    e = crc().batch_offsets(crc_data(), CRC_OFFSETS, masked=True).copy()
    e[2] ^= 1
    return e


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _crc_fixed(x, s):
    from lsbm_amd import engine
    out = engine.crc32c_fixed(x["data"], CRC_BLOCK, CRC_BLOCK, CRC_BLOCKS, stream=s)

    def read():
        return {"crc": _u32(out)}
    return read


def _crc_batch(x, s):
    from lsbm_amd import engine
    out = engine.crc32c_batch(x["data"], x["offsets"], masked=True, stream=s)

    def read():
        return {"crc": _u32(out)}
    return read


def _crc_extents(x, s):
    from lsbm_amd import engine
    out = engine.crc32c_extents(x["data"], x["extents"], stream=s)

    def read():
        return {"crc": _u32(out)}
    return read


def _crc_verify(x, s):
    from lsbm_amd import engine
    ok, nbad = engine.crc32c_verify(x["data"], x["offsets"], x["expect"], masked=True, stream=s)

    def read():
        return {"ok": ints(ok), "nbad": ints(nbad)}
    return read


def _crc_verify_want():
    ok = np.ones(len(CRC_OFFSETS) - 1, dtype=np.int64)
    ok[2] = 0
    return {"ok": ok, "nbad": arr([1])}


reg("engine.crc32c_fixed", ["crc"], _crc_make, _crc_fixed,
    lambda: {"crc": crc().batch_fixed(crc_data(), CRC_BLOCK, CRC_BLOCK, CRC_BLOCKS).astype(np.int64)})
reg("engine.crc32c_batch", ["crc"], _crc_make, _crc_batch,
    lambda: {"crc": crc().batch_offsets(crc_data(), CRC_OFFSETS, masked=True).astype(np.int64)})
reg("engine.crc32c_extents", ["crc"], _crc_make, _crc_extents,
    lambda: {"crc": arr([crc().value(crc_data()[o:o + n].tobytes())
                         for o, n in np.array(CRC_EXTENTS).reshape(-1, 2).tolist()])})
reg("engine.crc32c_verify", ["ok", "nbad"], _crc_make, _crc_verify, _crc_verify_want)

FILL_BYTES, FILL_SEED = 5003, 0xABCDEF0123


def _fill_call(x, s):
    from lsbm_amd import engine
    buf = engine.fill_splitmix64(x["buf"], FILL_SEED, stream=s)

    def read():
        return {"buf": byts(buf)}
    return read


reg("engine.fill_splitmix64", [], lambda torch: {"buf": filled(torch, FILL_BYTES)}, _fill_call,
    lambda: {"buf": crc().fill_splitmix64(0, FILL_BYTES, FILL_SEED).tobytes()},
    creates_nothing="fills the caller's buffer in place and returns it")

# stream_read folds every 16 bytes to x ^ y ^ z ^ w and stores a word of the
# sink only where a thread's fold equals a magic number: over words {x, x, 0, 0}
# every fold is 0, so the sink must stay exactly as it was
SINK_FILL = 0x5A5A5A5A


@cached
def _read_data():
    rng = np.random.default_rng(0x5EAD)
    w = np.zeros((2 * 32768 + 160) // 16 * 4, dtype=np.uint32).reshape(-1, 4)
    w[:, 0] = w[:, 1] = rng.integers(1, 1 << 32, w.shape[0], dtype=np.uint32)
    return w.reshape(-1).view(np.uint8)


def _read_call(x, s):
    from lsbm_amd import engine
    assert engine.stream_read(x["buf"], x["sink"], stream=s) is None

    def read():
        return {"sink": ints(x["sink"])}
    return read


reg("engine.stream_read", [],
    lambda torch: {"buf": u8(torch, _read_data().tobytes()), "sink": filled(torch, 1024, torch.int32, SINK_FILL)},
    _read_call, lambda: {"sink": np.full(1024, SINK_FILL, dtype=np.int64)},
    creates_nothing="reads only: its sink is the caller's and stays as it was for this input")


# ---------------------------------------------------------------- table: trailers
@cached
def table_case():
    """Three blocks laid out as TableBuilder lays them, a fourth handle whose
    trailer would pass the image, the sealed image, and one with block 2 damaged."""
    from lsbm_amd import table
    rng = np.random.default_rng(0x7AB1E)
    sizes, types = [300, 1, 4097], [0, 1, 0]
    blocks = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in sizes]
    handles, total = table.layout_blocks(sizes)
    raw, sealed = bytearray([FILL]) * total, bytearray([FILL]) * total
    for b, t, (o, n) in zip(blocks, types, handles.reshape(-1, 2).tolist()):
        raw[o:o + n] = b
        sealed[o:o + n + 5] = b + bd.trailer(b, t)
    handles = np.concatenate([handles, [total - 12, 10]])  # (10 + 5 bytes from total - 12: three past the image)
    damaged = bytearray(sealed)
    damaged[int(handles[4]) + 2000] ^= 0x40
    crcs = [struct.unpack("<I", bd.trailer(b, t)[1:])[0] for b, t in zip(blocks, types)] + [0]
    return {"raw": bytes(raw), "sealed": bytes(sealed), "damaged": bytes(damaged), "handles": handles,
            "types": types + [0], "crcs": crcs}


def _table_make(torch):
    c = table_case()
    return {"raw": u8(torch, c["raw"]), "damaged": u8(torch, c["damaged"]), "handles": dev(torch, c["handles"]),
            "types": dev(torch, c["types"], np.uint8)}


def _seal(x, s):
    from lsbm_amd import table
    nbad = table.seal_blocks(x["raw"], x["handles"], x["types"], stream=s)

    def read():
        return {"image": byts(x["raw"]), "nbad": ints(nbad)}
    return read


def _trailer_crcs(x, s):
    from lsbm_amd import table
    out, nbad = table.trailer_crcs(x["raw"], x["handles"], x["types"], stream=s)

    def read():
        return {"crc": _u32(out), "nbad": ints(nbad)}
    return read


def _verify_blocks(x, s):
    from lsbm_amd import table
    ok, nbad = table.verify_blocks(x["damaged"], x["handles"], stream=s)

    def read():
        return {"ok": ints(ok), "nbad": ints(nbad)}
    return read


def _verify_status(x, s):
    from lsbm_amd import table
    status, ok = table.verify_status(x["damaged"], x["handles"], stream=s)

    def read():
        return {"status": str(status), "ok": ints(ok)}
    return read


reg("table.seal_blocks", ["nbad"], _table_make, _seal, lambda: {"image": table_case()["sealed"], "nbad": arr([1])})
reg("table.trailer_crcs", ["crc", "nbad"], _table_make, _trailer_crcs,
    lambda: {"crc": arr(table_case()["crcs"]), "nbad": arr([1])})
reg("table.verify_blocks", ["ok", "nbad"], _table_make, _verify_blocks,
    lambda: {"ok": arr([1, 1, 0, 0]), "nbad": arr([2])})
reg("table.verify_status", ["ok"], _table_make, _verify_status,
    lambda: {"status": "Corruption: block checksum mismatch", "ok": arr([1, 1, 0, 0])})


# ---------------------------------------------------------------- log: seal, verify, log::Reader
@cached
def log_case():
    """Four records, the second of two fragments, as log::Writer frames them;
    `damaged` has a byte of the last payload flipped: one checksum report."""
    payloads = [b"first record", wc.pattern(5, 40000), b"", b"x" * 100]
    sealed, heads, _, _ = wm.add_records(payloads, 0, masked_crc)
    raw = wm.add_records(payloads, 0, None)[0]
    damaged = bytearray(sealed)
    damaged[-3] ^= 1
    img = np.frombuffer(bytes(damaged), dtype=np.uint8)
    ok_of = _ok_of()
    w, p, e = lrm.read(img, ok_of, 0)
    assert len(p.records) == 3 and len(p.events) == 1 and p.side_bytes == 40000
    return {"raw": raw, "sealed": sealed, "damaged": bytes(damaged), "heads": heads, "img": img,
            "ok": np.asarray(ok_of(img, w.headers), dtype=np.uint8), "w": w, "p": p, "e": e}


def _ok_of():
    def ok_of(buf, headers):
        stored, offs, data = lrm.header_fields(buf, headers)
        return crc().batch_offsets(data, offs, masked=True) == stored
    return ok_of


def _log_make(torch):
    c = log_case()
    n, side = len(c["damaged"]), c["p"].side_bytes
    w = c["w"]
    return {"raw": u8(torch, c["raw"]), "damaged": u8(torch, c["damaged"]), "heads": dev(torch, c["heads"]),
            "with_side": u8(torch, c["damaged"] + bytes([FILL]) * side), "n": n, "side": side,
            "block_first": dev(torch, w.block_first), "block_end": dev(torch, w.block_end),
            "headers": dev(torch, w.headers), "ok": dev(torch, c["ok"], np.uint8)}


def _log_seal(x, s):
    from lsbm_amd import log
    masked, nbad = log.seal_records(x["raw"], x["heads"], stream=s)

    def read():
        return {"image": byts(x["raw"]), "masked": _u32(masked), "nbad": ints(nbad)}
    return read


def _log_seal_want():
    c = log_case()
    return {"image": c["sealed"], "nbad": arr([0]),
            "masked": arr([struct.unpack_from("<I", c["sealed"], h)[0] for h in c["heads"]])}


def _log_verify(x, s):
    from lsbm_amd import log
    ok, nbad = log.verify_records(x["damaged"], x["heads"], stream=s)

    def read():
        return {"ok": ints(ok), "nbad": ints(nbad)}
    return read


def _log_walk(x, s):
    from lsbm_amd import log
    w = log.walk(x["damaged"], 0, x["n"], 0, headers_cap=x["headers"].numel(), stream=s)

    def read():
        return {"block_first": ints(w.block_first), "block_end": ints(w.block_end), "headers": ints(w.headers),
                "n_headers": ints(w.n_headers), "status": ints(w.status)}
    return read


def _log_walk_want():
    w = log_case()["w"]
    return {"block_first": w.block_first, "block_end": w.block_end, "headers": w.headers,
            "n_headers": arr([w.headers.size]), "status": arr([0])}


def _log_plan(x, s):
    from lsbm_amd import log
    p = log.plan(x["damaged"], 0, x["n"], 0, x["block_first"], x["block_end"], x["headers"], x["ok"], stream=s)

    def read():
        return {"totals": ints(p.totals), "status": ints(p.status)}
    return read


def _log_plan_want():
    p = log_case()["p"]
    return {"totals": arr([len(p.records), len(p.events), p.side_bytes, p.stop]), "status": arr([0])}


def _log_emit_make(torch):
    from lsbm_amd import log
    x = _log_make(torch)
    x["plan"] = log.plan(x["with_side"], 0, x["n"], 0, x["block_first"], x["block_end"], x["headers"], x["ok"])
    return x


def _log_emit(x, s):
    from lsbm_amd import log
    p = log_case()["p"]
    e = log.emit(x["with_side"], 0, x["n"], 0, x["plan"], x["n"], x["side"], len(p.records), len(p.events), stream=s)

    def read():
        return {"records": ints(e.records), "last_record_offset": ints(e.last_record_offset), "events": ints(e.events),
                "status": ints(e.status), "side": byts(x["with_side"][x["n"]:])}
    return read


def _log_read_want(status=True):
    e = log_case()["e"]
    out = {"records": arr(e.records).reshape(-1, 2), "last_record_offset": arr(e.last_record_offset),
           "events": arr(e.events).reshape(-1, 4), "side": e.side.tobytes()}
    if status:
        out["status"] = arr([0])
    return out


def _log_read(x, s):
    from lsbm_amd import log
    r = log.read_records(x["damaged"], stream=s)

    def read():
        image = byts(r.image)
        assert image[:x["n"]] == log_case()["damaged"]
        return {"records": ints(r.records), "last_record_offset": ints(r.last_record_offset), "events": ints(r.events),
                "side": image[x["n"]:]}
    return read


reg("log.seal_records", ["masked", "nbad"], _log_make, _log_seal, _log_seal_want)
reg("log.verify_records", ["ok", "nbad"], _log_make, _log_verify,
    lambda: {"ok": log_case()["ok"].astype(np.int64), "nbad": arr([1])})
reg("log.walk", ["block_first", "block_end", "headers", "n_headers", "status"], _log_make, _log_walk, _log_walk_want)
reg("log.plan", ["totals", "status"], _log_make, _log_plan, _log_plan_want)
reg("log.emit", ["records", "last_record_offset", "events", "status"], _log_emit_make, _log_emit, _log_read_want)
reg("log.read_records", ["records", "last_record_offset", "events", "side"], _log_make, _log_read,
    lambda: _log_read_want(status=False))

# ---------------------------------------------------------------- snappy
@cached
def snappy_case():
    with open(os.path.join(G, "snappy_fixture.json")) as f:
        golden = json.load(f)
    return ho.fixture_snappy_case(oracles()[2], golden)


@cached
def snappy_want():
    c = snappy_case()
    return ho.snappy_model(c.bufs, c.arrays, oracles()[2])


def _snappy_make(torch):
    c = snappy_case()
    return {"raw": u8(torch, c.bufs["raw"]), "comp": u8(torch, c.bufs["comp"]),
            "raw_offsets": dev(torch, c.arrays["raw_offsets"]), "comp_offsets": dev(torch, c.arrays["comp_offsets"])}


def _snappy_compress(x, s):
    from lsbm_amd import snappy
    out, off, n = snappy.compress(x["raw"], x["raw_offsets"], stream=s)

    def read():
        return {"compressed": cut(byts(out), np.stack([ints(off)[:-1], ints(n)], 1)), "compressed_len": ints(n)}
    return read


def _snappy_length(x, s):
    from lsbm_amd import snappy
    ulen, ok = snappy.uncompressed_length(x["comp"], x["comp_offsets"], stream=s)

    def read():
        return {"ulen": ints(ulen), "len_ok": ints(ok)}
    return read


def _snappy_uncompress(x, s):
    from lsbm_amd import snappy
    out, off, ok, n_bad = snappy.uncompress(x["comp"], x["comp_offsets"], stream=s)

    def read():
        return {"plain": split(byts(out), ints(off)), "ok": ints(ok), "n_bad": ints(n_bad)}
    return read


reg("snappy.compress", ["compressed", "compressed_len"], _snappy_make, _snappy_compress,
    lambda: pick(snappy_want(), "compressed", "compressed_len"))
reg("snappy.uncompressed_length", ["ulen", "len_ok"], _snappy_make, _snappy_length,
    lambda: pick(snappy_want(), "ulen", "len_ok"))
reg("snappy.uncompress", ["plain", "ok", "n_bad"], _snappy_make, _snappy_uncompress,
    lambda: dict(pick(snappy_want(), "plain", "ok"), n_bad=arr([0])))


# ---------------------------------------------------------------- bloom
BITS = 10


@cached
def bloom_case():
    return ho.fixture_bloom_case(oracles()[1])


@cached
def bloom_want():
    c = bloom_case()
    return ho.bloom_model(c.bufs, c.arrays, oracles()[1], BITS)


def _bloom_make(torch):
    c = bloom_case()
    x = {k: u8(torch, v) for k, v in c.bufs.items()}
    x.update({k: dev(torch, v) for k, v in c.arrays.items()})
    x["out"] = filled(torch, int(c.arrays["filter_out"][-1]) + c.extra["filter_bytes"][-1] + 16)
    return x


def _bloom_build(x, s):
    from lsbm_amd import bloom
    c = bloom_case()
    out = bloom.build_filters(x["keys"], x["key_offsets"], x["filter_first"], x["filter_out"], x["out"], BITS, stream=s)

    def read():
        host = byts(out)
        end = int(c.arrays["filter_out"][-1]) + c.extra["filter_bytes"][-1]
        return {"built": cut(host, np.stack([c.arrays["filter_out"], c.extra["filter_bytes"]], 1)), "after": host[end:]}
    return read


def _bloom_may(x, s):
    from lsbm_amd import bloom
    may, n_may = bloom.may_match(x["filters"], x["filter_handles"], x["probes"], x["probe_offsets"], BITS, stream=s)

    def read():
        return {"may": ints(may), "n_may": ints(n_may)}
    return read


def _bloom_block_may(x, s):
    from lsbm_amd import bloom
    may, n_may = bloom.filter_block_may_match(x["fblock"], x["fblock_handles"], x["data_offsets"], x["probes"],
                                              x["probe_offsets"], BITS, stream=s)

    def read():
        return {"block_may": ints(may), "n_may": ints(n_may)}
    return read


def _bloom_filter_block(x, s):
    from lsbm_amd import bloom
    c = bloom_case()
    n_f = len(c.arrays["filter_first"]) - 1
    block = bloom.build_filter_block(x["keys"], x["key_offsets"], [2048 * f for f in range(n_f)],
                                     c.arrays["filter_first"].tolist(), BITS, stream=s)

    def read():
        return {"block": block}
    return read


reg("bloom.build_filters", [], _bloom_make, _bloom_build,
    lambda: {"built": bloom_want()["built"], "after": bytes([FILL]) * 16},
    creates_nothing="writes into the caller's filter windows and returns them")
reg("bloom.may_match", ["may", "n_may"], _bloom_make, _bloom_may,
    lambda: {"may": bloom_want()["may"], "n_may": arr([bloom_want()["may"].sum()])})
reg("bloom.filter_block_may_match", ["block_may", "n_may"], _bloom_make, _bloom_block_may,
    lambda: {"block_may": bloom_want()["block_may"], "n_may": arr([bloom_want()["block_may"].sum()])})
reg("bloom.build_filter_block", ["block"], _bloom_make, _bloom_filter_block,
    lambda: {"block": bloom_case().bufs["fblock"]})


# ---------------------------------------------------------------- block reader
BLOCK_MODE = (bm.INTERNAL_KEY, False)


@cached
def block_case():
    return ho.fixture_block_case()


@cached
def block_want():
    c = block_case()
    return ho.block_model(c.bufs, c.arrays, *BLOCK_MODE)


def _block_make(torch):
    c = block_case()
    w = block_want()
    x = {k: u8(torch, v) for k, v in c.bufs.items()}
    x.update({k: dev(torch, v) for k, v in c.arrays.items()})
    x["found"] = filled(torch, len(w["found"]) + 16)
    x["found_offsets"] = dev(torch, np.concatenate([[0], np.cumsum(w["key_len"])]))
    return x


def _block_scan(x, s):
    from lsbm_amd import block
    counts, status = block.scan(x["image"], x["handles"], stream=s)

    def read():
        return {"counts": ints(counts), "status": ints(status)}
    return read


def _block_decode(x, s):
    """Without entry_base / key_base: the path with the cumsums and the host read."""
    from lsbm_amd import block
    keys, koff, values, entry_base, status = block.decode(x["image"], x["handles"], stream=s)

    def read():
        return {"keys": byts(keys), "key_offsets": ints(koff), "values": ints(values), "status": ints(status),
                "entry_base": ints(entry_base)}
    return read


def _block_seek(x, s):
    from lsbm_amd import block
    w = block_want()
    r = block.seek(x["image"], x["seek_handles"], x["targets"], x["target_offsets"], cmp=BLOCK_MODE[0],
                   value_is_handle=BLOCK_MODE[1], found=x["found"], found_offsets=x["found_offsets"], stream=s)

    def read():
        host = byts(x["found"])
        return {"state": ints(r.state), "pos": ints(r.pos), "key_len": ints(r.key_len), "value": ints(r.value),
                "found": host[:len(w["found"])], "after": host[len(w["found"]):]}
    return read


reg("block.scan", ["counts", "status"], _block_make, _block_scan, lambda: pick(block_want(), "counts", "status"))
reg("block.decode", ["keys", "key_offsets", "values", "status", "entry_base"], _block_make, _block_decode,
    lambda: dict(pick(block_want(), "keys", "key_offsets", "values", "status"),
                 entry_base=np.concatenate([[0], np.cumsum(block_want()["counts"][:, 0])])))
reg("block.seek", ["state", "pos", "key_len", "value"], _block_make, _block_seek,
    lambda: dict(pick(block_want(), "state", "pos", "key_len", "value", "found"), after=bytes([FILL]) * 16))


# ---------------------------------------------------------------- Table::InternalGet over one table
@cached
def get_table_case():
    """The snappy fixture's bloom_internal entries as one table file with a
    filter block, raw and snappy-compressed, and lookups of present keys, keys
    between them, keys past both ends; one data block of each file is damaged."""
    cmp, block_size, restart_interval, bits = tc.CASES["bloom_internal"]
    entries = tc.entries("bloom_internal")
    out = {"params": (cmp, block_size, restart_interval, bits)}
    users = [k[:-8] for k, _ in entries]
    probes = [gm.lookup_key(u, 2000) for u in users[::9]] + [gm.lookup_key(u + b"+", 2000) for u in users[3::17]] + \
        [gm.lookup_key(b"a", 5), gm.lookup_key(b"zz", 5), gm.lookup_key(users[40], 1)]
    out["keys"], out["key_offsets"] = packed(probes)
    out["probes"] = probes
    for name, comp in (("raw", None), ("snappy", compress)):
        data, handles, index_handle, _ = stm.table_file(entries, cmp, block_size, restart_interval, bits, comp)
        data = bytearray(data)
        data[handles[2][0] + 7] ^= 0x10  # the third data block: a checksum mismatch
        out[name] = {"data": bytes(data), "index_handle": index_handle, "handles": handles,
                     "table": gm.open_table(bytes(data), bits, uncompress)}
    return out


def _get_table_want(name):
    c = get_table_case()
    t = c[name]
    state, key_len, values, data_handle = [], [], [], []
    for k in c["probes"]:
        st, found, value = gm.table_get(t["table"], k, uncompress)
        idx = bm.seek(t["table"]["index"], k, bm.INTERNAL_KEY, value_is_handle=True)
        state.append(st)
        key_len.append(len(found) if st == gm.VALID else 0)
        values.append(value if st == gm.VALID else b"")
        data_handle.append(list(idx["handle"]) if idx["state"] == bm.VALID else [0, 0])
    return {"state": arr(state), "key_len": arr(key_len), "values": values, "data_handle": arr(data_handle)}


def _get_table_make(name):
    def make(torch):
        c = get_table_case()
        t = c[name]
        return {"image": u8(torch, t["data"]), "keys": u8(torch, c["keys"]),
                "key_offsets": dev(torch, c["key_offsets"]),
                "filter": u8(torch, t["table"]["filter"]), "index_handle": t["index_handle"]}
    return make


def _block_table_get(x, s):
    from lsbm_amd import block
    r = block.table_get(x["image"], x["index_handle"], x["keys"], x["key_offsets"], filter=x["filter"], verify=True,
                        bits_per_key=BITS, stream=s)

    def read():
        return {"state": ints(r.state), "key_len": ints(r.key_len), "values": cut(byts(x["image"]), ints(r.value)),
                "data_handle": ints(r.data_handle)}
    return read


def _sstable_table_get(x, s):
    from lsbm_amd import sstable
    r = sstable.table_get(x["image"], x["index_handle"], x["keys"], x["key_offsets"], filter=x["filter"], verify=True,
                          bits_per_key=BITS, stream=s)

    def read():
        return {"state": ints(r.state), "key_len": ints(r.key_len), "values": cut(byts(r.value_image), ints(r.value)),
                "data_handle": ints(r.data_handle)}
    return read


reg("block.table_get", ["state", "key_len", "data_handle"], _get_table_make("raw"), _block_table_get,
    lambda: _get_table_want("raw"))
reg("sstable.table_get", ["state", "key_len", "data_handle"], _get_table_make("snappy"), _sstable_table_get,
    lambda: _get_table_want("snappy"))


# ---------------------------------------------------------------- block and index builder
@cached
def build_case():
    return ho.build_case()


@cached
def build_windows():
    """Windows for the data blocks 7 bytes apart from 16 on, and for the two
    index blocks behind them: (block handles, index handles, output size)."""
    base0 = ho.build_model(build_case().bufs, build_case().arrays)
    sizes = base0["block_bytes"]
    pos = 16 + np.concatenate([[0], np.cumsum(sizes + 7)[:-1]])
    handles = np.stack([pos, sizes], 1).reshape(-1)
    want = ho.build_model(build_case().bufs, build_case().arrays, data_handles=handles)
    ipos = int(pos[-1] + sizes[-1]) + 9 + np.array([0, int(want["index_bytes"][0]) + 5])
    ihandles = np.stack([ipos, want["index_bytes"]], 1).reshape(-1)
    return handles, ihandles, int(ipos[-1] + want["index_bytes"][-1]) + 16, want


def _build_make(torch):
    c = build_case()
    handles, ihandles, size, want = build_windows()
    x = {k: u8(torch, v) for k, v in c.bufs.items()}
    x.update({k: dev(torch, v) for k, v in c.arrays.items()})
    x.update(out=filled(torch, size), handles=dev(torch, handles), ihandles=dev(torch, ihandles),
             block_first=dev(torch, want["block_first"]), table_block_first=dev(torch, want["table_block_first"]))
    return x


def _build_untouched(host):
    """The bytes of the output outside every window."""
    handles, ihandles, size, _ = build_windows()
    keep = np.ones(size, dtype=bool)
    for o, n in np.concatenate([handles, ihandles]).reshape(-1, 2).tolist():
        keep[o:o + n] = False
    return np.frombuffer(host, np.uint8)[keep].tobytes()


def _build_plan(x, s):
    from lsbm_amd import block_build
    p = block_build.plan(x["keys"], x["key_offsets"], x["values"], x["table_first"], ho.BUILD_BLOCK_SIZE,
                         ho.BUILD_RESTART, stream=s)

    def read():
        nb = len(build_windows()[3]["block_bytes"])
        return {"block_first": ints(p.block_first)[:nb + 1], "block_bytes": ints(p.block_bytes)[:nb],
                "table_block_first": ints(p.table_block_first), "plan_status": ints(p.status)}
    return read


def _build_build(x, s):
    from lsbm_amd import block_build
    built, status = block_build.build(x["keys"], x["key_offsets"], x["values"], x["vimage"], x["block_first"], x["out"],
                                      x["handles"], ho.BUILD_RESTART, stream=s)

    def read():
        host = byts(x["out"])
        return {"blocks": cut(host, build_windows()[0]), "built_bytes": ints(built), "build_status": ints(status),
                "index_blocks": cut(host, build_windows()[1]), "outside": _build_untouched(host)}
    return read


def _build_index(x, s):
    from lsbm_amd import block_build
    built, status = block_build.index_block(x["keys"], x["key_offsets"], x["block_first"], x["table_block_first"],
                                            x["handles"], cmp=bm.INTERNAL_KEY, out=x["out"], out_handles=x["ihandles"],
                                            stream=s)

    def read():
        host = byts(x["out"])
        return {"index_blocks": cut(host, build_windows()[1]), "index_bytes": ints(built), "index_status": ints(status),
                "blocks": cut(host, build_windows()[0]), "outside": _build_untouched(host)}
    return read


def _fill_blocks(handles):
    return [bytes([FILL]) * int(n) for n in np.asarray(handles).reshape(-1, 2)[:, 1]]


def _outside_want():
    handles, ihandles, size, _ = build_windows()
    return bytes([FILL]) * (size - int(handles[1::2].sum()) - int(ihandles[1::2].sum()))


reg("block_build.plan", ["block_first", "block_bytes", "table_block_first", "plan_status"], _build_make, _build_plan,
    lambda: pick(build_windows()[3], "block_first", "block_bytes", "table_block_first", "plan_status"))
reg("block_build.build", ["built_bytes", "build_status"], _build_make, _build_build,
    lambda: dict(pick(build_windows()[3], "blocks", "built_bytes", "build_status"),
                 index_blocks=_fill_blocks(build_windows()[1]), outside=_outside_want()))
reg("block_build.index_block", ["index_bytes", "index_status"], _build_make, _build_index,
    lambda: dict(pick(build_windows()[3], "index_blocks", "index_bytes", "index_status"),
                 blocks=_fill_blocks(build_windows()[0]), outside=_outside_want()))


# ---------------------------------------------------------------- whole tables: one, many, finished from blocks
@cached
def tables_case():
    """Three small tables of alternating compressible and random blocks (the
    middle one without entries), bytewise keys, a filter block each."""
    tables = [tc._blocks_of_kinds("rxr", 128, 4, 11), [], tc._blocks_of_kinds("xr", 128, 4, 12)]
    entries = [e for t in tables for e in t]
    first = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    return tables, entries, first


TABLE_PARAMS = (bm.BYTEWISE, 128, 4, BITS)


def _entries_make(entries):
    """[(key, value)] as test_sstable.Entries lays them out."""
    keys, koff = packed([k for k, _ in entries])
    image, values = bytearray(b"\x5a"), []
    for _, v in entries:
        values += [len(image), len(v)]
        image += v

    def make(torch):
        return {"keys": u8(torch, keys), "key_offsets": dev(torch, koff), "values": dev(torch, values),
                "image": u8(torch, bytes(image))}
    return make


def _tables_make(torch):
    _, entries, first = tables_case()
    x = _entries_make(entries)(torch)
    x["table_first"] = dev(torch, first)
    return x


def _tables_out(res, n):
    return {"tables": [byts(res.table(t)) for t in range(n)],
            "data_handles": [ints(res.table_data_handles(t)).reshape(-1, 2) for t in range(n)],
            "index_handles": arr([res.index_handle(t) for t in range(n)]),
            "smallest": list(res.smallest), "largest": list(res.largest)}


def _tables_want(comp):
    tables, _, _ = tables_case()
    files = [stm.table_file(t, *TABLE_PARAMS, comp) for t in tables]
    return {"tables": [f[0] for f in files], "data_handles": [arr(f[1]).reshape(-1, 2) for f in files],
            "index_handles": arr([f[2] for f in files]), "smallest": [t[0][0] if t else None for t in tables],
            "largest": [t[-1][0] if t else None for t in tables]}


def _write_tables(x, s):
    from lsbm_amd import sstable
    res = sstable.write_tables(x["keys"], x["key_offsets"], x["values"], x["image"], x["table_first"], *TABLE_PARAMS,
                               compression=1, stream=s)

    def read():
        return _tables_out(res, 3)
    return read


def _finish_make(torch):
    """The data blocks of all tables built by the model, raw, back to back."""
    from lsbm_amd import sstable
    tables, _, first = tables_case()
    x = _tables_make(torch)
    block_first, tbf, blocks = [0], [0], []
    for t, es in enumerate(tables):
        f, bs = stm.data_blocks(es, TABLE_PARAMS[1], TABLE_PARAMS[2])
        block_first += [int(first[t]) + e for e in f[1:]]
        blocks += bs
        tbf.append(len(blocks))
    raw, off = packed(blocks)
    x.update(block_first=dev(torch, block_first), table_block_first=dev(torch, tbf),
             blocks=sstable._Blocks(u8(torch, raw), dev(torch, np.stack([off[:-1], np.diff(off)], 1).reshape(-1)), None,
                                    None, None))
    return x


def _finish_tables(x, s):
    from lsbm_amd import sstable
    res = sstable.finish_tables(x["keys"], x["key_offsets"], x["block_first"], x["table_block_first"], x["blocks"],
                                TABLE_PARAMS[0], TABLE_PARAMS[2], TABLE_PARAMS[3], compression=0, stream=s)

    def read():
        return _tables_out(res, 3)
    return read


def _one_table_out(image, handles, index_handle):
    return {"table": byts(image), "data_handles": ints(handles).reshape(-1, 2), "index_handle": arr(index_handle)}


def _one_table_want(entries, params, comp):
    data, handles, index_handle, _ = stm.table_file(entries, *params, comp)
    return {"table": data, "data_handles": arr(handles).reshape(-1, 2), "index_handle": arr(index_handle)}


def _write_table(x, s):
    from lsbm_amd import sstable
    got = sstable.write_table(x["keys"], x["key_offsets"], x["values"], x["image"], *TABLE_PARAMS, compression=1,
                              stream=s)

    def read():
        return _one_table_out(*got)
    return read


def _table_build(x, s):
    from lsbm_amd import block_build
    cmp, block_size, restart_interval, bits = tc.CASES["bloom_internal"]
    got = block_build.table_build(x["keys"], x["key_offsets"], x["values"], x["image"], cmp, block_size,
                                  restart_interval, bits, stream=s)

    def read():
        return _one_table_out(*got)
    return read


reg("sstable.write_tables", ["tables", "data_handles", "index_handles"], _tables_make, _write_tables,
    lambda: _tables_want(compress))
reg("sstable.finish_tables", ["tables", "data_handles", "index_handles"], _finish_make, _finish_tables,
    lambda: _tables_want(None))
reg("sstable.write_table", ["table", "data_handles"], lambda torch: _entries_make(tables_case()[0][0])(torch),
    _write_table, lambda: _one_table_want(tables_case()[0][0], TABLE_PARAMS, compress))
reg("block_build.table_build", ["table", "data_handles"],
    lambda torch: _entries_make(tc.entries("bloom_internal"))(torch), _table_build,
    lambda: _one_table_want(tc.entries("bloom_internal"), tc.CASES["bloom_internal"], None))

# ---------------------------------------------------------------- table pack: plan, mover, ReadBlock
PACK_RAW = [1, 15, 4097, 300, 64, 17]
PACK_COMP = [-1, 9, 2000, 290, 20, -1]


def _pack_plan(x, s):
    from lsbm_amd import sstable
    types, handles, end = sstable.pack_plan(x["raw_len"], x["comp_len"], 77, 5, stream=s)

    def read():
        return {"types": ints(types), "handles": ints(handles), "end": ints(end)}
    return read


reg("sstable.pack_plan", ["types", "handles", "end"],
    lambda torch: {"raw_len": dev(torch, PACK_RAW), "comp_len": dev(torch, PACK_COMP)}, _pack_plan,
    lambda: ho.pack_plan_model(PACK_RAW, PACK_COMP, 77, 5))

# the mover: two good blocks, one whose source is 2^32 past its image
# (LSBM_BUILD_BAD_INPUT) and one whose window is 2^32 past the output
# (LSBM_BUILD_NO_ROOM); "nothing is written for that block"
PACK_DATA = bytes(range(200))
PACK_RAW_HANDLES = [0, 50, 60 + LINE, 50, 120, 50, 10, 50]
PACK_HANDLES = [8, 50, 108, 50, 208, 50, 308 + LINE, 50]


def _pack_make(torch):
    return {"raw": u8(torch, PACK_DATA), "raw_handles": dev(torch, PACK_RAW_HANDLES),
            "handles": dev(torch, PACK_HANDLES),
            "types": dev(torch, [0, 0, 0, 0], np.uint8), "out": filled(torch, 616)}


def _pack(x, s):
    from lsbm_amd import sstable
    status = sstable.pack(x["raw"], x["raw_handles"], None, None, x["types"], x["handles"], x["out"], gap=0, stream=s)

    def read():
        return {"status": ints(status), "out": byts(x["out"])}
    return read


def _pack_want():
    out = bytearray([FILL]) * 616
    out[8:58], out[208:258] = PACK_DATA[:50], PACK_DATA[120:170]
    return {"status": arr([0, 2, 0, 1]), "out": bytes(out)}


reg("sstable.pack", ["status"], _pack_make, _pack, _pack_want)


@cached
def read_case():
    """Every block of table 0 of tables_case (snappy and raw data blocks, the
    filter, metaindex and index blocks) in file order, one of them damaged, and
    a handle past the file."""
    data, handles, index_handle, _ = stm.table_file(tables_case()[0][0], *TABLE_PARAMS, compress)
    t = stm.read_table(data, uncompress)
    hs = list(handles) + [t["filter_handle"], t["meta_handle"], index_handle, (len(data) - 3, 10)]
    data = bytearray(data)
    data[hs[1][0] + 3] ^= 1
    want = [stm.read_block(bytes(data), h, uncompress) for h in hs]
    return bytes(data), arr(hs).reshape(-1), want


def _read_blocks(x, s):
    from lsbm_amd import sstable
    contents, out_handles, status = sstable.read_blocks(x["image"], x["handles"], stream=s)

    def read():
        return {"blocks": cut(byts(contents), ints(out_handles)), "status": ints(status)}
    return read


reg("sstable.read_blocks", ["blocks", "status"],
    lambda torch: {"image": u8(torch, read_case()[0]), "handles": dev(torch, read_case()[1])}, _read_blocks,
    lambda: {"blocks": [c for _, c, _ in read_case()[2]], "status": arr([st for st, _, _ in read_case()[2]])})


# ---------------------------------------------------------------- the batched table finish, step by step
PPT_RAW, PPT_TBF, PPT_FIRST = [100, 200, 300, 50, 60], [0, 2, 2, 5], [1 << 33, 7, 0]


def _ppt_want():
    types, handles, end = [], [], []
    for t in range(3):
        w = ho.pack_plan_model(PPT_RAW[PPT_TBF[t]:PPT_TBF[t + 1]], [-1] * (PPT_TBF[t + 1] - PPT_TBF[t]), PPT_FIRST[t],
                               5)
        types += w["types"].tolist()
        handles += w["handles"].tolist()
        end += w["end"].tolist()
    return {"types": arr(types), "handles": arr(handles), "end": arr(end), "status": arr([0, 0, 0])}


def _ppt(x, s):
    from lsbm_amd import sstable
    types, handles, end, status = sstable.pack_plan_tables(x["raw_len"], None, x["tbf"], x["first"], 5, stream=s)

    def read():
        return {"types": ints(types), "handles": ints(handles), "end": ints(end), "status": ints(status)}
    return read


reg("sstable.pack_plan_tables", ["handles", "end", "types", "status"],
    lambda torch: {"raw_len": dev(torch, PPT_RAW), "tbf": dev(torch, PPT_TBF), "first": dev(torch, PPT_FIRST)}, _ppt,
    _ppt_want)

LAYOUT_NAMES = ["many_256", "above_4k", "single"]


@cached
def layout_case():
    """Three tables of tablewritemodel.LAYOUT_CASES, their filter blocks'
    windows 3 bytes apart from 7 on, and the model's layout of each."""
    from test_table_write_gpu import layout_inputs
    bf, tbf, handles, ends, per = layout_inputs(LAYOUT_NAMES)
    want = [tw.filter_layout(start, first, end, BITS) for start, first, end in per]
    win, at = [], 7
    for w in want:
        win += [at, w["size"]]
        at += w["size"] + 3
    return {"block_first": bf, "tbf": tbf, "handles": handles, "ends": ends, "want": want, "win": win, "size": at + 9}


def _layout_make(torch):
    c = layout_case()
    return {"block_first": dev(torch, c["block_first"]), "tbf": dev(torch, c["tbf"]),
            "handles": dev(torch, c["handles"]),
            "ends": dev(torch, c["ends"]), "win": dev(torch, c["win"]), "out": filled(torch, c["size"]),
            "sizes": dev(torch, [w["size"] for w in c["want"]])}


def _layout(x, s):
    from lsbm_amd import sstable
    c = layout_case()
    lay = sstable.filter_layout(x["block_first"], x["tbf"], x["handles"], x["ends"], BITS, x["out"], x["win"],
                                sum(w["count"] for w in c["want"]), stream=s)

    def read():
        host = np.frombuffer(byts(x["out"]), np.uint8).copy()
        for t, w in enumerate(c["want"]):  # (the filters' own bytes are lsbm_bloom_build_dev's: left alone here)
            assert (host[c["win"][2 * t]:c["win"][2 * t] + w["data_bytes"]] == FILL).all()
        return {"size": ints(lay.size), "count": ints(lay.count), "filter_first": ints(lay.filter_first),
                "filter_out": ints(lay.filter_out), "status": ints(lay.status), "out": host.tobytes()}
    return read


def _layout_want():
    c = layout_case()
    out = bytearray([FILL]) * c["size"]
    for t, w in enumerate(c["want"]):
        at = c["win"][2 * t] + w["data_bytes"]
        out[at:at + len(w["trailer"])] = w["trailer"]
    keys = [k for w in c["want"] for k in w["filter_keys"]]
    return {"size": arr([w["size"] for w in c["want"]]), "count": arr([w["count"] for w in c["want"]]),
            "filter_first": arr([k0 for k0, _ in keys] + [c["block_first"][-1]]),
            "filter_out": arr([c["win"][2 * t] + o for t, w in enumerate(c["want"]) for o in w["filter_out"]]),
            "status": arr([0, 0, 0]), "out": bytes(out)}


reg("sstable.filter_layout", ["size", "count", "filter_first", "filter_out", "status"], _layout_make, _layout,
    _layout_want)


def _meta_blocks():
    """One metaindex block per table of layout_case: the filter block's handle
    under its name, one restart."""
    c = layout_case()
    out = []
    for end, w in zip(c["ends"], c["want"]):
        h = bd.encode_handle(end, w["size"])
        out.append(b"\0\x21" + bytes([len(h)]) + bd.FILTER_KEY + h + b"\0\0\0\0\1\0\0\0")
    return out


def _meta_make(torch):
    x = _layout_make(torch)
    blocks = _meta_blocks()
    win, at = [], 8
    for b in blocks:
        win += [at, len(b)]
        at += len(b) + 8
    x.update(mwin=dev(torch, win), mout=filled(torch, at), mwin_host=win)
    return x


def _meta(x, s):
    from lsbm_amd import sstable
    sizes, status = sstable.metaindex_blocks(x["ends"], x["sizes"], x["mout"], x["mwin"], stream=s)

    def read():
        host = byts(x["mout"])
        return {"sizes": ints(sizes), "status": ints(status), "blocks": cut(host, x["mwin_host"]),
                "between": bytes(b for i, b in enumerate(host) if not any(
                    o <= i < o + n for o, n in np.array(x["mwin_host"]).reshape(-1, 2).tolist()))}
    return read


reg("sstable.metaindex_blocks", ["sizes", "status"], _meta_make, _meta,
    lambda: {"sizes": arr([len(b) for b in _meta_blocks()]), "status": arr([0, 0, 0]), "blocks": _meta_blocks(),
             "between": bytes([FILL]) * (8 * (len(_meta_blocks()) + 1))})


def _place_make(torch):
    return {"data_handles": dev(torch, [0, 995, 0, 495]), "tbf": dev(torch, [0, 1, 2]),
            "tail_handles": dev(torch, [1000, 10, 1015, 20, 500, 10, 515, 20]), "tail_end": dev(torch, [1040, 540]),
            "base": dev(torch, [0, 1280]), "arena": filled(torch, 1280 + 588 + 64)}


def _place(x, s):
    from lsbm_amd import sstable
    p = sstable.place_tables(x["data_handles"], x["tbf"], x["tail_handles"], 2, x["tail_end"], x["base"], x["arena"],
                             stream=s)

    def read():
        return {"table_size": ints(p.table_size), "data_handles": ints(p.data_handles),
                "tail_handles": ints(p.tail_handles),
                "status": ints(p.status), "arena": byts(x["arena"])}
    return read


def _place_want():
    arena = bytearray([FILL]) * (1280 + 588 + 64)
    arena[1040:1088] = bd.footer((1000, 10), (1015, 20))
    arena[1280 + 540:1280 + 588] = bd.footer((500, 10), (515, 20))
    return {"table_size": arr([1088, 588]), "data_handles": arr([0, 995, 1280, 495]),
            "tail_handles": arr([1000, 10, 1015, 20, 1780, 10, 1795, 20]), "status": arr([0, 0]), "arena": bytes(arena)}


reg("sstable.place_tables", ["table_size", "data_handles", "tail_handles", "status"], _place_make, _place, _place_want)


# ---------------------------------------------------------------- merge and compaction
@cached
def merge_case():
    return ho.merge_case()


@cached
def merge_want():
    c = merge_case()
    return ho.merge_model(c.bufs, c.arrays, True)


def _merge_make(torch):
    c = merge_case()
    x = {k: u8(torch, v) for k, v in c.bufs.items()}
    x.update({k: dev(torch, v) for k, v in c.arrays.items()})
    return x


MERGE_RULE = dict(cmp=bm.INTERNAL_KEY, drop=True, smallest_snapshot=15, bottom_level=True)


def _merge_plan(x, s):
    from lsbm_amd import merge
    p = merge.plan(x["keys"], x["key_offsets"], x["run_first"], stream=s, **MERGE_RULE)

    def read():
        n_out = int(merge_want()["counts"][0])
        return {"source": ints(p.source)[:n_out], "out_key_offsets": ints(p.out_key_offsets)[:n_out + 1],
                "counts": ints(p.counts), "run_status": ints(p.run_status)}
    return read


def _gather_make(torch):
    from lsbm_amd import merge
    x = _merge_make(torch)
    x["plan"] = merge.plan(x["keys"], x["key_offsets"], x["run_first"], **MERGE_RULE)
    return x


def _merge_gather(x, s):
    from lsbm_amd import merge
    g = merge.gather(x["keys"], x["key_offsets"], x["values"], x["plan"], stream=s)

    def read():
        n_out, nbytes = (int(v) for v in merge_want()["counts"])
        return {"out_keys": byts(g.keys)[:nbytes], "out_key_offsets": ints(g.key_offsets)[:n_out + 1],
                "out_values": ints(g.values).reshape(-1, 2)[:n_out], "gather_status": ints(g.status)}
    return read


def _merge_merge(x, s):
    from lsbm_amd import merge
    m = merge.merge(x["keys"], x["key_offsets"], x["values"], x["run_first"], stream=s, **MERGE_RULE)

    def read():
        return {"out_keys": byts(m.keys), "out_key_offsets": ints(m.key_offsets),
                "out_values": ints(m.values).reshape(-1, 2),
                "source": ints(m.source), "run_status": ints(m.run_status)}
    return read


reg("merge.plan", ["source", "out_key_offsets", "counts", "run_status"], _merge_make, _merge_plan,
    lambda: pick(merge_want(), "source", "out_key_offsets", "counts", "run_status"))
reg("merge.gather", ["out_keys", "out_key_offsets", "out_values", "gather_status"], _gather_make, _merge_gather,
    lambda: pick(merge_want(), "out_keys", "out_key_offsets", "out_values", "gather_status"))
reg("merge.merge", ["out_keys", "out_key_offsets", "out_values", "source"], _merge_make, _merge_merge,
    lambda: pick(merge_want(), "out_keys", "out_key_offsets", "out_values", "source", "run_status"))


def _compact_rule():
    c = dict(tc.COMPACTION)
    return c.pop("cmp"), c.pop("max_file_size"), c


@cached
def compact_inputs(snappy):
    cmp, _, c = _compact_rule()
    return [stm.table_file(run, cmp, c["block_size"], c["restart_interval"], c["bits_per_key"],
                           compress if snappy else None) for run in tc.compaction_runs()]


def _compact_make(snappy):
    def make(torch):
        files = compact_inputs(snappy)
        return {"images": [u8(torch, f[0]) for f in files], "index_handles": [f[2] for f in files],
                "data_handles": [arr(f[1]).reshape(-1) for f in files]}
    return make


def _compact_out(out):
    return {"tables": [byts(o.image) for o in out], "data_handles": [ints(o.data_handles).reshape(-1, 2) for o in out],
            "index_handles": arr([o.index_handle for o in out])}


def _compact_want(snappy):
    cmp, max_file_size, c = _compact_rule()
    files = (stm.compact(tc.compaction_runs(), cmp, max_file_size, compress=compress, **c) if snappy else
             mm.compact(tc.compaction_runs(), cmp, max_file_size, **c))
    read = [stm.read_table(f, uncompress) for f in files]
    assert len(files) >= 3
    return {"tables": files, "data_handles": [arr(r["data_handles"]).reshape(-1, 2) for r in read],
            "index_handles": arr([r["index_handle"] for r in read])}


def _merge_compact(x, s):
    from lsbm_amd import merge
    cmp, max_file_size, c = _compact_rule()
    out = merge.compact(x["images"], x["data_handles"], max_file_size, cmp=cmp, stream=s, **c)

    def read():
        return _compact_out(out)
    return read


def _sstable_compact(x, s):
    from lsbm_amd import sstable
    cmp, max_file_size, c = _compact_rule()
    out = sstable.compact(x["images"], None, max_file_size, index_handles=x["index_handles"], cmp=cmp, compression=1,
                          stream=s, **c)

    def read():
        return _compact_out(out)
    return read


reg("merge.compact", ["tables", "data_handles", "index_handles"], _compact_make(False), _merge_compact,
    lambda: _compact_want(False))
reg("sstable.compact", ["tables", "data_handles", "index_handles"], _compact_make(True), _sstable_compact,
    lambda: _compact_want(True))

# ---------------------------------------------------------------- memtable: WriteBatch decode and sort
@cached
def memtable_case():
    return ho.memtable_case()


@cached
def memtable_want():
    c = memtable_case()
    return ho.memtable_model(c.bufs, c.arrays)


def _memtable_make(torch):
    c = memtable_case()
    return {"image": u8(torch, c.bufs["image"]), "records": dev(torch, c.arrays["records"])}


def _memtable_scan(x, s):
    from lsbm_amd import memtable
    counts, status = memtable.scan(x["image"], x["records"], stream=s)

    def read():
        return {"counts": ints(counts), "status": ints(status)}
    return read


def _memtable_decode(x, s):
    """Without entry_base / key_base: scan, the running sums and the host read."""
    from lsbm_amd import memtable
    d = memtable.decode(x["image"], x["records"], stream=s)

    def read():
        return {"keys": byts(d.keys), "key_offsets": ints(d.key_offsets), "values": ints(d.values).reshape(-1, 2),
                "status": ints(d.status), "max_sequence": arr([memtable.max_sequence_of(d.max_sequence)])}
    return read


reg("memtable.scan", ["counts", "status"], _memtable_make, _memtable_scan,
    lambda: pick(memtable_want(), "counts", "status"))
reg("memtable.decode", ["keys", "key_offsets", "values", "status", "max_sequence"], _memtable_make, _memtable_decode,
    lambda: pick(memtable_want(), "keys", "key_offsets", "values", "status", "max_sequence"))

SEG_FIRST = [0, 100, 100, 257]


@cached
def sort_case():
    return ho.sort_case()


def _sort_make(torch):
    c = sort_case()
    return {"keys": u8(torch, c.bufs["keys"]), "key_offsets": dev(torch, c.arrays["key_offsets"]),
            "seg_first": dev(torch, SEG_FIRST)}


def _sort_out(p):
    return {"source": ints(p.source), "out_key_offsets": ints(p.out_key_offsets), "counts": ints(p.counts),
            "status": ints(p.run_status)}


def _sort(x, s):
    from lsbm_amd import memtable
    p = memtable.sort(x["keys"], x["key_offsets"], stream=s)

    def read():
        return _sort_out(p)
    return read


def _sort_segments(x, s):
    from lsbm_amd import memtable
    p = memtable.sort_segments(x["keys"], x["key_offsets"], x["seg_first"], stream=s)

    def read():
        return _sort_out(p)
    return read


def _sort_segments_want():
    c = sort_case()
    keys = split(c.bufs["keys"], c.arrays["key_offsets"])
    order = [lo + i for lo, hi in zip(SEG_FIRST[:-1], SEG_FIRST[1:]) for i in mt.order(keys[lo:hi])]
    return {"source": arr(order), "out_key_offsets": np.cumsum([0] + [len(keys[i]) for i in order]).astype(np.int64),
            "counts": arr([len(keys), sum(len(k) for k in keys)]), "status": arr([0])}


reg("memtable.sort", ["source", "out_key_offsets", "counts", "status"], _sort_make, _sort,
    lambda: ho.sort_model(sort_case().bufs, sort_case().arrays))
reg("memtable.sort_segments", ["source", "out_key_offsets", "counts", "status"], _sort_make, _sort_segments,
    _sort_segments_want)


# ---------------------------------------------------------------- memtable: a log to a Level-0 table
@cached
def flush_case():
    """The smallest log of memtable_fixture.json that has five records or more
    and writes a table: its records, iteration and table file are the
    reference's."""
    cases, _ = mtc.load()
    c = min((c for c in cases if c["table"] is not None and len(c["record_lens"]) >= 5), key=lambda c: len(c["log"]))
    payloads = mt.log_records(c["log"])
    image, recs = b"", []
    for p in payloads:
        recs.append((len(image), len(p)))
        image += p
    n = len(recs)
    c = dict(c, payloads=payloads, image=image, recs=recs, kw=dict(
        block_size=c["block_size"], restart_interval=c["restart_interval"], bits_per_key=c["bits_per_key"]))
    c["mem_first"] = [0, 1, n // 2, n // 2, n]
    c["max_sequence"] = mt.max_sequence(image, recs)
    return c


def _flush_make(torch):
    c = flush_case()
    return {"image": u8(torch, c["image"]), "records": dev(torch, arr(c["recs"]).reshape(-1)),
            "log": u8(torch, c["log"])}


def _entries(x, s):
    from lsbm_amd import memtable
    e = memtable.entries(x["image"], x["records"], paranoid=True, stream=s)

    def read():
        keys = split(byts(e.keys), ints(e.key_offsets))
        return {"entries": list(zip(keys, cut(flush_case()["image"], ints(e.values)))), "status": ints(e.status),
                "max_sequence": e.max_sequence}
    return read


def _flush_out(f):
    return {"table": byts(f.image), "data_handles": ints(f.data_handles).reshape(-1, 2),
            "index_handle": arr(f.index_handle),
            "smallest": f.smallest, "largest": f.largest, "max_sequence": f.max_sequence,
            "status": ints(f.status) if hasattr(f.status, "cpu") else arr(f.status)}


def _flush_want(recs=None):
    c = flush_case()
    recs = c["recs"] if recs is None else recs
    ents, status, max_seq = mt.entries(c["image"], recs)
    table = mt.table_file(ents, **c["kw"])
    read = stm.read_table(table, uncompress)
    return {"table": table, "data_handles": arr(read["data_handles"]).reshape(-1, 2),
            "index_handle": arr(read["index_handle"]), "smallest": ents[0][0], "largest": ents[-1][0],
            "max_sequence": max_seq, "status": arr(status)}


def _flush(x, s):
    from lsbm_amd import memtable
    f = memtable.flush(x["image"], x["records"], stream=s, **flush_case()["kw"])

    def read():
        return _flush_out(f)
    return read


def _flush_many(x, s):
    from lsbm_amd import memtable
    got = memtable.flush_many(x["image"], x["records"], flush_case()["mem_first"], stream=s, **flush_case()["kw"])

    def read():
        return {"flushes": [_flush_out(f) for f in got]}
    return read


def _flush_many_want():
    c = flush_case()
    slices = [c["recs"][lo:hi] for lo, hi in zip(c["mem_first"][:-1], c["mem_first"][1:])]
    return {"flushes": [_flush_want(r) for r in slices if r and mt.entries(c["image"], r)[0]]}


def _log_records(x, s):
    from lsbm_amd import memtable
    image, records = memtable.log_records(flush_case()["log"], stream=s)

    def read():
        return {"records": cut(byts(image), ints(records))}
    return read


def _recover_log(x, s):
    from lsbm_amd import memtable
    f = memtable.recover_log(flush_case()["log"], stream=s, **flush_case()["kw"])

    def read():
        return _flush_out(f)
    return read


def _recover(x, s):
    from lsbm_amd import memtable
    r = memtable.recover(x["log"], stream=s, **flush_case()["kw"])

    def read():
        return dict(_flush_out(r.flush), events=ints(r.events).reshape(-1, 4), recover_status=r.status)
    return read


def _recover_all(x, s):
    from lsbm_amd import memtable
    r = memtable.recover_all(x["log"], stream=s, **flush_case()["kw"])

    def read():
        return {"flushes": [_flush_out(f) for f in r.flushes], "mem_first": list(r.mem_first),
                "events": ints(r.events).reshape(-1, 4), "recover_status": r.status}
    return read


def _fixture_table_want():
    """flush's result over the whole log: the table is the reference's own."""
    w = _flush_want()
    assert w["table"] == flush_case()["table"] and w["smallest"] == flush_case()["iteration"][0][0]
    return w


reg("memtable.entries", ["entries", "status"], _flush_make, _entries,
    lambda: {"entries": [tuple(e) for e in flush_case()["iteration"]], "status": arr([0] * len(flush_case()["recs"])),
             "max_sequence": flush_case()["max_sequence"]})
reg("memtable.flush", ["table", "data_handles"], _flush_make, _flush, _fixture_table_want)
reg("memtable.flush_many", ["flushes"], _flush_make, _flush_many, _flush_many_want)
reg("memtable.log_records", ["records"], _flush_make, _log_records, lambda: {"records": flush_case()["payloads"]})
reg("memtable.recover_log", ["table", "data_handles"], _flush_make, _recover_log, _fixture_table_want)
reg("memtable.recover", ["table", "data_handles"], _flush_make, _recover,
    lambda: dict(_fixture_table_want(), events=np.zeros((0, 4), dtype=np.int64), recover_status=None))
reg("memtable.recover_all", ["flushes"], _flush_make, _recover_all,
    lambda: {"flushes": [_fixture_table_want()], "mem_first": [0, len(flush_case()["recs"])],
             "events": np.zeros((0, 4), dtype=np.int64), "recover_status": None})


# ---------------------------------------------------------------- memtable: heights and the cut
N_HEIGHTS = 300


def _heights(x, s):
    from lsbm_amd import memtable
    h, rnd = memtable.heights(N_HEIGHTS, stream=s)

    def read():
        return {"heights": ints(h), "rnd": ints(rnd)}
    return read


def _heights_want():
    h, rnd = mcm.heights(mcm.SEED, N_HEIGHTS)
    return {"heights": arr(h), "rnd": arr([rnd])}


reg("memtable.heights", ["heights", "rnd"], lambda torch: {}, _heights, _heights_want)

# ten records of four entries of 24-byte internal keys and 300-byte values:
# about 13 KiB in all, so that a write buffer of 8 KiB closes one memtable
CUT_ENTRIES = [(24, 300, 1)] * 39 + [(24, 0, 0)]
CUT_BASE = list(range(0, 41, 4))
CUT_STATUS = [0, 0, 1, 0, 0, 0, 0, 0, 0, 0]  # (the third record is LSBM_WB_TOO_SMALL: counted by none)
CUT_BUFFER = 8192


def _cut_make(torch):
    koff = np.concatenate([[0], np.cumsum([ikl for ikl, _, _ in CUT_ENTRIES])])
    return {"key_offsets": dev(torch, koff), "values": dev(torch, [x for _, vl, _ in CUT_ENTRIES for x in (7, vl)]),
            "entry_base": dev(torch, CUT_BASE), "rec_status": dev(torch, CUT_STATUS, np.int32)}


def _cut(x, s):
    from lsbm_amd import memtable
    r = memtable.cut(x["key_offsets"], x["values"], x["entry_base"], memtable.RECOVER, CUT_BUFFER,
                     rec_status=x["rec_status"], stream=s)

    def read():
        n_mem = int(r.counts.cpu()[0])
        return {"status": ints(r.status), "usage": ints(r.usage), "mem_first": ints(r.mem_first)[:n_mem + 1],
                "mem_usage": ints(r.mem_usage)[:n_mem], "counts": ints(r.counts), "state": ints(r.state)}
    return read


def _cut_want():
    w = mcm.cut(CUT_ENTRIES, CUT_BASE, CUT_STATUS, mcm.RECOVER, CUT_BUFFER)
    assert w["counts"][0] >= 2
    return {k: arr([v] if k == "status" else v) for k, v in w.items()}


reg("memtable.cut", ["usage", "mem_first", "mem_usage", "counts", "state", "status"], _cut_make, _cut, _cut_want)


# ---------------------------------------------------------------- DB::Get: the kernels
@cached
def get_case():
    return ho.get_case()


@cached
def get_want():
    c = get_case()
    return ho.get_model(c.bufs, c.arrays)


GET_VISIBLE = [1, 1, 0, 1, 1, 1, 1, 0]


def _get_make(torch):
    from lsbm_amd import db
    c, w = get_case(), get_want()
    x = {k: u8(torch, v) for k, v in c.bufs.items()}
    x.update({k: dev(torch, v) for k, v in c.arrays.items()})
    n = len(c.arrays["state"])
    x.update(n=n, lkeys=u8(torch, w["lookup_keys"]), lk_off=dev(torch, w["lookup_offsets"]),
             state=dev(torch, c.arrays["state"], np.int32), run_first=dev(torch, ho.GET_RUN_FIRST),
             run_flags=dev(torch, ho.GET_RUN_FLAGS, np.int32), visible=dev(torch, GET_VISIBLE, np.uint8),
             mem=db.MemTable(x["mem"], x["mem_offsets"], x["mem_values"], x["vimage"]))
    x["verdicts"] = db.new_verdicts(n, "cuda")
    # the smallest refused inputs: two lookup keys, the first of them 7 bytes long; a found key that is
    # longer than its window
    a, b = gm.lookup_key(b"a", 9), gm.lookup_key(b"b", 9)
    x["short"] = (u8(torch, a + b), dev(torch, [0, 7, 18]), db.new_verdicts(2, "cuda"))
    key, longer = gm.lookup_key(b"user", 9), gm.lookup_key(b"user-longer", 4)
    x["tight"] = (dev(torch, [gm.VALID, gm.VALID], np.int32), dev(torch, [len(key), len(longer)]),
                  u8(torch, key + longer[:len(key)]), dev(torch, [0, len(key), 2 * len(key)]), dev(torch, [0, 1, 0, 1]),
                  u8(torch, key + key), dev(torch, [0, len(key), 2 * len(key)]), db.new_verdicts(2, "cuda"))
    lens = [len(g) for g in w["gathered"]]
    x["gather_offsets"] = dev(torch, 8 + np.concatenate([[0], np.cumsum(lens)]))
    x["gather_out"] = filled(torch, 8 + sum(lens) + 8)
    x["save_value"] = dev(torch, w["save_value"].reshape(-1))
    x["save_where"] = dev(torch, w["save_where"], np.int32)
    bad = w["save_value"].copy()
    hit = int(np.nonzero((w["save_where"] >= 0) & (bad[:, 1] > 0))[0][2])
    bad[hit, 0] += LINE  # a selected slice 2^32 past the image: that query is not copied, the others are
    x["bad_slices"], x["bad_out"], x["hit"] = dev(torch, bad.reshape(-1)), filled(torch, 8 + sum(lens) + 8), hit
    return x


def _verdicts_out(v, tag):
    verdict, value, where = v
    return {tag + "_verdict": ints(verdict), tag + "_value": ints(value), tag + "_where": ints(where)}


UNTOUCHED = {"refused_verdict": arr([0, 0]), "refused_value": np.zeros((2, 2), dtype=np.int64),
             "refused_where": arr([-1, -1]), "refused_status": arr([2])}


def _lookup_keys(x, s):
    from lsbm_amd import db
    keys, off, status = db.lookup_keys(x["users"][:-1], x["user_offsets"], ho.GET_SNAPSHOT, stream=s)

    def read():
        return {"lookup_keys": byts(keys), "lookup_offsets": ints(off), "lookup_status": ints(status)}
    return read


def _memtable_probe(x, s):
    from lsbm_amd import db
    st = db.memtable_probe(x["mem"], x["lkeys"], x["lk_off"], ho.GET_SOURCE, *x["verdicts"], stream=s)
    keys, off, v = x["short"]
    refused = db.memtable_probe(x["mem"], keys, off, 0, *v, stream=s)

    def read():
        return dict(_verdicts_out(x["verdicts"], "mem"), status=ints(st), refused_status=ints(refused),
                    **_verdicts_out(v, "refused"))
    return read


def _find_file(x, s):
    from lsbm_amd import db
    file, st = db.find_file(x["bounds"], x["bound_offsets"], x["run_first"], x["run_flags"], x["visible"], x["lkeys"],
                            x["lk_off"], stream=s)

    def read():
        return {"file": ints(file), "status": ints(st)}
    return read


def _save_value(x, s):
    from lsbm_amd import db
    st = db.save_value(x["state"], x["key_len"], x["found"], x["found_offsets"], x["value_in"], x["lkeys"], x["lk_off"],
                       ho.GET_SOURCE + 1, *x["verdicts"], stream=s)
    *tight, v = x["tight"]
    refused = db.save_value(*tight, 1, *v, stream=s)

    def read():
        return dict(_verdicts_out(x["verdicts"], "save"), status=ints(st), refused_status=ints(refused),
                    **_verdicts_out(v, "refused"))
    return read


def _slices_gather(x, s):
    from lsbm_amd import db
    lo, hi = ho.GET_SOURCE + 1, ho.GET_SOURCE + 2
    st = db.slices_gather(x["vimage"], x["save_value"], x["save_where"], lo, hi, x["gather_out"], x["gather_offsets"],
                          stream=s)
    refused = db.slices_gather(x["vimage"][:len(get_case().bufs["vimage"])], x["bad_slices"], x["save_where"], lo, hi,
                               x["bad_out"], x["gather_offsets"], stream=s)

    def read():
        off = ints(x["gather_offsets"])
        return {"gathered": split(byts(x["gather_out"]), off), "status": ints(st), "refused_status": ints(refused),
                "refused_gathered": split(byts(x["bad_out"]), off), "guards": byts(x["gather_out"])[:8] +
                byts(x["gather_out"])[int(off[-1]):] + byts(x["bad_out"])[:8] + byts(x["bad_out"])[int(off[-1]):]}
    return read


def _slices_gather_want():
    w = get_want()
    refused = list(w["gathered"])
    bad = w["save_value"]
    hit = int(np.nonzero((w["save_where"] >= 0) & (bad[:, 1] > 0))[0][2])
    refused[hit] = bytes([FILL]) * len(refused[hit])
    return {"gathered": w["gathered"], "status": arr([0]), "refused_status": arr([2]), "refused_gathered": refused,
            "guards": bytes([FILL]) * 32}


def _memtable_get(x, s):
    from lsbm_amd import db
    r = db.memtable_get(x["mem"], x["users"][:-1], x["user_offsets"], ho.GET_SNAPSHOT, stream=s)

    def read():
        return {"status": ints(r.status), "values": split(byts(r.values), ints(r.value_offsets)),
                "where": ints(r.where)}
    return read


def _memtable_get_want():
    c, w = get_case(), get_want()
    found = w["mem_verdict"] == gm.FOUND
    return {"status": w["mem_verdict"], "where": np.where(w["mem_where"] >= 0, 0, -1).astype(np.int64),
            "values": [c.bufs["vimage"][o:o + n] if f else b"" for (o, n), f in zip(w["mem_value"].tolist(), found)]}


reg("db.lookup_keys", ["lookup_keys", "lookup_offsets", "lookup_status"], _get_make, _lookup_keys,
    lambda: pick(get_want(), "lookup_keys", "lookup_offsets", "lookup_status"))
reg("db.memtable_probe", ["status", "refused_status"], _get_make, _memtable_probe,
    lambda: dict(pick(get_want(), "mem_verdict", "mem_value", "mem_where"), status=arr([0]), **UNTOUCHED))
reg("db.find_file", ["file", "status"], _get_make, _find_file, lambda: {"file": get_want()["file"], "status": arr([0])})
reg("db.save_value", ["status", "refused_status"], _get_make, _save_value,
    lambda: dict(pick(get_want(), "save_verdict", "save_value", "save_where"), status=arr([0]), **UNTOUCHED))
reg("db.slices_gather", ["status", "refused_status"], _get_make, _slices_gather, _slices_gather_want)
reg("db.memtable_get", ["status", "values", "where"], _get_make, _memtable_get, _memtable_get_want)

# ---------------------------------------------------------------- DB::Get and NewIterator over a version
@cached
def version_case():
    """A memtable, a Level-0 file that overlaps two files of a sorted run; some
    deletions; queries of every user key at a snapshot above and one between
    the sequences."""
    def user(i):
        return b"key%03d" % i

    def table(users, seq, dele=()):
        ents = [(mm.internal_key(user(u), seq, 0 if u in dele else 1), b"" if u in dele else b"f%d:%03d" % (seq, u) * 3)
                for u in users]
        return ents, bd.table_file(ents, bm.INTERNAL_KEY, 256, 4, BITS)[0]
    mem = sm.sort_entries([(mm.internal_key(user(u), 100 + u % 3, int(u % 5 != 0)), b"mem%03d" % u if u % 5 else b"")
                           for u in range(0, 48, 7)])
    tables = [table(range(0, 20), 50), table(range(20, 40), 40, dele=(25, 33)), table(range(10, 30), 90, dele=(12, 21))]
    runs = [([2], gm.RUN_LEVEL0), ([0, 1], 0)]
    queries = [(user(u), s) for u in range(0, 46) for s in (1000, 45)]
    return {"mem": mem, "tables": tables, "runs": runs, "queries": queries}


def _version_make(torch):
    from lsbm_amd import db
    c = version_case()
    files = [db.TableFile(data, 10 + i, BITS, ents[0][0], ents[-1][0]) for i, (ents, data) in enumerate(c["tables"])]
    keys, koff = packed([k for k, _ in c["mem"]])
    image, voff = packed([v for _, v in c["mem"]])
    users, uoff = packed([u for u, _ in c["queries"]])
    return {"version": db.Version(files, [db.Run(idx, flags) for idx, flags in c["runs"]]),
            "mem": db.MemTable(u8(torch, keys), dev(torch, koff), dev(torch, np.stack([voff[:-1], np.diff(voff)], 1)),
                               u8(torch, image)),
            "users": u8(torch, users), "user_offsets": dev(torch, uoff),
            "snapshots": dev(torch, [s for _, s in c["queries"]])}


def _version_get(x, s):
    r = x["version"].get(x["users"], x["user_offsets"], x["snapshots"], [x["mem"]], stream=s)

    def read():
        return {"status": ints(r.status), "values": split(byts(r.values), ints(r.value_offsets)),
                "where": ints(r.where)}
    return read


def _version_get_want():
    c = version_case()
    tables = [gm.open_table(data, BITS, None) for _, data in c["tables"]]
    bounds = [(ents[0][0], ents[-1][0]) for ents, _ in c["tables"]]
    got = [gm.version_get([c["mem"]], tables, bounds, c["runs"], u, s, None) for u, s in c["queries"]]
    assert {v for v, _, _ in got} >= {gm.FOUND, gm.DELETED, gm.UNDECIDED} and {w for _, _, w in got} == {-1, 0, 1, 2}
    return {"status": arr([v for v, _, _ in got]), "values": [val or b"" for _, val, _ in got],
            "where": arr([w for _, _, w in got])}


VIEW_SNAPSHOT = 95


def _version_view(x, s):
    v = x["version"].view(VIEW_SNAPSHOT, [x["mem"]], stream=s)

    def read():
        return {"n": v.n, "n_yield": v.n_yield, "live_keys": split(byts(v.live_keys), ints(v.live_key_offsets)),
                "live_values": cut(byts(v.value_image), ints(v.live_values))}
    return read


def _version_view_want():
    c = version_case()
    merged = sm.sort_entries(list(c["mem"]) + [e for idx, _ in c["runs"] for f in idx for e in c["tables"][f][0]])
    view = sm.View(merged, VIEW_SNAPSHOT)
    return {"n": len(merged), "n_yield": view.n_yield, "live_keys": [merged[j][0] for j in view.live],
            "live_values": [merged[j][1] for j in view.live]}


reg("db.Version.get", ["status", "values", "where"], _version_make, _version_get, _version_get_want)
reg("db.Version.view", ["live_keys", "live_values"], _version_make, _version_view, _version_view_want)


# ---------------------------------------------------------------- range scans
SCAN_SNAPSHOT = ho.SCAN_SNAPSHOTS[0]
SEEK_USERS = [b"", b"a04", b"a0990", b"m", b"n000", b"p", b"zzzz"]


@cached
def scan_case():
    from test_scan_gpu import tile_edge_history
    history = tile_edge_history()
    return ho.scan_case(history), history


@cached
def scan_want():
    c, history = scan_case()
    w = ho.scan_model(c.bufs, c.arrays, SCAN_SNAPSHOT)
    view = sm.View(history, SCAN_SNAPSHOT)
    los, his = split(c.bufs["lo"], c.arrays["lo_offsets"]), split(c.bufs["hi"], c.arrays["hi_offsets"])
    closed = [sm.scan_closed(view, lo if p else None, hi if h else None, int(lim)) for lo, hi, p, h, lim in
              zip(los, his, c.arrays["lo_present"], c.arrays["hi_present"], c.arrays["limits"])]
    first = w["forward_entry_first"]
    w.update(j_begin=arr([j for j, _, _ in closed]), count=arr([n for _, n, _ in closed]),
             key_bytes=np.diff(w["forward_key_offsets"][first]), value_bytes=np.diff(w["forward_value_offsets"][first]),
             # (emit's running sums: user key bytes and value bytes before every query)
             key_first=w["forward_key_offsets"][first])
    assert (w["count"] == np.diff(first)).all() and w["forward_status"].tolist() == [st for _, _, st in closed]
    return w


def _scan_make(torch):
    c, _ = scan_case()
    x = {k: u8(torch, v) for k, v in c.bufs.items()}
    x.update({k: dev(torch, v) for k, v in c.arrays.items()})
    x.update(lo_present=dev(torch, c.arrays["lo_present"], np.uint8),
             hi_present=dev(torch, c.arrays["hi_present"], np.uint8))
    x["seek_keys"], x["seek_offsets"] = (f(torch, v) for f, v in zip((u8, dev), packed(SEEK_USERS)))
    return x


def _view_make(torch):
    from lsbm_amd import scan
    x = _scan_make(torch)
    w = scan_want()
    x["view"] = scan.view(x["keys"], x["key_offsets"], x["values"], x["vimage"], SCAN_SNAPSHOT)
    first = w["forward_entry_first"]
    x.update(j_begin=dev(torch, w["j_begin"]), entry_first=dev(torch, first), key_first=dev(torch, w["key_first"]),
             value_first=dev(torch, w["forward_value_offsets"][first]),
             totals=(int(first[-1]), int(w["key_first"][-1]), int(w["forward_value_offsets"][-1])))
    return x


def _plan_out(p, ny):
    return {"live": ints(p.source)[:ny], "yield_rank": ints(p.yield_rank), "corrupt_rank": ints(p.corrupt_rank),
            "first": ints(p.first)[:ny], "back": ints(p.back)[:ny], "counts": ints(p.counts)}


PLAN_NAMES = ("live", "yield_rank", "corrupt_rank", "first", "back", "counts")


def _scan_plan(x, s):
    from lsbm_amd import scan
    p = scan.plan(x["keys"], x["key_offsets"], SCAN_SNAPSHOT, stream=s)

    def read():
        return dict(_plan_out(p, int(scan_want()["counts"][0])), status=ints(p.status))
    return read


def _scan_view(x, s):
    from lsbm_amd import scan
    v = scan.view(x["keys"], x["key_offsets"], x["values"], x["vimage"], SCAN_SNAPSHOT, stream=s)

    def read():
        return dict(_plan_out(v.plan, v.n_yield), live_values=ints(v.live_values).reshape(-1, 2))
    return read


def _view_range(x, s):
    r = x["view"].range(x["lo"], x["lo_offsets"], x["hi"], x["hi_offsets"], limit=x["limits"],
                        lo_present=x["lo_present"],
                        hi_present=x["hi_present"], stream=s)

    def read():
        count = ints(r.count)
        return {"j_begin": np.where(count > 0, ints(r.j_begin), 0), "count": count, "forward_status": ints(r.status),
                "key_bytes": ints(r.key_bytes), "value_bytes": ints(r.value_bytes), "call_status": ints(r.call_status)}
    return read


def _range_want():
    w = scan_want()
    out = pick(w, "count", "forward_status", "value_bytes")
    out.update(j_begin=np.where(w["count"] > 0, w["j_begin"], 0), key_bytes=w["key_bytes"], call_status=arr([0]))
    return out


def _scan_out(r):
    return {"forward_status": ints(r.status), "forward_entry_first": ints(r.entry_first),
            "forward_keys": byts(r.keys), "forward_key_offsets": ints(r.key_offsets), "forward_values": byts(r.values),
            "forward_value_offsets": ints(r.value_offsets)}


SCAN_NAMES = ("forward_status", "forward_entry_first", "forward_keys", "forward_key_offsets", "forward_values",
              "forward_value_offsets")


def _view_emit(x, s):
    keys, koff, values, voff, status = x["view"].emit(x["j_begin"], x["entry_first"], x["key_first"], x["value_first"],
                                                      totals=x["totals"], stream=s)

    def read():
        return {"forward_keys": byts(keys), "forward_key_offsets": ints(koff), "forward_values": byts(values),
                "forward_value_offsets": ints(voff), "status": ints(status)}
    return read


def _view_scan(x, s):
    r = x["view"].scan(x["lo"], x["lo_offsets"], x["hi"], x["hi_offsets"], limit=x["limits"],
                       lo_present=x["lo_present"], hi_present=x["hi_present"], stream=s)

    def read():
        return _scan_out(r)
    return read


def _entries_out(r):
    return {"entries": list(zip(split(byts(r.keys), ints(r.key_offsets)),
                                split(byts(r.values), ints(r.value_offsets)))),
            "entry_first": ints(r.entry_first), "status": ints(r.status)}


def _view_seek(x, s):
    r = x["view"].seek(x["seek_keys"], x["seek_offsets"], stream=s)

    def read():
        return _entries_out(r)
    return read


def _view_first(x, s):
    r = x["view"].seek_to_first(stream=s)

    def read():
        return _entries_out(r)
    return read


def _view_last(x, s):
    r = x["view"].seek_to_last(stream=s)

    def read():
        return _entries_out(r)
    return read


def _seek_want(queries):
    got = [sm.scan_port(scan_case()[1], SCAN_SNAPSHOT, lo, None, 1, reverse)[:2] for lo, reverse in queries]
    return {"entries": [e for es, _ in got for e in es], "status": arr([st for _, st in got]),
            "entry_first": np.cumsum([0] + [len(es) for es, _ in got]).astype(np.int64)}


reg("scan.plan", PLAN_NAMES + ("status",), _scan_make, _scan_plan,
    lambda: dict(pick(scan_want(), *PLAN_NAMES), status=arr([0])))
reg("scan.view", PLAN_NAMES + ("live_values",), _scan_make, _scan_view,
    lambda: pick(scan_want(), "live_values", *PLAN_NAMES))
reg("scan.SnapshotView.range", ["j_begin", "count", "forward_status", "key_bytes", "value_bytes", "call_status"],
    _view_make, _view_range, _range_want)
reg("scan.SnapshotView.emit", ["forward_keys", "forward_key_offsets", "forward_values", "forward_value_offsets",
                               "status"],
    _view_make, _view_emit, lambda: dict(pick(scan_want(), *SCAN_NAMES[2:]), status=arr([0])))
reg("scan.SnapshotView.scan", SCAN_NAMES, _view_make, _view_scan, lambda: pick(scan_want(), *SCAN_NAMES))
reg("scan.SnapshotView.seek", ["entries", "entry_first", "status"], _view_make,
    _view_seek,
    lambda: _seek_want([(u, False) for u in SEEK_USERS]))
reg("scan.SnapshotView.seek_to_first", ["entries", "entry_first", "status"], _view_make,
    _view_first, lambda: _seek_want([(None, False)]))
reg("scan.SnapshotView.seek_to_last", ["entries", "entry_first", "status"], _view_make,
    _view_last, lambda: _seek_want([(None, True)]))

# ---------------------------------------------------------------- DB::Write
WRITERS = [([(1, b"alpha", b"one"), (0, b"beta", b"")], False), ([], False), ([(1, b"gamma", b"three" * 30)], True),
           ([(1, b"d", b"")], False), ([(1, b"epsilon-key", wc.pattern(3, 300)), (0, b"zeta", b"")], False)]
LAST_SEQUENCE, LOG_OFFSET = 100, 40


@cached
def write_case():
    reps, gf, gs, seqs, counts, last = wm.write(WRITERS, LAST_SEQUENCE)
    assert len(reps) >= 2  # (a sync writer does not join a leader that is not)
    ops = [op for o, _ in WRITERS for op in o]
    op_sum = np.concatenate([[0], np.cumsum([wm.op_bytes(op) for op in ops])]).astype(np.int64)
    batch_sum = np.concatenate([[0], np.cumsum([wm.batch_of(o).byte_size() for o, _ in WRITERS])]).astype(np.int64)
    body, rec_off = packed(reps)
    records = np.stack([rec_off[:-1], np.diff(rec_off)], 1).reshape(-1)
    out = {"reps": reps, "group_first": arr(gf), "group_sync": arr([int(x) for x in gs]), "sequences": arr(seqs),
           "counts": arr(counts), "last": last, "op_sum": op_sum, "batch_sum": batch_sum, "body": body,
           "records": records}
    for name, at, crc_of in (("plain", LOG_OFFSET, None), ("sealed", LOG_OFFSET, masked_crc), ("file", 0, masked_crc)):
        log, heads, frags, end = wm.add_records(reps, at, crc_of)
        firsts = np.concatenate([[0], np.cumsum(frags)]).astype(np.int64)
        out[name] = {"log": log, "heads": arr(heads), "end": end, "frag_first": firsts,
                     "rec_start": arr([at + heads[f] for f in firsts[:-1]] + [end])}
    return out


def _write_make(torch):
    from test_write_gpu import dev_ops
    c = write_case()
    ops, sync = dev_ops(torch, WRITERS)
    p = c["plain"]
    return dict(ops, sync=sync, op_sum=dev(torch, c["op_sum"]), batch_sum=dev(torch, c["batch_sum"]),
                group_first=dev(torch, c["group_first"]), body=u8(torch, c["body"]), records=dev(torch, c["records"]),
                frag_first=dev(torch, p["frag_first"]), rec_start=dev(torch, p["rec_start"]))


def _ops(x):
    return {k: x[k] for k in ("types", "keys", "key_offsets", "value_image", "values", "batch_first")}


def _write_sizes(x, s):
    from lsbm_amd import write
    r = write.sizes(x["types"], x["key_offsets"], x["keys"].numel(), x["values"], x["value_image"].numel(),
                    x["batch_first"], stream=s)

    def read():
        return {"op_sum": ints(r.op_sum), "batch_sum": ints(r.batch_sum), "status": ints(r.status)}
    return read


def _write_group(x, s):
    from lsbm_amd import write
    g = write.group(batch_sum=x["batch_sum"], sync=x["sync"], stream=s)

    def read():
        n = int(g.n_groups.cpu()[0])
        return {"group_first": ints(g.group_first)[:n + 1], "group_sync": ints(g.group_sync)[:n],
                "n_groups": ints(g.n_groups),
                "status": ints(g.status)}
    return read


def _write_build(x, s):
    """Without `reps`: the host read of op_sum's total sizes it."""
    from lsbm_amd import write
    n = len(write_case()["reps"])
    b = write.build(x["types"], x["keys"], x["key_offsets"], x["value_image"], x["values"], x["batch_first"],
                    x["op_sum"],
                    x["group_first"], n, LAST_SEQUENCE, stream=s)

    def read():
        sc = ints(b.seq_counts).reshape(-1, 2)
        return {"body": byts(b.reps), "records": ints(b.records), "sequences": sc[:, 0], "counts": sc[:, 1],
                "last": ints(b.last_sequence), "status": ints(b.status)}
    return read


def _frame_plan(x, s):
    from lsbm_amd import write
    p = write.frame_plan(x["records"], x["body"].numel(), LOG_OFFSET, stream=s)

    def read():
        return {"frag_first": ints(p.frag_first), "rec_start": ints(p.rec_start), "status": ints(p.status)}
    return read


def _frame(x, s):
    from lsbm_amd import write
    f = write.frame(x["body"], x["records"], LOG_OFFSET, x["frag_first"], x["rec_start"], stream=s)

    def read():
        return {"log": byts(f.out), "heads": ints(f.headers), "status": ints(f.status)}
    return read


def _frame_records(x, s):
    from lsbm_amd import write
    f = write.frame_records(x["body"], x["records"], LOG_OFFSET, stream=s)

    def read():
        return {"log": byts(f.log), "heads": ints(f.headers), "end": f.end_offset}
    return read


def _groups_out(r):
    return {"body": byts(r.reps), "records": ints(r.records), "group_first": ints(r.group_first),
            "group_sync": ints(r.group_sync), "sequences": ints(r.sequences), "counts": ints(r.counts),
            "last": r.last_sequence}


GROUP_NAMES = ("body", "records", "group_first", "group_sync", "sequences", "counts", "last")


def _write_batches(x, s):
    from lsbm_amd import write
    r = write.write_batches(sync=x["sync"], last_sequence=LAST_SEQUENCE, log_offset=LOG_OFFSET, stream=s, **_ops(x))

    def read():
        return dict(_groups_out(r), log=byts(r.log), heads=ints(r.headers), end=r.end_offset)
    return read


def _write_logs(x, s):
    from lsbm_amd import write
    r = write.write_logs(sync=x["sync"], last_sequence=LAST_SEQUENCE, stream=s, **_ops(x))

    def read():
        return dict(_groups_out(r), logs=[byts(g.log) for g in r.logs], heads=[ints(g.headers) for g in r.logs],
                    ends=[g.end_offset for g in r.logs], first_log_continues=r.first_log_continues,
                    mem_first=list(r.mem_first), usage=ints(r.usage), mem_state=ints(r.mem_state))
    return read


def _write_logs_want():
    """One memtable takes every group (they are far below the write buffer):
    one log, from offset 0; the accounting is the cut model's in WRITE mode
    over the groups."""
    c = write_case()
    f = c["file"]
    bf = np.concatenate([[0], np.cumsum([len(o) for o, _ in WRITERS])])
    entries = [(len(k) + 8, len(v), t) for o, _ in WRITERS for t, k, v in o]
    cutw = mcm.cut(entries, bf[c["group_first"]].tolist(), None, mcm.WRITE, 4 << 20)
    assert cutw["status"] == mcm.OK and cutw["mem_first"] == [0, len(c["reps"])]
    return dict(pick(c, *GROUP_NAMES), logs=[f["log"]], heads=[f["heads"]], ends=[f["end"]], first_log_continues=True,
                mem_first=cutw["mem_first"], usage=arr(cutw["usage"]), mem_state=arr(cutw["state"]))


reg("write.sizes", ["op_sum", "batch_sum", "status"], _write_make, _write_sizes,
    lambda: dict(pick(write_case(), "op_sum", "batch_sum"), status=arr([0])))
reg("write.group", ["group_first", "group_sync", "n_groups", "status"], _write_make, _write_group,
    lambda: dict(pick(write_case(), "group_first", "group_sync"), n_groups=arr([len(write_case()["reps"])]),
                 status=arr([0])))
reg("write.build", ["body", "records", "sequences", "counts", "last", "status"], _write_make, _write_build,
    lambda: dict(pick(write_case(), "body", "records", "sequences", "counts"), last=arr([write_case()["last"]]),
                 status=arr([0])))
reg("write.frame_plan", ["frag_first", "rec_start", "status"], _write_make, _frame_plan,
    lambda: dict(pick(write_case()["plain"], "frag_first", "rec_start"), status=arr([0])))
reg("write.frame", ["log", "heads", "status"], _write_make, _frame,
    lambda: dict(pick(write_case()["plain"], "log", "heads"), status=arr([0])))
reg("write.frame_records", ["log", "heads"], _write_make, _frame_records,
    lambda: pick(write_case()["sealed"], "log", "heads", "end"))
reg("write.write_batches", GROUP_NAMES + ("log", "heads"), _write_make, _write_batches,
    lambda: dict(pick(write_case(), *GROUP_NAMES), **pick(write_case()["sealed"], "log", "heads", "end")))
reg("write.write_logs", GROUP_NAMES + ("logs", "heads", "usage", "mem_state"), _write_make, _write_logs,
    _write_logs_want)


# ---------------------------------------------------------------- VersionEdit and the MANIFEST
M64 = (1 << 64) - 1


@cached
def decode_case():
    """Records of manifest_cases.records(): every field, repeated tags, files,
    an unknown tag (a verdict that is not 0), laid out back to back."""
    named = dict(mfc.records())
    recs = [named[n] for n in ("all_tags", "empty", "repeated_files", "unknown_tag_5", "numbers_2_63", "chain_65")]
    image, at = b"", []
    for r in recs:
        at.append((len(image), len(r)))
        image += r
    decoded = [mfm.decode(r) for r in recs]
    assert {code for code, _ in decoded} > {0}
    n_new = [len(e["new"]) if not code else 0 for code, e in decoded]
    n_del = [len(e["deleted"]) if not code else 0 for code, e in decoded]
    return {"recs": recs, "image": image, "at": at, "decoded": decoded,
            "new_first": np.concatenate([[0], np.cumsum(n_new)]), "del_first": np.concatenate([[0], np.cumsum(n_del)]),
            "key_bytes": sum(len(f[4]) + len(f[5]) for code, e in decoded if not code for f in e["new"])}


def _decode_make(torch):
    c = decode_case()
    return {"image": u8(torch, c["image"]), "records": dev(torch, arr(c["at"]))}


def _decode_plan(x, s):
    from lsbm_amd import manifest
    c = decode_case()
    p = manifest.decode_plan(x["image"], x["records"], len(c["image"]), max(len(r) for r in c["recs"]), stream=s)

    def read():
        return {"verdict": ints(p.verdict), "new_first": ints(p.new_first), "del_first": ints(p.del_first),
                "totals": ints(p.totals), "status": ints(p.status), "has": ints(p.fields)[:, 0]}
    return read


def _decode_plan_want():
    c = decode_case()
    has = []
    for code, e in c["decoded"]:
        bits = [e["comparator"], e["log_number"], e["prev_log_number"], e["next_file"], e["last_sequence"],
                e["write_cursor"]]
        has.append(0 if code else sum(1 << i for i, v in enumerate(bits) if v is not None))
    return {"verdict": arr([code for code, _ in c["decoded"]]), "new_first": c["new_first"],
            "del_first": c["del_first"],
            "totals": arr([c["new_first"][-1], c["del_first"][-1], c["key_bytes"]]), "status": arr([0]),
            "has": arr(has)}


def _decode_emit_make(torch):
    from lsbm_amd import manifest
    x = _decode_make(torch)
    c = decode_case()
    x["plan"] = manifest.decode_plan(x["image"], x["records"], len(c["image"]), max(len(r) for r in c["recs"]))
    return x


def _items_out(new_items, key_offsets, keys, del_items):
    """The items as the model holds them: per new file (record, type, level,
    number, size, smallest, largest), per deleted file (record, type, level, number)."""
    k = split(keys, key_offsets)
    return {"new": [tuple(row[:3]) + (row[3] & M64, row[4] & M64, k[2 * j], k[2 * j + 1])
                    for j, row in enumerate(new_items.tolist())],
            "deleted": [tuple(row[:3]) + (row[3] & M64,) for row in del_items.tolist()]}


def _decode_emit(x, s):
    from lsbm_amd import manifest
    c = decode_case()
    e = manifest.decode_emit(x["image"], x["records"], x["plan"], int(c["new_first"][-1]), int(c["del_first"][-1]),
                             c["key_bytes"], stream=s)

    def read():
        return dict(_items_out(ints(e.new_items), ints(e.key_offsets), byts(e.keys), ints(e.del_items)),
                    status=ints(e.status))
    return read


def _items_want():
    new, dele = [], []
    for r, (code, e) in enumerate(decode_case()["decoded"]):
        if not code:
            new += [(r,) + tuple(f) for f in e["new"]]
            dele += [(r,) + tuple(d) for d in e["deleted"]]
    return {"new": new, "deleted": dele}


def _decode_edits(x, s):
    from lsbm_amd import manifest
    from test_manifest_gpu import host_edits
    e = manifest.decode_edits(x["image"], x["records"], stream=s)

    def read():
        return {"edits": host_edits(e, decode_case()["image"])}
    return read


reg("manifest.decode_plan", ["verdict", "new_first", "del_first", "totals", "status", "has"], _decode_make,
    _decode_plan,
    _decode_plan_want)
reg("manifest.decode_emit", ["new", "deleted", "status"], _decode_emit_make, _decode_emit,
    lambda: dict(_items_want(), status=arr([0])))
reg("manifest.decode_edits", ["edits"], _decode_make, _decode_edits,
    lambda: {"edits": [(code, e) for code, e in decode_case()["decoded"]]})


@cached
def encode_case():
    edits = [e for name, e in mfc.edits() if name in ("nothing", "all_fields", "files", "items_63", "key_9",
                                                      "random_3")]
    assert len(edits) == 6
    return edits, [mfm.encode(e) for e in edits]


def _encode_make(torch):
    from lsbm_amd import manifest
    from test_manifest_gpu import device_edits
    d = device_edits(torch, encode_case()[0], sort=False)  # (encode_edits sorts the deleted files itself)
    d["sorted_first"], d["sorted_items"] = manifest.sort_deleted(d["del_items"], len(encode_case()[0]))
    total = sum(len(r) for r in encode_case()[1])
    d.update(out=filled(torch, 8 + total + 8), short_out=filled(torch, 8 + total + 8), total=total)
    return d


def _encode_args(d):
    return (d["fields"], d["names"], d["sorted_first"], d["sorted_items"], d["new_first"], d["new_items"], d["keys"],
            d["key_offsets"])


def _encode_plan(x, s):
    from lsbm_amd import manifest
    p = manifest.encode_plan(*_encode_args(x), 8, stream=s)

    def read():
        return {"records": ints(p.records), "totals": ints(p.totals), "status": ints(p.status)}
    return read


def _encode_plan_want():
    lens = [len(r) for r in encode_case()[1]]
    at = 8 + np.concatenate([[0], np.cumsum(lens)])[:-1]
    return {"records": np.stack([at, lens], 1).astype(np.int64), "totals": arr([sum(lens)]), "status": arr([0])}


def _encode_emit_make(torch):
    from lsbm_amd import manifest
    x = _encode_make(torch)
    x["plan"] = manifest.encode_plan(*_encode_args(x), 8)
    return x


def _encode_emit(x, s):
    from lsbm_amd import manifest
    status = manifest.encode_emit(*_encode_args(x), x["plan"], x["out"], 8, x["total"], stream=s)
    refused = manifest.encode_emit(*_encode_args(x), x["plan"], x["short_out"], 8, x["total"] - 1, stream=s)

    def read():
        return {"out": byts(x["out"]), "status": ints(status), "refused_out": byts(x["short_out"]),
                "refused_status": ints(refused)}
    return read


def _encode_emit_want():
    body = b"".join(encode_case()[1])
    return {"out": bytes([FILL]) * 8 + body + bytes([FILL]) * 8, "status": arr([0]),
            "refused_out": bytes([FILL]) * (16 + len(body)), "refused_status": arr([1])}


def _encode_edits(x, s):
    from lsbm_amd import manifest
    r = manifest.encode_edits(x["fields"], x["names"], x["del_items"], x["new_first"], x["new_items"], x["keys"],
                              x["key_offsets"], stream=s)

    def read():
        return {"records": cut(byts(r.image), ints(r.records))}
    return read


reg("manifest.encode_plan", ["records", "totals", "status"], _encode_make, _encode_plan, _encode_plan_want)
reg("manifest.encode_emit", ["status", "refused_status"], _encode_emit_make, _encode_emit, _encode_emit_want)
reg("manifest.encode_edits", ["records"], _encode_make, _encode_edits, lambda: {"records": encode_case()[1]})

SNAPSHOT_NUMBERS = dict(log_number=12, prev_log_number=0, next_file=5000, last_sequence=1 << 50, write_cursor=M64,
                        read_cursors=(1, 0, 1 << 63, 3))


@cached
def snapshot_files():
    rnd = random.Random(8)
    files = mfc.snapshot_files(70, 3)
    rnd.shuffle(files)
    return [(rnd.randrange(4),) + f[1:] for f in files]


def _snapshot_make(torch):
    from test_manifest_gpu import file_table
    return {"files": file_table(torch, snapshot_files())}


def _snapshot(x, s):
    from lsbm_amd import manifest
    r = manifest.snapshot(x["files"], stream=s, **SNAPSHOT_NUMBERS)

    def read():
        return {"image": byts(r.image), "records": ints(r.records)}
    return read


def _snapshot_want():
    image = mfm.encode(mfm.snapshot_edit(snapshot_files(), **SNAPSHOT_NUMBERS))
    return {"image": image, "records": arr([[0, len(image)]])}


reg("manifest.snapshot", ["image", "records"], _snapshot_make, _snapshot, _snapshot_want)


@cached
def manifest_case():
    """The `history` MANIFEST of manifest_cases.manifests(): twelve edits that
    add, delete and add files again, framed as log::Writer frames them."""
    from test_manifest import manifest_file, model_recover
    payloads = dict((name, p) for name, p, how in mfc.manifests() if how is None)["history"]
    image = manifest_file(crc(), payloads)
    return image, model_recover(crc(), image)


def _manifest_recover(x, s):
    from lsbm_amd import manifest
    r = manifest.recover(x["image"], stream=s)

    def read():
        return {"status": r.status, "log_number": r.log_number, "prev_log_number": r.prev_log_number,
                "next_file_number": r.next_file_number, "manifest_file_number": r.manifest_file_number,
                "last_sequence": r.last_sequence, "files": r.files}
    return read


reg("manifest.recover", ["status", "files", "last_sequence"], lambda torch: {"image": u8(torch, manifest_case()[0])},
    _manifest_recover, lambda: dict(manifest_case()[1]))


# ---------------------------------------------------------------- LSbM's buffered Get
PLAN_QUERIES, PLAN_SLOTS = 65, 64


@cached
def plan_case():
    from test_buffered_gpu import plan_model, random_plan_values
    values = random_plan_values(random.Random(77), PLAN_QUERIES, PLAN_SLOTS)
    probes = plan_model(*values)
    assert sum(len(p) for p in probes) > 100
    return values, probes


def _plan_make(torch):
    from test_buffered_gpu import PlanInput
    x = PlanInput(torch, *plan_case()[0])
    counts = [len(p) for p in plan_case()[1]]
    total = sum(counts)
    return {"inputs": x.inputs(), "first": dev(torch, np.concatenate([[0], np.cumsum(counts)])), "total": total,
            "slots": filled(torch, total + 8, torch.int32, -7),
            "short_slots": filled(torch, total + 8, torch.int32, -7)}


def _probe_plan(x, s):
    from lsbm_amd import buffered
    count, status = buffered.probe_plan(*x["inputs"], stream=s)

    def read():
        return {"count": ints(count), "status": ints(status)}
    return read


def _probe_emit(x, s):
    from lsbm_amd import buffered
    status = buffered.probe_emit(*x["inputs"], x["first"], x["slots"], x["total"], stream=s)
    refused = buffered.probe_emit(*x["inputs"], x["first"], x["short_slots"], x["total"] - 1, stream=s)

    def read():
        return {"slots": ints(x["slots"]), "status": ints(status), "refused_slots": ints(x["short_slots"]),
                "refused_status": ints(refused)}
    return read


def _probe_emit_want():
    flat = [s for p in plan_case()[1] for s in p]
    return {"slots": arr(flat + [-7] * 8), "status": arr([0]), "refused_slots": arr([-7] * (len(flat) + 8)),
            "refused_status": arr([1])}


reg("buffered.probe_plan", ["count", "status"], _plan_make, _probe_plan,
    lambda: {"count": arr([len(p) for p in plan_case()[1]]), "status": arr([0])})
reg("buffered.probe_emit", ["status", "refused_status"], _plan_make, _probe_emit, _probe_emit_want)


@cached
def buffered_case():
    """The fixture's `lists` case and its first run: the model's version, the
    opened tables, the run's parameters and queries."""
    _, body = bc.load_fixture()
    case = body["cases"]["lists"]
    files = bc.case_files(body, case)
    v, tables = bc.case_version(case, files)
    run = case["runs"][0]
    bc.set_visible(v, run)
    return {"case": case, "files": files, "v": v, "tables": tables, "p": bc.run_params(run),
            "queries": [(bytes.fromhex(k), s) for k, s in run["queries"]], "results": run["results"]}


def _buffered_make(torch):
    from lsbm_amd import buffered
    from test_buffered_gpu import visible_of
    c = buffered_case()
    image = u8(torch, bytes.fromhex(c["case"]["manifest"]))
    bv = buffered.BufferedVersion.from_manifest(image, c["files"], c["case"]["compaction_buffer_length"],
                                                bits_per_key=bc.BITS)
    bv.configure(c["p"].use_length, c["p"].buffered_merge, c["p"].read_cursor_keys)
    bv.visible.copy_(dev(torch, visible_of(bv, c["v"].lists()), np.uint8))
    users, uoff = packed([u for u, _ in c["queries"]])
    return {"bv": bv, "users": u8(torch, users), "user_offsets": dev(torch, uoff),
            "snapshots": dev(torch, [s for _, s in c["queries"]])}


def _buffered_get(x, s):
    from lsbm_amd import db
    r = x["bv"].get(x["users"], x["user_offsets"], x["snapshots"], stream=s)

    def read():
        status = ints(r.status).tolist()
        return {"status": [db.status_string(st, u) for st, (u, _) in zip(status, buffered_case()["queries"])],
                "values": split(byts(r.values), ints(r.value_offsets)), "where": ints(r.where)}
    return read


def _buffered_get_want():
    c = buffered_case()
    layout, memo = bfm.slots(c["v"], c["p"]), {}
    got = [bfm.rule_get(c["v"], c["tables"], c["p"], u, s, layout=layout, memo=memo) for u, s in c["queries"]]
    status = [gm.status_string(g[0], u) for g, (u, _) in zip(got, c["queries"])]
    assert status == [st for st, _ in c["results"]]  # (the reference's own answers)
    return {"status": status, "values": [g[1] or b"" for g in got], "where": arr([g[3] for g in got])}


reg("buffered.BufferedVersion.get", ["status", "values", "where"], _buffered_make, _buffered_get, _buffered_get_want)
