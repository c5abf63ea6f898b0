"""Fixture of the reference's own TableBuilder / BlockBuilder / comparator
results for the GPU block builder (include/lsbm_block_build.h).

    python tests/golden/make_build_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(everything but db_bench's main), runs it, and writes
tests/golden/build_fixture.json and build_tables.bin:

  * table files written by the reference's TableBuilder through a string sink
    (kNoCompression): block sizes 256 / 1024 / 4096 x restart intervals
    1 / 3 / 16 under the bytewise comparator; empty keys and values, keys
    > 127 B and > 16383 B and a 16 KiB value; entries that land
    CurrentSizeEstimate() exactly on block_size and one byte below it;
    internal keys with a 10-bit bloom filter; a one-entry and an empty table.
    A table's entries, cuts, block sizes, data blocks, filter, metaindex and
    index blocks are all read back from its bytes (tests/test_block_build.py);
  * FindShortestSeparator / FindShortSuccessor of both comparators on crafted
    and random pairs.

Only bytes produced by the reference are stored; no reference source.
"""
import glob
import json
import os
import random
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from golden import buildmodel as bd  # noqa: E402

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

DRIVER = r"""
// Driver for tests/golden/make_build_fixture.py: runs the reference's
// TableBuilder into a string, and its comparators' FindShortestSeparator /
// FindShortSuccessor, over a command file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/filter_policy.h"
#include "leveldb/options.h"
#include "leveldb/table_builder.h"
#include "dbformat.h"
using namespace leveldb;

static FILE *in, *out;
static uint32_t r32() { uint32_t v; if (fread(&v, 4, 1, in) != 1) exit(3); return v; }
static std::string rstr() { uint32_t n = r32(); std::string s(n, '\0'); if (n && fread(&s[0], 1, n, in) != n) exit(3); return s; }
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void wstr(const std::string& s) { w32(s.size()); fwrite(s.data(), 1, s.size(), out); }

class StringSink : public WritableFile {
 public:
  std::string contents;
  virtual Status Append(const Slice& d) { contents.append(d.data(), d.size()); return Status::OK(); }
  virtual Status Close() { return Status::OK(); }
  virtual Status Flush() { return Status::OK(); }
  virtual Status Sync() { return Status::OK(); }
};

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const Comparator* bytewise = BytewiseComparator();
  InternalKeyComparator internal(bytewise);
  int c;
  while ((c = fgetc(in)) != EOF) {
    const uint32_t cmpi = r32();
    const Comparator* cmp = cmpi ? static_cast<const Comparator*>(&internal) : bytewise;
    if (c == 'T') {  // block_size, restart interval, bits per key (0: no filter), n, (key, value)*
      Options o;
      o.comparator = cmp;
      o.block_size = r32();
      o.block_restart_interval = (int)r32();
      o.compression = kNoCompression;
      const uint32_t bits = r32();
      const FilterPolicy* user = bits ? NewBloomFilterPolicy((int)bits) : NULL;
      InternalFilterPolicy wrapped(user);
      o.filter_policy = user ? (cmpi ? static_cast<const FilterPolicy*>(&wrapped) : user) : NULL;
      StringSink sink;
      {
        TableBuilder b(o, &sink);
        const uint32_t n = r32();
        for (uint32_t i = 0; i < n; i++) {
          std::string k = rstr(), v = rstr();
          b.Add(k, v);
        }
        if (!b.Finish().ok() || b.FileSize() != sink.contents.size()) exit(4);
      }
      wstr(sink.contents);
      delete user;
    } else if (c == 'P') {
      std::string start = rstr(), limit = rstr();
      cmp->FindShortestSeparator(&start, limit);
      wstr(start);
    } else if (c == 'U') {
      std::string key = rstr();
      cmp->FindShortSuccessor(&key);
      wstr(key);
    } else {
      exit(5);
    }
  }
  fclose(out);
  return 0;
}
"""


def build_driver(tmp):
    if not os.path.isdir(OBJ):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "dbbench"], check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*", "*.o"))) if not o.endswith("lsbm/db_bench.o")]
    src = os.path.join(tmp, "build_driver.cc")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "build_driver")
    subprocess.run(["g++", "-std=c++11", "-w", "-O2", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX",
                    "-I" + REF, "-I" + REF + "/include", "-I" + REF + "/common", "-o", exe, src] + objs, check=True)
    return exe


def p32(v):
    return struct.pack("<I", v)


def pstr(b):
    return p32(len(b)) + bytes(b)


def internal_key(user, seq, typ=1):
    return user + struct.pack("<Q", (seq << 8) | typ)


def table_specs():
    """(name, cmp, block_size, restart interval, bits per key or None, [(key, value)])."""
    rng = random.Random(0xB01D)
    specs = []

    def rand_keys(n, lo, hi, alphabet=b"abcdefgh"):
        ks = set()
        while len(ks) < n:
            ks.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))))
        return sorted(ks)

    def vals(n, lo, hi):
        return [bytes(rng.randrange(256) for _ in range(rng.randint(lo, hi))) for _ in range(n)]

    for bs in (256, 1024, 4096):
        for ri in (1, 3, 16):
            n = 60 if bs == 256 else 140
            k = rand_keys(n, 3, 22)
            specs.append((f"bytewise_bs{bs}_ri{ri}", 0, bs, ri, None, list(zip(k, vals(n, 0, 60)))))
    # empty keys and values, multi-byte varints in all three header fields, a one-entry block
    pre = bytes(rng.choice(b"xyz") for _ in range(140))
    long_keys = sorted({pre + bytes(rng.choice(b"0123456789") for _ in range(rng.randint(1, 120)))
                        for _ in range(8)})
    e = [(b"", b""), (b"a", b""), (b"ab", b"x"), (b"b", b"")]
    e += list(zip(long_keys, vals(len(long_keys), 0, 300)))
    e.append((pre + b"~" * 16400, b"v"))
    e.append((pre + b"~" * 16400 + b"a", bytes(rng.randrange(256) for _ in range(16384))))
    e.append((pre + b"~" * 16400 + b"b", b"after"))
    e.append((b"zz", b""))
    specs.append(("edges_bs4096_ri16", 0, 4096, 16, None, e))
    # CurrentSizeEstimate() exactly block_size (flush) and one byte below (no flush)
    e = [(b"ea", b"A" * 242), (b"eb", b"B" * 241), (b"ec", b"C"), (b"ed", b"D" * 242), (b"ee", b"E" * 100)]
    for (k, v), want in zip(e, (256, 255, None, 256, None)):
        if want is not None:  # the first entry of a block: shared = 0, one restart point
            assert 1 + 1 + bd.varint_len(len(v)) + len(k) + len(v) + 4 + 4 == want
    specs.append(("exact_bs256_ri16", 0, 256, 16, None, e))
    # internal keys, with equal user keys under different tags, and a bloom filter
    users = rand_keys(280, 6, 18)
    e = []
    for u in users:
        seqs = sorted({rng.randrange(1, 1 << 40) for _ in range(3 if rng.random() < 0.08 else 1)}, reverse=True)
        e += [internal_key(u, s, rng.choice((0, 1))) for s in seqs]
    specs.append(("internal_bloom10_bs1024_ri16", 1, 1024, 16, 10, list(zip(e, vals(len(e), 8, 48)))))
    k = rand_keys(100, 2, 14, b"abc\xff")
    specs.append(("bytewise_nofilter_bs256_ri3", 0, 256, 3, None, list(zip(k, vals(100, 0, 30)))))
    specs.append(("one_entry_internal_bloom10", 1, 4096, 16, 10, [(internal_key(b"only", 7), b"value")]))
    specs.append(("one_entry_bytewise", 0, 4096, 16, None, [(b"only", b"value")]))
    specs.append(("empty_internal_bloom10", 1, 4096, 16, 10, []))
    specs.append(("empty_bytewise", 0, 4096, 16, None, []))
    return specs


def pair_specs():
    """([(cmp, start, limit)], [(cmp, key)])."""
    rng = random.Random(0x5E9A)
    tag = lambda s, t=1: struct.pack("<Q", (s << 8) | t)  # noqa: E731
    user_pairs = [
        (b"abc", b"abcdef"), (b"abcdef", b"abc"),            # one a prefix of the other
        (b"abc1x", b"abc2y"), (b"abc1x", b"abc3y"),          # x, x+1 and x, x+2
        (b"ab\xffz", b"ac"), (b"ab\xfe\x01", b"ab\xff\x01"), (b"a\xfdzz", b"a\xffzz"),  # 0xff at the difference
        (b"\xff\xff\xff", b"\xff\xff\xff\xff"), (b"\xff\xff", b"\xff\xff"),
        (b"same", b"same"), (b"", b""), (b"", b"a"), (b"a", b""), (b"a", b"c"), (b"ax", b"c"),
        (b"the quick brown fox", b"the who"), (b"\x00", b"\x02"), (b"\x00\x00", b"\x02"),
    ]
    alphabet = b"ab\x00\x01\xfe\xff"
    for _ in range(200):
        n = rng.randint(0, 5)
        pre = bytes(rng.choice(alphabet) for _ in range(n))
        a = pre + bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 4)))
        b = pre + bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 4)))
        user_pairs.append((min(a, b), max(a, b)))
    seps, sucs = [], []
    for a, b in user_pairs:
        seps.append((0, a, b))
        seps.append((1, a + tag(rng.randrange(1 << 40)), b + tag(rng.randrange(1 << 40))))
    seps.append((1, b"user" + tag(9), b"user" + tag(5)))       # equal user keys, different tags
    seps.append((1, b"user" + tag(9, 1), b"user" + tag(9, 0)))
    seps.append((1, tag(9), tag(5)))                           # an empty user key
    seps.append((1, tag(9), b"b" + tag(5)))
    for k in sorted({p[0] for p in user_pairs} | {p[1] for p in user_pairs}):
        sucs.append((0, k))
        sucs.append((1, k + tag(rng.randrange(1 << 40))))
    return seps, sucs


def main():
    tmp = tempfile.mkdtemp(prefix="lsbm_buildfx_")
    exe = build_driver(tmp)
    tables, (seps, sucs) = table_specs(), pair_specs()
    cmds = []
    for _, cmp, bs, ri, bits, entries in tables:
        cmds.append(b"T" + p32(cmp) + p32(bs) + p32(ri) + p32(bits or 0) + p32(len(entries))
                    + b"".join(pstr(k) + pstr(v) for k, v in entries))
    cmds += [b"P" + p32(c) + pstr(a) + pstr(b) for c, a, b in seps]
    cmds += [b"U" + p32(c) + pstr(k) for c, k in sucs]
    fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(fi, "wb").write(b"".join(cmds))
    subprocess.run([exe, fi, fo], check=True)
    buf, p = open(fo, "rb").read(), 0

    def s():
        nonlocal p
        n = struct.unpack_from("<I", buf, p)[0]
        p += 4 + n
        return buf[p - n:p]

    blob, recs = bytearray(), []
    for name, cmp, bs, ri, bits, entries in tables:
        f = s()
        recs.append({"name": name, "cmp": cmp, "block_size": bs, "restart_interval": ri, "bits_per_key": bits,
                     "n_entries": len(entries), "offset": len(blob), "size": len(f)})
        blob += f
    fx = {"source": "lsbm's TableBuilder (kNoCompression) and comparators, built from the reference's objects "
                    "(oracle/Makefile dbbench)",
          "tables": recs,
          "separators": [{"cmp": c, "start": a.hex(), "limit": b.hex(), "out": s().hex()} for c, a, b in seps],
          "successors": [{"cmp": c, "key": k.hex(), "out": s().hex()} for c, k in sucs]}
    assert p == len(buf)
    open(os.path.join(HERE, "build_tables.bin"), "wb").write(blob)
    json.dump(fx, open(os.path.join(HERE, "build_fixture.json"), "w"), indent=0)
    print(f"{len(recs)} tables ({len(blob)} B), {len(seps)} separators, {len(sucs)} successors")


if __name__ == "__main__":
    sys.exit(main())
