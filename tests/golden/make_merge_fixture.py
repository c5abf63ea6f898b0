"""Fixture of the reference's own MergingIterator results for the GPU
compaction merge (include/lsbm_merge.h).

    python tests/golden/make_merge_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(everything but db_bench's main), runs it, and writes
tests/golden/merge_fixture.json and merge_tables.bin.  For every case, under
the bytewise and under the internal-key comparator, the driver

  * writes each run with the reference's TableBuilder through a string sink
    (kNoCompression),
  * reopens it with the reference's Table::Open over a string source,
  * merges the tables' iterators with NewMergingIterator under the case's
    comparator and records key() / value() from SeekToFirst until !Valid().

merge_tables.bin holds the runs' table files and the merged records (u32
length + bytes for each key and each value); the runs' entries are read back
from the table files (tests/test_merge.py).  A value names its entry (run and
position), so the merged records say which input entry came out where.

Cases: 1 / 2 / 3 / 8 / 64 runs; empty runs first, in the middle and last; all
runs empty; identical runs; equal neighbours inside a run; disjoint runs in
ascending and in descending run order; a perfect interleave; a key that is a
prefix of the next; the empty user key; keys > 127 bytes that differ only in
the last byte and only in byte 8k-1 / 8k / 8k+1; internal keys with several
tags per user key spread over different runs.

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

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

DRIVER = r"""
// Driver for tests/golden/make_merge_fixture.py: writes runs with the
// reference's TableBuilder, reopens them with its Table::Open and merges them
// with its NewMergingIterator, over a command file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "leveldb/table.h"
#include "leveldb/table_builder.h"
#include "dbformat.h"
#include "table/merger.h"
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

class StringSource : public RandomAccessFile {
 public:
  explicit StringSource(const std::string& c) : contents_(c) {}
  virtual Status Read(uint64_t offset, size_t n, Slice* result, char* scratch) const {
    if (offset > contents_.size()) return Status::InvalidArgument("invalid Read offset");
    if (offset + n > contents_.size()) n = contents_.size() - offset;
    memcpy(scratch, &contents_[offset], n);
    *result = Slice(scratch, n);
    return Status::OK();
  }
 private:
  std::string contents_;
};

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const Comparator* bytewise = BytewiseComparator();
  InternalKeyComparator internal(bytewise);
  int c;
  while ((c = fgetc(in)) != EOF) {
    if (c != 'M') exit(5);  // cmp, block_size, restart interval, n_runs, per run: n, (key, value)*
    const uint32_t cmpi = r32();
    const Comparator* cmp = cmpi ? static_cast<const Comparator*>(&internal) : bytewise;
    Options o;
    o.comparator = cmp;
    o.block_size = r32();
    o.block_restart_interval = (int)r32();
    o.compression = kNoCompression;
    const uint32_t n_runs = r32();
    std::vector<StringSource*> files;
    std::vector<Table*> tables;
    std::vector<Iterator*> iters;
    w32(n_runs);
    for (uint32_t r = 0; r < n_runs; r++) {
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
      files.push_back(new StringSource(sink.contents));
      Table* t = NULL;
      if (!Table::Open(o, r + 1, files.back(), sink.contents.size(), &t).ok()) exit(6);
      tables.push_back(t);
      ReadOptions ro;
      ro.verify_checksums = true;
      ro.fill_cache = false;
      iters.push_back(t->NewIterator(ro));
    }
    Iterator* m = NewMergingIterator(cmp, iters.empty() ? NULL : &iters[0], (int)n_runs);
    std::vector<std::string> ks, vs;
    for (m->SeekToFirst(); m->Valid(); m->Next()) {
      ks.push_back(m->key().ToString());
      vs.push_back(m->value().ToString());
    }
    if (!m->status().ok()) exit(7);
    w32(ks.size());
    for (size_t i = 0; i < ks.size(); i++) {
      wstr(ks[i]);
      wstr(vs[i]);
    }
    delete m;  // (owns the children)
    for (size_t i = 0; i < tables.size(); i++) delete tables[i];
    for (size_t i = 0; i < files.size(); i++) delete files[i];
  }
  fclose(out);
  return 0;
}
"""


def build_driver(tmp):
    if not os.path.isdir(OBJ):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "dbbench"], check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*", "*.o"))) if not o.endswith("lsbm/db_bench.o")]
    src = os.path.join(tmp, "merge_driver.cc")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "merge_driver")
    subprocess.run(["g++", "-std=c++11", "-w", "-O2", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX",
                    "-I" + REF, "-I" + REF + "/include", "-I" + REF + "/common", "-o", exe, src] + objs, check=True)
    return exe


def p32(v):
    return struct.pack("<I", v)


def pstr(b):
    return p32(len(b)) + bytes(b)


def case_specs():
    """[(name, [run])], a run a list of (user key, seq, type) sorted by user key
    ascending, then seq descending: sorted under both comparators (under the
    bytewise one the key is the user key alone, and versions are equal
    neighbours)."""
    rng = random.Random(0x3E26E)

    def users(n, lo=3, hi=12, alphabet=b"abcd"):
        ks = set()
        while len(ks) < n:
            ks.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))))
        return sorted(ks)

    def run(us, seq_hi=1 << 30):
        return sorted(((u, rng.randrange(1, seq_hi), rng.choice((0, 1, 1))) for u in us), key=lambda e: (e[0], -e[1]))

    def sample(pool, n):
        return sorted(rng.sample(pool, n))

    pool = users(60)
    cases = [("one_run", [run(sample(pool, 20))]),
             ("two_runs", [run(sample(pool, 25)), run(sample(pool, 18))]),
             ("three_runs", [run(sample(pool, 20)), run(sample(pool, 9)), run(sample(pool, 14))]),
             ("eight_runs", [run(sample(pool, rng.randint(3, 12))) for _ in range(8)]),
             ("sixty_four_runs", [run(sample(pool, rng.randint(0, 4))) for _ in range(64)]),
             ("empty_first_middle_last", [[], run(sample(pool, 7)), [], [], run(sample(pool, 9)), []]),
             ("all_empty", [[], [], []]),
             ("no_runs", [])]
    same = run(sample(pool, 10))
    cases.append(("identical_runs", [list(same) for _ in range(5)]))
    # equal neighbours inside a run: the same internal key twice, and versions of one user key
    dup = run(sample(pool, 8))
    dup = sorted(dup + [dup[2], dup[2], dup[5]] + [(dup[6][0], dup[6][1] + 7, 1)], key=lambda e: (e[0], -e[1]))
    cases.append(("equal_neighbours", [dup, run(sample(pool, 6)), list(dup)]))
    lo, mid, hi = pool[:15], pool[15:30], pool[30:45]
    cases.append(("disjoint_ascending", [run(lo), run(mid), run(hi)]))
    cases.append(("disjoint_descending", [run(hi), run(mid), run(lo)]))
    cases.append(("interleave", [run(pool[r::4]) for r in range(4)]))
    pre = [b"a", b"ab", b"abc", b"abcd", b"abcd\x00", b"abcd\x00\x00", b"abcd\xff"]
    cases.append(("prefix_of_next", [run(pre[0::2]), run(pre[1::2]), run(pre)]))
    cases.append(("empty_user_key", [run([b"", b"a"]), run([b""]), run([b"", b"\x00"])]))
    # keys > 127 bytes that differ only in the last byte, and only in byte 8k-1 / 8k / 8k+1
    base = bytes(rng.choice(b"xyz") for _ in range(137))
    long_keys = {base[:-1] + bytes([b]) for b in (0x01, 0x7f, 0x80, 0xfe)}
    for k in (1, 8, 16):
        for at in (8 * k - 1, 8 * k, 8 * k + 1):
            for b in (0x00, 0x80, 0xff):
                long_keys.add(base[:at] + bytes([b]) + base[at + 1:])
    long_keys = sorted(long_keys)
    rng.shuffle(long_keys)
    cases.append(("long_keys_one_byte", [run(long_keys[r::3]) for r in range(3)]))
    # several tags per user key, spread over different runs; seqs collide across
    # runs too (the type byte and then the run number break the tie)
    hot = sample(pool, 6)
    runs = [[] for _ in range(5)]
    for u in hot:
        for seq in rng.sample(range(1, 40), 9):
            runs[rng.randrange(5)].append((u, seq, rng.choice((0, 1))))
        runs[0].append((u, 41, 1))
        runs[3].append((u, 41, 1))
        runs[4].append((u, 41, 0))
    cases.append(("versions_across_runs", [sorted(r, key=lambda e: (e[0], -e[1], -e[2])) for r in runs]))
    return cases


def entries_of(case_runs, cmp):
    """[[(key, value)]]: a value is its entry's run and position."""
    out = []
    for r, run in enumerate(case_runs):
        out.append([((u + struct.pack("<Q", (s << 8) | t)) if cmp else u, bytes([r, i & 0xff, i >> 8]))
                    for i, (u, s, t) in enumerate(run)])
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="lsbm_mergefx_")
    exe = build_driver(tmp)
    cases = case_specs()
    cmds, order = [], []
    for name, runs in cases:
        for cmp in (0, 1):
            order.append((name, cmp, len(runs)))
            cmds.append(b"M" + p32(cmp) + p32(256) + p32(4) + p32(len(runs)) + b"".join(
                p32(len(run)) + b"".join(pstr(k) + pstr(v) for k, v in run) for run in entries_of(runs, cmp)))
    fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(fi, "wb").write(b"".join(cmds))
    subprocess.run([exe, fi, fo], check=True)
    buf, p = open(fo, "rb").read(), 0

    def u32():
        nonlocal p
        p += 4
        return struct.unpack_from("<I", buf, p - 4)[0]

    def s():
        nonlocal p
        n = u32()
        p += n
        return buf[p - n:p]

    blob, recs = bytearray(), []
    for name, cmp, n_runs in order:
        assert u32() == n_runs
        tables = []
        for _ in range(n_runs):
            f = s()
            tables.append([len(blob), len(f)])
            blob += f
        n, start = u32(), p
        for _ in range(2 * n):
            s()
        recs.append({"name": name, "cmp": cmp, "tables": tables, "n_merged": n,
                     "merged": [len(blob), p - start]})
        blob += buf[start:p]
    assert p == len(buf)
    fx = {"source": "lsbm's TableBuilder (kNoCompression, block_size 256, restart interval 4), Table::Open and "
                    "NewMergingIterator under both comparators, built from the reference's objects "
                    "(oracle/Makefile dbbench)",
          "cases": recs}
    open(os.path.join(HERE, "merge_tables.bin"), "wb").write(blob)
    json.dump(fx, open(os.path.join(HERE, "merge_fixture.json"), "w"), indent=0)
    print(f"{len(recs)} cases, {sum(len(r['tables']) for r in recs)} tables, "
          f"{sum(r['n_merged'] for r in recs)} merged records ({len(blob)} B)")


if __name__ == "__main__":
    sys.exit(main())
