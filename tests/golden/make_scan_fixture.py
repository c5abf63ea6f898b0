"""Fixture of the reference's own iterator for the GPU range scan (include/lsbm_iter.h).

    python tests/golden/make_scan_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj, on
the pattern of make_get_fixture.py (whose snappy.h shim and build recipe it
shares), runs it, and writes tests/golden/scan_fixture.json and scan_tables.bin.

The driver
  * builds memtables with WriteBatch / WriteBatchInternal::InsertInto;
  * writes table files with TableBuilder (block_size 256, restart interval 4,
    kNoCompression and kSnappyCompression) -- keys with type bytes 2 and 255
    are handed to Add as they are, as make_get_fixture.py's "wrong" table does;
  * opens the files through the reference's TableCache and, per query, makes
    NewMergingIterator over MemTable::NewIterator and TableCache::NewIterator
    (the children of DBImpl::NewInternalIterator, lsbm/db_impl.cc:1139-1157) and
    wraps it in NewDBIterator(NULL, BytewiseComparator(), iter, s, seed) -- db_
    is stored and never used in this version of db_iter.cc;
  * records each child's iteration and the merging iterator's, and for each
    query every (key, value) the idioms of golden/scanmodel.py yield and the
    final status().ToString().  A fresh iterator is made per query.

scan_tables.bin is one zlib stream of the iterations and, as JSON text with
keys in hex, each case's queries and recorded results; scan_fixture.json holds
the cases' parameters and {offset, size} pairs into the inflated bytes.

Only bytes produced by the reference are stored; no reference source.
"""
import glob
import json
import os
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

from golden import make_get_fixture as gf  # noqa: E402
from golden.make_get_fixture import batches_cmd, ikey, p32, p64, pstr  # noqa: E402

REF, OBJ = gf.REF, gf.OBJ
kMaxSequenceNumber = (1 << 56) - 1

DRIVER = r"""
// Driver for tests/golden/make_scan_fixture.py: memtables, table files and
// DBIter over a MergingIterator through the reference's classes, over a
// command file.
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
#include "leveldb/table_builder.h"
#include "leveldb/write_batch.h"
#include "dbformat.h"
#include "filename.h"
#include "memtable.h"
#include "table_cache.h"
#include "write_batch_internal.h"
#include "table/merger.h"
#include "lsbm/db_iter.h"
using namespace leveldb;

static FILE *in, *out;
static uint32_t r32() { uint32_t v; if (fread(&v, 4, 1, in) != 1) exit(3); return v; }
static uint64_t r64() { uint64_t v; if (fread(&v, 8, 1, in) != 1) exit(3); return v; }
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

static MemTable* read_memtable(const InternalKeyComparator& internal) {
  MemTable* mem = new MemTable(internal);
  mem->Ref();
  const uint32_t n_batches = r32();
  for (uint32_t b = 0; b < n_batches; b++) {
    WriteBatch batch;
    WriteBatchInternal::SetSequence(&batch, r64());
    const uint32_t n_ops = r32();
    for (uint32_t i = 0; i < n_ops; i++) {
      const uint32_t type = r32();
      std::string k = rstr(), v = rstr();
      if (type) batch.Put(k, v); else batch.Delete(k);
    }
    if (!WriteBatchInternal::InsertInto(&batch, mem).ok()) exit(5);
  }
  return mem;
}

static void write_iteration(Iterator* it) {
  std::vector<std::string> ks, vs;
  for (it->SeekToFirst(); it->Valid(); it->Next()) {
    ks.push_back(it->key().ToString());
    vs.push_back(it->value().ToString());
  }
  if (!it->status().ok()) exit(6);
  delete it;
  w32(ks.size());
  for (size_t i = 0; i < ks.size(); i++) {
    wstr(ks[i]);
    wstr(vs[i]);
  }
}

struct TableRef { uint64_t number, size; };

static Iterator* internal_iterator(const InternalKeyComparator& internal, const std::vector<MemTable*>& mems,
                                   TableCache* cache, const ReadOptions& ro, const std::vector<TableRef>& tables) {
  std::vector<Iterator*> list;
  for (size_t i = 0; i < mems.size(); i++) list.push_back(mems[i]->NewIterator());
  for (size_t i = 0; i < tables.size(); i++) list.push_back(cache->NewIterator(ro, tables[i].number, tables[i].size));
  return NewMergingIterator(&internal, list.empty() ? NULL : &list[0], list.size());
}

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const std::string dbname = argv[3];
  InternalKeyComparator internal(BytewiseComparator());
  Env* env = Env::Default();
  int c;
  while ((c = fgetc(in)) != EOF) {
    if (c == 'T') {  // compression, block_size, restart interval, n x (key, value)
      Options o;
      o.comparator = &internal;
      o.compression = r32() ? kSnappyCompression : kNoCompression;
      o.block_size = r32();
      o.block_restart_interval = (int)r32();
      const uint32_t n = r32();
      StringSink table;
      TableBuilder builder(o, &table);
      for (uint32_t i = 0; i < n; i++) {
        std::string k = rstr(), v = rstr();
        builder.Add(k, v);
      }
      if (!builder.Finish().ok() || builder.FileSize() != table.contents.size()) exit(7);
      wstr(table.contents);
    } else if (c == 'D') {  // a database: memtables, table files, queries
      Options o;
      o.comparator = &internal;
      o.env = env;
      ReadOptions ro;
      ro.verify_checksums = true;
      ro.fill_cache = false;
      const uint32_t n_mem = r32();
      std::vector<MemTable*> mems;
      for (uint32_t i = 0; i < n_mem; i++) mems.push_back(read_memtable(internal));
      const uint32_t nt = r32();
      std::vector<TableRef> tables;
      for (uint32_t i = 0; i < nt; i++) {
        TableRef t;
        t.number = r64();
        std::string bytes = rstr();
        t.size = bytes.size();
        if (!WriteStringToFile(env, bytes, TableFileName(dbname, t.number)).ok()) exit(11);
        tables.push_back(t);
      }
      TableCache* cache = new TableCache(dbname, &o, 100);
      for (uint32_t i = 0; i < n_mem; i++) write_iteration(mems[i]->NewIterator());
      for (uint32_t i = 0; i < nt; i++) write_iteration(cache->NewIterator(ro, tables[i].number, tables[i].size));
      write_iteration(internal_iterator(internal, mems, cache, ro, tables));
      const uint32_t nq = r32();
      for (uint32_t q = 0; q < nq; q++) {
        const uint64_t snapshot = r64();
        const uint32_t has_lo = r32(), has_hi = r32(), reverse = r32();
        const std::string lo = rstr(), hi = rstr();
        const uint64_t limit = r64();
        Iterator* it = NewDBIterator(NULL, BytewiseComparator(), internal_iterator(internal, mems, cache, ro, tables),
                                     snapshot, 301 + q);
        std::vector<std::string> got;
        uint64_t n = 0;
        if (limit > 0 && !reverse) {
          if (has_lo) it->Seek(lo); else it->SeekToFirst();
          while (n < limit && it->Valid() && (!has_hi || it->key().compare(hi) < 0)) {
            got.push_back(it->key().ToString());
            got.push_back(it->value().ToString());
            if (++n == limit) break;
            it->Next();
          }
        } else if (limit > 0) {
          if (has_hi) {
            it->Seek(hi);
            if (it->Valid()) it->Prev(); else it->SeekToLast();
          } else {
            it->SeekToLast();
          }
          while (n < limit && it->Valid() && (!has_lo || it->key().compare(lo) >= 0)) {
            got.push_back(it->key().ToString());
            got.push_back(it->value().ToString());
            if (++n == limit) break;
            it->Prev();
          }
        }
        w32(got.size() / 2);
        for (size_t i = 0; i < got.size(); i++) wstr(got[i]);
        wstr(it->status().ToString());
        delete it;
      }
      delete cache;
      for (uint32_t i = 0; i < nt; i++) env->DeleteFile(TableFileName(dbname, tables[i].number));
      for (uint32_t i = 0; i < n_mem; i++) mems[i]->Unref();
    } else {
      exit(10);
    }
  }
  fclose(out);
  return 0;
}
"""


def build_driver(tmp):
    if not os.path.isdir(OBJ):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "dbbench"], check=True)
    again = ("table/format", "table/table_builder")  # once more, with snappy
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*", "*.o")))
            if not o.endswith("lsbm/db_bench.o") and not any(o.endswith(a + ".o") for a in again)]
    open(os.path.join(tmp, "snappy.h"), "w").write(gf.SNAPPY_H)
    flags = ["-std=c++11", "-w", "-O2", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX", "-I" + REF,
             "-I" + REF + "/include", "-I" + REF + "/common"]
    for a in again:
        o = os.path.join(tmp, os.path.basename(a) + ".o")
        subprocess.run(["g++"] + flags + ["-DSNAPPY", "-I" + tmp, "-c", "-o", o, os.path.join(REF, a + ".cc")], check=True)
        objs.append(o)
    so = os.path.join(tmp, "snappy_oracle.o")
    subprocess.run(["gcc", "-O2", "-w", "-c", "-o", so, os.path.join(REPO, "oracle", "snappy_oracle.c")], check=True)
    src = os.path.join(tmp, "scan_driver.cc")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "scan_driver")
    subprocess.run(["g++"] + flags + ["-o", exe, src] + objs + [so], check=True)
    return exe


# ---------------------------------------------------------------- the cases


def sort_entries(entries):
    return sorted(entries, key=lambda e: (e[0][:-8], -int.from_bytes(e[0][-8:], "little")))


def semantics_case():
    """One memtable (batches) and two tables ([(internal key, value)], raw and
    snappy).  Sequence numbers are 10..90, so the snapshots below sit below all
    of them, between two versions, at versions exactly, and above all."""
    mem = [(50, [(0, b"", b""),                        # seq 50: the first user key deleted
                 (1, b"both", b"both-mem"),            # 51
                 (1, b"versions", b"v51")]),       # 52
           (80, [(0, b"zz-last", b""),                 # 80: the last user key deleted
                 (1, b"late", b"only-late")])]         # 81: versions only above most snapshots
    long_user = b"L" * 137
    t0 = [(ikey(b"", 10), b"empty-user-key"),
          (ikey(b"ab", 11), b"AB"), (ikey(b"ab\x00", 12), b"AB0"),          # a prefix pair
          (ikey(b"both", 30), b"both-t0"),
          (ikey(b"dup", 33), b"dup-t0"),                                   # the same internal key in two children
          (ikey(b"del-then-val", 21, 0), b""),
          (ikey(b"val-then-del", 22), b"was-here"),
          (ikey(b"k1", 14), b"K1"),
          (ikey(b"k2", 55, 255), b"type255"), (ikey(b"k2", 16), b"K2"),    # an error key above a value of its user key
          (ikey(b"k3", 17), b""),                                          # an empty value
          (ikey(b"k5", 18), b"K5" * 300),
          (ikey(b"versions", 15), b"v15"), (ikey(b"versions", 35), b"v35"),
          (ikey(long_user, 23), b"long-key"),
          (ikey(b"zz-last", 19), b"last")]
    t1 = [(ikey(b"abc", 13), b"ABC"),
          (ikey(b"both", 40), b"both-t1"),
          (ikey(b"dup", 33), b"dup-t1"),
          (ikey(b"del-then-val", 41), b"back-again"),
          (ikey(b"val-then-del", 42, 0), b""),
          (ikey(b"k4", 44, 2), b"type2"),                                  # a user key with an error key only
          (ikey(b"versions", 25), b"v25"), (ikey(b"versions", 45), b"v45"),
          (ikey(b"zz-last", 20, 2), b"type2-old")]                         # an error key below a value
    tables = [(0, sort_entries(t0)), (1, sort_entries(t1))]
    users = [b"", b"ab", b"ab\x00", b"abc", b"both", b"del-then-val", b"dup", b"k1", b"k2", b"k3", b"k4", b"k5",
             b"late", b"val-then-del", b"versions", long_user, b"zz-last"]
    users = sorted(users)
    probes = users + [b"a", b"k", b"k2\x00", b"k45", b"zzzz"]  # between keys, and past the last
    intervals = [(None, None)] + [(k, None) for k in probes] + [(None, k) for k in probes]
    intervals += [(k, k) for k in (b"", b"both", b"k2", b"zzzz")]                              # hi == lo
    intervals += [(users[i], users[i + 1]) for i in range(len(users) - 1)]
    intervals += [(users[i], users[i + 3]) for i in range(0, len(users) - 3, 2)]
    intervals += [(users[i + 2], users[i]) for i in range(0, len(users) - 2, 3)]               # hi < lo
    intervals += [(b"k1", b"k2"), (b"k1", b"k2\x00"), (b"k2", b"k3"), (b"k3", b"k45"), (b"k45", b"k5"),
                  (b"k3", b"k4"), (b"k4", b"k5"), (b"zzzz", None), (b"zzzz", b"zzzzz"), (None, b""), (b"", b"")]
    snapshots = (5, 16, 24, 33, 42, 45, 55, 60, 85, kMaxSequenceNumber)
    queries = [(s, lo, hi, limit, rev) for s in snapshots for lo, hi in intervals for limit in (0, 1, 2, 1000)
               for rev in (0, 1)]
    return "semantics", [mem], tables, queries


def empty_case():
    queries = [(s, lo, hi, limit, rev) for s in (0, 7, kMaxSequenceNumber) for lo, hi in
               ((None, None), (b"a", None), (None, b"a"), (b"a", b"b")) for limit in (0, 1, 5) for rev in (0, 1)]
    return "empty", [], [], queries


def tables_only_case():
    """No memtable; one user key whose every version is in a table of its own."""
    tables = [(0, [(ikey(b"p", 7), b"p7"), (ikey(b"q", 9, 0), b"")]), (1, [(ikey(b"p", 8, 0), b""), (ikey(b"q", 6), b"q6")]),
              (0, [(ikey(b"p", 9), b"p9"), (ikey(b"r", 3, 255), b"bad")])]
    queries = [(s, lo, hi, limit, rev) for s in (2, 3, 6, 7, 8, 9, 10) for lo, hi in
               ((None, None), (b"p", None), (b"q", None), (None, b"q"), (None, b"r"), (b"p", b"q"), (b"q", b"r"),
                (b"r", None), (b"q", b"p")) for limit in (0, 1, 2, 9) for rev in (0, 1)]
    return "tables_only", [], tables, queries


def main():
    tmp = tempfile.mkdtemp(prefix="lsbm_scanfx_")
    exe = build_driver(tmp)
    cases = [semantics_case(), empty_case(), tables_only_case()]
    blob = bytearray()

    def keep(b):
        blob.extend(b)
        return [len(blob) - len(b), len(b)]

    # ---- phase A: the table files
    cmds = []
    for _, _, tables, _ in cases:
        for comp, entries in tables:
            cmds.append(b"T" + p32(comp) + p32(256) + p32(4) + p32(len(entries))
                        + b"".join(pstr(k) + pstr(v) for k, v in entries))
    rd = gf.run_driver(exe, tmp, cmds)
    files = [[rd.s() for _ in tables] for _, _, tables, _ in cases]
    assert rd.p == len(rd.buf)

    # ---- phase B: the databases
    cmds = []
    for (name, mems, tables, queries), built in zip(cases, files):
        cmd = b"D" + p32(len(mems)) + b"".join(batches_cmd(m) for m in mems) + p32(len(built))
        cmd += b"".join(p64(11 + i) + pstr(data) for i, data in enumerate(built))
        cmd += p32(len(queries))
        for s, lo, hi, limit, rev in queries:
            cmd += p64(s) + p32(lo is not None) + p32(hi is not None) + p32(rev) + pstr(lo or b"") + pstr(hi or b"") + \
                p64(limit)
        cmds.append(cmd)
    rd = gf.run_driver(exe, tmp, cmds)
    fx = {"source": "lsbm's WriteBatch, MemTable, TableBuilder (block_size 256, restart interval 4, kNoCompression / "
                    "kSnappyCompression), TableCache::NewIterator, NewMergingIterator and NewDBIterator, built from "
                    "the reference's objects (oracle/Makefile dbbench, -DNDEBUG; table/format.cc and "
                    "table/table_builder.cc once more with -DSNAPPY over oracle/snappy_oracle.c); scan_tables.bin "
                    "is one zlib stream, {offset, size} pairs index its inflated bytes.  An iteration is u32 n, "
                    "then n x (u32 length, key, u32 length, value); a query record is [snapshot, lo hex or null, "
                    "hi hex or null, limit, reverse, [[key hex, value hex]], status]",
          "cases": []}
    for name, mems, tables, queries in cases:
        def iteration():
            n, start = rd.u32(), rd.p
            for _ in range(2 * n):
                rd.s()
            return {"n_entries": n, "at": keep(rd.buf[start - 4:rd.p])}
        rec = {"name": name, "n_memtables": len(mems), "n_tables": len(tables),
               "snappy": [comp for comp, _ in tables],
               "children": [iteration() for _ in range(len(mems) + len(tables))], "merged": iteration()}
        results = []
        for s, lo, hi, limit, rev in queries:
            got = [[rd.s().hex(), rd.s().hex()] for _ in range(rd.u32())]
            results.append([s, None if lo is None else lo.hex(), None if hi is None else hi.hex(), limit, rev, got,
                            rd.s().decode()])
        rec["n_queries"] = len(results)
        rec["queries_at"] = keep(json.dumps(results, separators=(",", ":")).encode())
        rec["statuses"] = sorted({r[6] for r in results})
        fx["cases"].append(rec)
    assert rd.p == len(rd.buf)

    # every case shows what it exists for, or the run fails
    by = {c["name"]: c for c in fx["cases"]}
    assert by["semantics"]["statuses"] == ["Corruption: corrupted internal key in DBIter", "OK"]
    assert by["empty"]["statuses"] == ["OK"]
    assert by["semantics"]["merged"]["n_entries"] == sum(c["n_entries"] for c in by["semantics"]["children"])

    fx["inflated_bytes"] = len(blob)
    packed = zlib.compress(bytes(blob), 9)
    open(os.path.join(HERE, "scan_tables.bin"), "wb").write(packed)
    with open(os.path.join(HERE, "scan_fixture.json"), "w") as f:
        f.write("{\n" + json.dumps("source") + ":" + json.dumps(fx["source"]) + ",\n" + json.dumps("cases") + ":[\n"
                + ",\n".join(json.dumps(c, separators=(",", ":")) for c in fx["cases"]) + "\n],\n"
                + json.dumps("inflated_bytes") + ":" + str(fx["inflated_bytes"]) + "\n}\n")
    print(f"{len(fx['cases'])} cases, {sum(c['n_queries'] for c in fx['cases'])} queries "
          f"({len(blob)} B inflated, {len(packed)} B stored)")


if __name__ == "__main__":
    sys.exit(main())
