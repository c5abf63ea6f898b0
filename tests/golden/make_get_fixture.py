"""Fixture of the reference's own read path for the GPU Get (include/lsbm_get.h).

    python tests/golden/make_get_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(built with -DNDEBUG; everything but db_bench's main), runs it, and writes
tests/golden/get_fixture.json and get_tables.bin.  Those objects are built
without snappy, so the reference's table/format.cc and table/table_builder.cc
are compiled once more for the driver with -DSNAPPY against a four-function
snappy.h of ours that forwards to oracle/snappy_oracle.c (the restatement the
suite pins to libsnappy); nothing else differs.

The driver
  * builds memtables with WriteBatch / WriteBatchInternal::InsertInto, records
    their iteration and calls MemTable::Get(LookupKey(k, s));
  * writes table files with TableBuilder (kNoCompression and
    kSnappyCompression, with and without InternalFilterPolicy over a 10-bit
    bloom, block_size 256);
  * fills FileMetaData vectors and calls the reference's FindFile, and restates
    the tests beside it (version_set.cc:364-379) over the reference's
    comparators;
  * opens table files (as built, or with bytes changed by this script) through
    the reference's TableCache and calls Get, or ContainKey and SkipFilterGet,
    with a saver that records the (ikey, value) it was handed and the returned
    status;
  * walks the probe list with the loop of version_set.cc:381-408, the saver's
    state set as SaveValue sets it (ParseInternalKey and the user comparator
    are the reference's; SaveValue itself is a static function).

Stored are each step's result and the final status string and value per query.
get_tables.bin is one zlib stream of the memtable iterations, the table files
and, as JSON text with keys in hex, each case's queries and recorded results;
get_fixture.json holds the cases' parameters and {offset, size} pairs into the
inflated bytes (`<name>_at` for a list that lives in the stream).

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
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

from golden import buildmodel as bd  # noqa: E402
from golden import snappytablemodel as stm  # noqa: E402

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

SNAPPY_H = r"""
// snappy.h for the fixture driver: the four calls port_posix.h makes, forwarded
// to oracle/snappy_oracle.c.
#pragma once
#include <stddef.h>
#include <stdint.h>
extern "C" {
uint64_t so_max_compressed_length(uint64_t n);
int so_get_uncompressed_length(const uint8_t* in, uint64_t n, uint32_t* out);
int so_uncompress(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* produced);
uint64_t so_compress(const uint8_t* in, uint32_t n, uint8_t* out);
}
namespace snappy {
inline size_t MaxCompressedLength(size_t n) { return so_max_compressed_length(n) + 8; }
inline void RawCompress(const char* in, size_t n, char* out, size_t* outlen) {
  *outlen = so_compress(reinterpret_cast<const uint8_t*>(in), (uint32_t)n, reinterpret_cast<uint8_t*>(out));
}
inline bool GetUncompressedLength(const char* in, size_t n, size_t* result) {
  uint32_t v = 0;
  if (!so_get_uncompressed_length(reinterpret_cast<const uint8_t*>(in), n, &v)) return false;
  *result = v;
  return true;
}
inline bool RawUncompress(const char* in, size_t n, char* out) {
  uint32_t v = 0;
  uint64_t produced = 0;
  if (!so_get_uncompressed_length(reinterpret_cast<const uint8_t*>(in), n, &v)) return false;
  return so_uncompress(reinterpret_cast<const uint8_t*>(in), n, reinterpret_cast<uint8_t*>(out), v, &produced) &&
         produced == v;
}
}  // namespace snappy
"""

DRIVER = r"""
// Driver for tests/golden/make_get_fixture.py: memtables, table files, FindFile
// and Get through the reference's classes, over a command file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/filter_policy.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "leveldb/table_builder.h"
#include "leveldb/write_batch.h"
#include "dbformat.h"
#include "filename.h"
#include "memtable.h"
#include "table_cache.h"
#include "write_batch_internal.h"
#include "lsbm/version_edit.h"
#include "lsbm/version_set.h"
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

static void write_iteration(MemTable* mem) {
  Iterator* it = mem->NewIterator();
  std::vector<std::string> ks, vs;
  for (it->SeekToFirst(); it->Valid(); it->Next()) {
    ks.push_back(it->key().ToString());
    vs.push_back(it->value().ToString());
  }
  delete it;
  w32(ks.size());
  for (size_t i = 0; i < ks.size(); i++) {
    wstr(ks[i]);
    wstr(vs[i]);
  }
}

// what SaveValue keeps, and what it was handed
enum SaverState { kNotFound, kFound, kDeleted, kCorrupt };
struct Saver {
  SaverState state;
  const Comparator* ucmp;
  Slice user_key;
  std::string value;
  bool called;
  std::string ikey, v;
};
static void Save(void* arg, const Slice& ikey, const Slice& v) {
  Saver* s = reinterpret_cast<Saver*>(arg);
  s->called = true;
  s->ikey = ikey.ToString();
  s->v = v.ToString();
  ParsedInternalKey parsed;
  if (!ParseInternalKey(ikey, &parsed)) {
    s->state = kCorrupt;
  } else if (s->ucmp->Compare(parsed.user_key, s->user_key) == 0) {
    s->state = (parsed.type == kTypeValue) ? kFound : kDeleted;
    if (s->state == kFound) s->value.assign(v.data(), v.size());
  }
}

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const std::string dbname = argv[3];
  InternalKeyComparator internal(BytewiseComparator());
  const Comparator* ucmp = BytewiseComparator();
  const FilterPolicy* bloom = NewBloomFilterPolicy(10);
  InternalFilterPolicy internal_bloom(bloom);
  Env* env = Env::Default();
  int c;
  while ((c = fgetc(in)) != EOF) {
    if (c == 'M') {  // batches, then n_queries x (user key, sequence)
      MemTable* mem = read_memtable(internal);
      write_iteration(mem);
      const uint32_t nq = r32();
      for (uint32_t q = 0; q < nq; q++) {
        std::string k = rstr();
        LookupKey lk(k, r64());
        std::string value;
        Status s;
        const bool got = mem->Get(lk, &value, &s);
        w32(got);
        wstr(s.ToString());
        wstr(value);
      }
      mem->Unref();
    } else if (c == 'T') {  // compression, filter, block_size, restart interval, n x (key, value)
      Options o;
      o.comparator = &internal;
      o.compression = r32() ? kSnappyCompression : kNoCompression;
      o.filter_policy = r32() ? &internal_bloom : NULL;
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
    } else if (c == 'F') {  // n_files x (smallest, largest, visible), n_queries x internal key
      const uint32_t nf = r32();
      std::vector<FileMetaData*> files;
      for (uint32_t i = 0; i < nf; i++) {
        FileMetaData* f = new FileMetaData();
        f->number = i + 1;
        std::string s = rstr(), g = rstr();
        f->smallest.DecodeFrom(s);
        f->largest.DecodeFrom(g);
        f->visible = r32() != 0;
        files.push_back(f);
      }
      const uint32_t nq = r32();
      for (uint32_t q = 0; q < nq; q++) {
        std::string ikey = rstr();
        const Slice user_key = ExtractUserKey(ikey);
        const uint32_t index = FindFile(internal, files, ikey);
        w32(index);
        // version_set.cc:376-378 and, for a buffer's table, :457
        const bool covered = index < files.size() && ucmp->Compare(user_key, files[index]->smallest.user_key()) >= 0;
        w32(covered ? 1 : 0);
        w32(covered && files[index]->visible ? 1 : 0);
        std::string overlap;  // version_set.cc:364-370, per file
        for (uint32_t i = 0; i < nf; i++)
          overlap.push_back(ucmp->Compare(user_key, files[i]->smallest.user_key()) >= 0 &&
                            ucmp->Compare(user_key, files[i]->largest.user_key()) <= 0 ? 1 : 0);
        wstr(overlap);
      }
      for (uint32_t i = 0; i < nf; i++) delete files[i];
    } else if (c == 'S') {  // n x (internal key, value, user key): the saver alone
      const uint32_t n = r32();
      for (uint32_t i = 0; i < n; i++) {
        std::string ikey = rstr(), v = rstr(), user = rstr();
        Saver saver;
        saver.state = kNotFound;
        saver.ucmp = ucmp;
        saver.user_key = user;
        saver.called = false;
        Save(&saver, ikey, v);
        w32(saver.state);
        wstr(saver.value);
      }
    } else if (c == 'V') {  // a version: memtables, files, runs, queries
      Options o;
      o.comparator = &internal;
      o.env = env;
      o.filter_policy = r32() ? &internal_bloom : NULL;
      ReadOptions ro;
      ro.verify_checksums = r32() != 0;
      ro.fill_cache = false;
      const uint32_t n_mem = r32();
      std::vector<MemTable*> mems;
      for (uint32_t i = 0; i < n_mem; i++) mems.push_back(read_memtable(internal));
      const uint32_t nf = r32();
      std::vector<FileMetaData*> files;
      for (uint32_t i = 0; i < nf; i++) {
        FileMetaData* f = new FileMetaData();
        f->number = r64();
        std::string bytes = rstr(), s = rstr(), g = rstr();
        f->file_size = bytes.size();
        f->smallest.DecodeFrom(s);
        f->largest.DecodeFrom(g);
        f->visible = r32() != 0;
        if (!WriteStringToFile(env, bytes, TableFileName(dbname, f->number)).ok()) exit(11);
        files.push_back(f);
      }
      const uint32_t n_runs = r32();
      std::vector<uint32_t> flags;
      std::vector<std::vector<FileMetaData*> > runs;
      for (uint32_t r = 0; r < n_runs; r++) {
        flags.push_back(r32());
        std::vector<FileMetaData*> fs;
        const uint32_t n = r32();
        for (uint32_t i = 0; i < n; i++) fs.push_back(files[r32()]);
        runs.push_back(fs);
      }
      TableCache* cache = new TableCache(dbname, &o, 100);
      const uint32_t nq = r32();
      for (uint32_t q = 0; q < nq; q++) {
        std::string user = rstr();
        LookupKey lk(user, r64());
        const Slice ikey = lk.internal_key(), user_key = lk.user_key();
        std::string value;
        Status s;
        int where = -1;
        bool done = false;
        for (uint32_t i = 0; i < n_mem && !done; i++) {
          if (mems[i]->Get(lk, &value, &s)) {
            done = true;
            where = i;
          }
        }
        std::vector<std::string> probes;  // one record per table read
        for (uint32_t r = 0; r < n_runs && !done; r++) {
          FileMetaData* f = NULL;
          if (flags[r] & 1) {  // version_set.cc:364-370
            FileMetaData* g = runs[r].empty() ? NULL : runs[r][0];
            if (g != NULL && ucmp->Compare(user_key, g->smallest.user_key()) >= 0 &&
                ucmp->Compare(user_key, g->largest.user_key()) <= 0)
              f = g;
          } else {  // :376-378, and :457's visible
            const uint32_t index = FindFile(internal, runs[r], ikey);
            if (index < runs[r].size() && ucmp->Compare(user_key, runs[r][index]->smallest.user_key()) >= 0 &&
                runs[r][index]->visible)
              f = runs[r][index];
          }
          if (f == NULL) continue;
          Saver saver;
          saver.state = kNotFound;
          saver.ucmp = ucmp;
          saver.user_key = user_key;
          saver.called = false;
          uint32_t contain = 2;  // not asked
          if (flags[r] & 2) {   // :441, :482
            contain = cache->ContainKey(ro, f->number, f->file_size, ikey) ? 1 : 0;
            if (contain) s = cache->SkipFilterGet(ro, f->number, f->file_size, ikey, &saver, Save);
          } else {
            s = cache->Get(ro, f->number, f->file_size, ikey, &saver, Save);
          }
          std::string rec;
          uint32_t head[4] = {r, (uint32_t)f->number, contain, (uint32_t)saver.called};
          rec.append(reinterpret_cast<const char*>(head), 16);
          probes.push_back(rec);
          probes.push_back(contain ? s.ToString() : std::string("OK"));
          probes.push_back(saver.ikey);
          probes.push_back(saver.v);
          if (!contain) continue;
          if (!s.ok()) {  // :392-394
            done = true;
            where = n_mem + r;
            break;
          }
          switch (saver.state) {  // :395-407
            case kNotFound:
              break;
            case kFound:
              value = saver.value;
              done = true;
              break;
            case kDeleted:
              s = Status::NotFound(Slice());
              done = true;
              break;
            case kCorrupt:
              s = Status::Corruption("corrupted key for ", user_key);
              done = true;
              break;
          }
          if (done) where = n_mem + r;
        }
        if (!done) s = Status::NotFound(Slice());
        w32(probes.size() / 4);
        for (size_t i = 0; i < probes.size(); i++) wstr(probes[i]);
        wstr(s.ToString());
        wstr(s.ok() ? value : std::string());
        w32((uint32_t)where);
      }
      delete cache;
      for (uint32_t i = 0; i < nf; i++) {
        env->DeleteFile(TableFileName(dbname, files[i]->number));
        delete files[i];
      }
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
    open(os.path.join(tmp, "snappy.h"), "w").write(SNAPPY_H)
    flags = ["-std=c++11", "-w", "-O2", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX", "-I" + REF,
             "-I" + REF + "/include", "-I" + REF + "/common"]
    for a in again:
        o = os.path.join(tmp, os.path.basename(a) + ".o")
        subprocess.run(["g++"] + flags + ["-DSNAPPY", "-I" + tmp, "-c", "-o", o, os.path.join(REF, a + ".cc")], check=True)
        objs.append(o)
    so = os.path.join(tmp, "snappy_oracle.o")
    subprocess.run(["gcc", "-O2", "-w", "-c", "-o", so, os.path.join(REPO, "oracle", "snappy_oracle.c")], check=True)
    src = os.path.join(tmp, "get_driver.cc")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "get_driver")
    subprocess.run(["g++"] + flags + ["-o", exe, src] + objs + [so], check=True)
    return exe


def p32(v):
    return struct.pack("<I", v)


def p64(v):
    return struct.pack("<Q", v)


def pstr(b):
    return p32(len(b)) + bytes(b)


def ikey(user, seq, kind=1):
    return bytes(user) + p64((seq << 8) | kind)


class Reader:
    def __init__(self, buf):
        self.buf, self.p = buf, 0

    def u32(self):
        self.p += 4
        return struct.unpack_from("<I", self.buf, self.p - 4)[0]

    def s(self):
        n = self.u32()
        self.p += n
        return self.buf[self.p - n:self.p]


def run_driver(exe, tmp, cmds):
    fi, fo, db = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), os.path.join(tmp, "db")
    os.makedirs(db, exist_ok=True)
    open(fi, "wb").write(b"".join(cmds))
    subprocess.run([exe, fi, fo, db], check=True)
    return Reader(open(fo, "rb").read())


def batches_cmd(batches):
    cmd = p32(len(batches))
    for seq, ops in batches:
        cmd += p64(seq) + p32(len(ops)) + b"".join(p32(t) + pstr(k) + pstr(v) for t, k, v in ops)
    return cmd


# ---------------------------------------------------------------- the cases


def memtable_specs():
    """[(name, [(sequence, [(type, key, value)])], [(user key, sequence)])]."""
    rng = random.Random(0x6E7F1A57)
    cases = []
    for n in (0, 1, 2, 255, 256, 257):
        users = [b"k%05d" % (2 * i + 2) for i in range(n)]
        order = list(range(n))
        rng.shuffle(order)
        ops = [(1 if i % 7 else 0, users[i], b"v%d" % i) for i in order]
        batches = [(10 + at, ops[at:at + 50]) for at in range(0, n, 50)]
        top = 10 + n
        picks = sorted(set(range(0, n, 16)) | {0, n - 1, n // 2, n - 2} & set(range(n)))
        queries = [(b"k", top), (b"k00001", top), (b"l", top), (b"k%05d" % (2 * n + 3), top)]
        for i in picks:
            queries += [(users[i], top), (users[i], 9), (users[i][:-1], top), (users[i] + b"\x00", top)]
            queries.append((b"k%05d" % (2 * i + 3), top))
        cases.append(("entries_%d" % n, batches, queries))
    long137 = bytes(rng.choice(b"xyz") for _ in range(137))
    sem = [(100, [(1, b"", b"empty-user-key"), (1, b"ab", b"AB"), (1, b"ab\x00", b"AB0"), (1, b"abc", b"ABC"),
                  (1, b"only-late", b"late"), (1, b"versions", b"v1"), (1, b"val-then-del", b"x"),
                  (0, b"del-then-val", b"")]),
           (200, [(1, b"versions", b"v2"), (0, b"val-then-del", b""), (1, b"del-then-val", b"back"),
                  (1, b"12345678" + b"a", b"8a"), (1, b"12345678" + b"b", b"8b"),
                  (1, b"0123456789abcdef" + b"a", b"16a"), (1, b"0123456789abcdef" + b"c", b"16c"),
                  (1, long137 + b"a", b"137a"), (1, long137 + b"c", b"137c")]),
           (300, [(1, b"versions", b"v3"), (1, b"only-late2", b"later")])]
    users = sorted({k for _, ops in sem for _, k, _ in ops})
    probes = users + [b"a", b"ab\x00\x00", b"abb", b"12345678", b"12345678b\x00", b"0123456789abcdefb",
                      long137 + b"b", long137, b"zzzz", b"only-lat", b"only-late1"]
    queries = [(u, s) for u in probes for s in (50, 104, 150, 201, 250, 1000)]
    cases.append(("semantics", sem, queries))
    return cases


def file_bounds(n):
    return [(ikey(b"f%03d_a" % i, 100 + i), ikey(b"f%03d_z" % i, 50, 1)) for i in range(n)]


def find_file_specs():
    """[(name, [(smallest, largest, visible)], [internal key])]."""
    cases = []
    for n in (0, 1, 2, 3, 64, 65):
        files = [(s, g, 0 if (n >= 3 and i == 1) else 1) for i, (s, g) in enumerate(file_bounds(n))]
        queries = [ikey(b"a", 70), ikey(b"f", 70), ikey(b"zzz", 70), ikey(b"", 70)]
        for i in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
            for user in (b"f%03d_a" % i, b"f%03d_" % i, b"f%03d_m" % i, b"f%03d_z" % i, b"f%03d_zz" % i):
                queries += [ikey(user, s) for s in (40, 50, 60, 200)]
            queries.append(ikey(b"f%03d_z" % i, 50, 0))
        cases.append(("files_%d" % n, files, queries))
    return cases


def saver_specs():
    """[(internal key, value, user key)]: the callback alone."""
    u = b"user-key"
    return [(ikey(u, 5, 1), b"value", u), (ikey(u, 5, 0), b"", u), (ikey(b"user-kez", 5, 1), b"other", u),
            (ikey(b"user", 5, 1), b"shorter", u), (ikey(b"user-key-longer", 5, 1), b"longer", u),
            (b"7 bytes", b"short", u), (b"", b"none", u), (ikey(u, 5, 2), b"type2", u),
            (ikey(b"user-key-longer", 5, 2), b"type2-longer", u), (ikey(b"another", 5, 255), b"type255", u),
            (ikey(b"", 9, 1), b"empty", b""), (ikey(b"", 9, 0), b"", b"")]


def table_entries(rng, prefix, n, seq0, deleted=(), extra=()):
    """Sorted [(internal key, value)]: users prefix%04d, one version each."""
    out = []
    for i in range(n):
        user = b"%s%04d" % (prefix, i)
        kind = 0 if i in deleted else 1
        out.append((ikey(user, seq0 + i, kind), b"" if not kind else b"%s-value-%d-" % (prefix, i) + bytes(
            rng.choice(b"abc") for _ in range(rng.randint(0, 40)))))
    out += list(extra)
    out.sort(key=lambda e: (e[0][:-8], -struct.unpack("<Q", e[0][-8:])[0]))
    return out


def reseal(data, handle, contents):
    """The file with the block at `handle` replaced by `contents` of the same size, its trailer recomputed."""
    off, size = handle
    assert len(contents) == size
    return data[:off] + contents + bd.trailer(contents, 0) + data[off + size + 5:]


def main():
    tmp = tempfile.mkdtemp(prefix="lsbm_getfx_")
    exe = build_driver(tmp)
    rng = random.Random(0x9E7A11)
    blob = bytearray()

    def keep(b):
        blob.extend(b)
        return [len(blob) - len(b), len(b)]

    # ---- phase A: memtables, FindFile, the saver, and the table files
    mems, finds, savers = memtable_specs(), find_file_specs(), saver_specs()
    hot = b"hot-key"
    tables = {  # name -> (compression, filter, entries)
        "l0_new": (0, 1, table_entries(rng, b"m", 30, 3000, extra=[(ikey(hot, 3500, 1), b"hot-newest"),
                                                                  (ikey(b"gone", 3600, 0), b"")])),
        "l0_mid": (0, 0, table_entries(rng, b"m", 40, 2000, deleted=(3, 4), extra=[(ikey(hot, 2500, 0), b""),
                                                                                 (ikey(b"gone", 2600, 1), b"was-here")])),
        "l0_old": (1, 1, table_entries(rng, b"m", 50, 1000, extra=[(ikey(hot, 1500, 1), b"hot-oldest")])),
        "l1_a": (1, 1, table_entries(rng, b"a", 60, 500, deleted=(7,))),
        "l1_b": (0, 0, table_entries(rng, b"m", 60, 600)),
        "l2_a": (0, 1, table_entries(rng, b"a", 80, 100)),
        "l2_b": (1, 0, table_entries(rng, b"m", 80, 200, extra=[(ikey(hot, 250, 1), b"hot-ancient")])),
        "l2_c": (1, 1, table_entries(rng, b"t", 80, 300)),
        # keys whose bytes are wrong: type byte 2 at the lookup key's length and longer
        "wrong": (0, 0, sorted([(ikey(b"w-corrupt", 7, 2), b"type2"), (ikey(b"w-deleted", 7, 0), b""),
                                (ikey(b"w-longer-corrupt", 7, 2), b"type2-longer"), (ikey(b"w-value", 7, 1), b"fine"),
                                (ikey(b"w-z", 7, 1), b"last")], key=lambda e: e[0][:-8])),
    }
    cmds = []
    for _, batches, queries in mems:
        cmds.append(b"M" + batches_cmd(batches) + p32(len(queries)) + b"".join(pstr(k) + p64(s) for k, s in queries))
    for _, files, queries in finds:
        cmds.append(b"F" + p32(len(files)) + b"".join(pstr(s) + pstr(g) + p32(v) for s, g, v in files)
                    + p32(len(queries)) + b"".join(pstr(k) for k in queries))
    cmds.append(b"S" + p32(len(savers)) + b"".join(pstr(k) + pstr(v) + pstr(u) for k, v, u in savers))
    for name, (comp, filt, entries) in tables.items():
        cmds.append(b"T" + p32(comp) + p32(filt) + p32(256) + p32(4) + p32(len(entries))
                    + b"".join(pstr(k) + pstr(v) for k, v in entries))
    rd = run_driver(exe, tmp, cmds)
    fx = {"source": "lsbm's WriteBatch, MemTable::Get, TableBuilder (block_size 256, restart interval 4, "
                    "kNoCompression / kSnappyCompression, InternalFilterPolicy over a 10-bit bloom where a file has "
                    "a filter), FindFile, TableCache::Get / ContainKey / SkipFilterGet and ParseInternalKey, built "
                    "from the reference's objects (oracle/Makefile dbbench, -DNDEBUG; table/format.cc and "
                    "table/table_builder.cc once more with -DSNAPPY over oracle/snappy_oracle.c); get_tables.bin is "
                    "one zlib stream, {offset, size} pairs index its inflated bytes",
          "memtables": [], "find_file": [], "saver": [], "versions": []}
    for name, batches, queries in mems:
        n, start = rd.u32(), rd.p
        for _ in range(2 * n):
            rd.s()
        rec = {"name": name, "n_entries": n, "iteration": keep(rd.buf[start:rd.p]), "queries": []}
        assert n == sum(len(ops) for _, ops in batches)
        for k, s in queries:
            got, status, value = rd.u32(), rd.s().decode(), rd.s()
            rec["queries"].append([k.hex(), s, got, status, value.hex()])
        fx["memtables"].append(rec)
    for name, files, queries in finds:
        rec = {"name": name, "files": [[s.hex(), g.hex(), v] for s, g, v in files], "queries": []}
        for k in queries:
            rec["queries"].append([k.hex(), rd.u32(), rd.u32(), rd.u32(), rd.s().hex()])
        fx["find_file"].append(rec)
    for k, v, u in savers:
        fx["saver"].append([k.hex(), v.hex(), u.hex(), rd.u32(), rd.s().hex()])
    built = {}
    for name, (comp, filt, entries) in tables.items():
        built[name] = rd.s()
        assert stm.decode_footer(built[name])
    assert rd.p == len(rd.buf)

    # ---- the files whose bytes this script changes
    def data_handles(data):
        from golden import blockmodel as bm
        _, index_handle = stm.decode_footer(data)
        index = data[index_handle[0]:index_handle[0] + index_handle[1]]
        assert data[index_handle[0] + index_handle[1]] == 0, "the index block must be raw"
        return [bm.decode_handle(bytes(index[vo:vo + vl])) for _, vo, vl, _ in bm.walk(index)[1]], index_handle, index

    # one data block of l0_mid with a flipped value byte (the block that holds "hot-key")
    handles, _, _ = data_handles(built["l0_mid"])
    from golden import blockmodel as bm
    at = None
    for h in handles:
        walked = bm.walk(built["l0_mid"][h[0]:h[0] + h[1]])[1]
        if any(k[:-8] == hot for k, _, _, _ in walked):
            at = h[0] + next(vo for _, vo, vl, _ in walked if vl >= 4) + 1
    assert at is not None
    flipped = built["l0_mid"][:at] + bytes([built["l0_mid"][at] ^ 0x40]) + built["l0_mid"][at + 1:]
    # l1_b with an index block whose last entry is bad: its value length runs past the restart array
    handles, index_handle, index = data_handles(built["l1_b"])
    walked = bm.walk(index)[1]
    last = walked[-1][3]
    assert index[last + 2] < 128
    bad_index = index[:last + 2] + bytes([127]) + index[last + 3:]
    assert bm.walk(bad_index)[0] == bm.BAD_ENTRY and len(bm.walk(bad_index)[1]) == len(walked) - 1
    bad_tail = reseal(built["l1_b"], index_handle, bad_index)
    files = dict(built, l0_mid_flipped=flipped, l1_b_bad_index=bad_tail)
    entries_of = {n: t[2] for n, t in tables.items()}
    entries_of["l0_mid_flipped"] = entries_of["l0_mid"]
    entries_of["l1_b_bad_index"] = entries_of["l1_b"]
    file_blob = {n: keep(d) for n, d in files.items()}

    # ---- phase B: the versions
    mem = [(5000, [(1, b"both", b"in-mem"), (1, b"m0001", b"mem-m0001"), (0, b"m0002", b""), (1, hot, b"hot-mem")])]
    imm = [(4000, [(1, b"both", b"in-imm"), (1, b"m0003", b"imm-m0003"), (0, b"a0001", b""), (1, b"imm-only", b"imm")])]
    users = [hot, b"both", b"imm-only", b"gone", b"never", b"", b"zzzz", b"m0000", b"m0001", b"m0002", b"m0003", b"m0004",
             b"m0005", b"m0029", b"m0030", b"m0039", b"m0040", b"m0049", b"m0050", b"m0059", b"m0060", b"m0079",
             b"m0080", b"a0000", b"a0001", b"a0007", b"a0059", b"a0060", b"a0079", b"a008", b"t0000", b"t0040",
             b"t0079", b"t0080", b"m00", b"m0010x"]
    snapshots = (150, 1250, 2550, 9999)
    main_runs = {"l0": ["l0_old", "l0_mid", "l0_new"], "levels": [(["l1_a", "l1_b"], []), ([], ["l2_a", "l2_b", "l2_c"])]}

    def version(name, swap, filt, verify, memtables, tree=None, runs=None, queries=None, invisible=()):
        number = {"l0_old": 11, "l0_mid": 12, "l0_new": 13, "l1_a": 21, "l1_b": 22, "l2_a": 31, "l2_b": 32, "l2_c": 33,
                  "wrong": 41}
        order, run_list = [], []

        def add(names, flags):
            idx = []
            for nm in names:
                order.append(nm)
                idx.append(len(order) - 1)
            run_list.append((flags, idx))

        if tree is not None:
            for nm in sorted(tree["l0"], key=lambda nm: -number[nm]):
                add([nm], 1)
            add([], 0)
            for deletion, insertion in tree["levels"]:
                add(deletion, 2)
                add(insertion, 2)
        else:
            for flags, names in runs:
                add(names, flags)
        recs = []
        for nm in order:
            real = swap.get(nm, nm)
            e = entries_of[real]
            recs.append({"name": real, "number": number[nm], "file": file_blob[real], "smallest": e[0][0].hex(),
                         "largest": e[-1][0].hex(), "visible": 0 if nm in invisible else 1,
                         "filter": tables[nm][1], "snappy": tables[nm][0]})
        qs = queries if queries is not None else [(u, s) for u in users for s in snapshots]
        cmd = b"V" + p32(filt) + p32(verify) + p32(len(memtables)) + b"".join(batches_cmd(m) for m in memtables)
        cmd += p32(len(recs))
        for r in recs:
            data = files[r["name"]]
            cmd += p64(r["number"]) + pstr(data) + pstr(bytes.fromhex(r["smallest"])) + \
                pstr(bytes.fromhex(r["largest"])) + p32(r["visible"])
        cmd += p32(len(run_list)) + b"".join(p32(fl) + p32(len(ix)) + b"".join(p32(i) for i in ix) for fl, ix in run_list)
        cmd += p32(len(qs)) + b"".join(pstr(u) + p64(s) for u, s in qs)
        return {"name": name, "filter_policy": filt, "verify": verify,
                "memtables": [[[seq, [[t, k.hex(), v.hex()] for t, k, v in ops]] for seq, ops in m] for m in memtables],
                "files": recs, "runs": [[fl, ix] for fl, ix in run_list], "tree": tree is not None,
                "queries": [[u.hex(), s] for u, s in qs]}, cmd

    level_queries = [(u, s) for u in users if u[:1] in (b"m", b"a", b"z", b"") for s in (650, 9999)]
    wrong_queries = [(u, 100) for u in (b"w-corrupt", b"w-deleted", b"w-longer", b"w-longer-corrupt", b"w-value", b"w-valu",
                                        b"w-value-longer", b"w-a", b"w-y", b"w-z", b"w-zz", b"w-d", b"w-corrupu")]
    specs = [version("tree", {}, 1, 1, [mem, imm], tree=main_runs),
             version("tree_no_filter_policy", {}, 0, 1, [], tree=main_runs),
             version("tree_flipped_block", {"l0_mid": "l0_mid_flipped"}, 1, 1, [mem, imm], tree=main_runs),
             version("tree_flipped_block_no_verify", {"l0_mid": "l0_mid_flipped"}, 1, 0, [mem, imm], tree=main_runs),
             version("bad_index_prechecked", {"l1_b": "l1_b_bad_index"}, 1, 1, [], runs=[(2, ["l1_a", "l1_b"])],
                     queries=level_queries),
             version("bad_index_plain", {"l1_b": "l1_b_bad_index"}, 1, 1, [], runs=[(0, ["l1_a", "l1_b"])],
                     queries=level_queries),
             version("invisible_file", {}, 1, 1, [], runs=[(0, ["l2_a", "l2_b", "l2_c"]), (0, ["l1_a", "l1_b"])],
                     queries=level_queries, invisible=("l2_b",)),
             version("wrong_bytes", {}, 0, 1, [], runs=[(0, ["wrong"])], queries=wrong_queries)]
    rd = run_driver(exe, tmp, [cmd for _, cmd in specs])
    for rec, _ in specs:
        results = []
        for _ in rec["queries"]:
            probes = []
            for _ in range(rd.u32()):
                head = struct.unpack("<4I", rd.s())
                probes.append({"run": head[0], "number": head[1], "contain": head[2], "saver_called": head[3],
                               "status": rd.s().decode(), "ikey": rd.s().hex(), "value": rd.s().hex()})
            status, value, where = rd.s().decode("latin-1"), rd.s().hex(), rd.u32()
            results.append({"probes": probes, "status": status, "value": value,
                            "where": where - (1 << 32) if where >= 1 << 31 else where})
        rec["results"] = results
        fx["versions"].append(rec)
    assert rd.p == len(rd.buf)

    # every case shows what it exists for, or the run fails
    by = {v["name"]: v for v in fx["versions"]}
    statuses = lambda v: {r["status"] for r in v["results"]}  # noqa: E731
    assert "Corruption: block checksum mismatch" in statuses(by["tree_flipped_block"])
    assert "Corruption: block checksum mismatch" not in statuses(by["tree_flipped_block_no_verify"])
    assert "Corruption: bad entry in block" in statuses(by["bad_index_plain"])
    assert "Corruption: bad entry in block" not in statuses(by["bad_index_prechecked"])
    assert any(s.startswith("Corruption: corrupted key for ") for s in statuses(by["wrong_bytes"]))
    assert any(p["contain"] == 0 for r in by["bad_index_prechecked"]["results"] for p in r["probes"])
    assert {"OK", "NotFound: "} <= statuses(by["tree"])
    assert any(s == 3 for _, _, _, s, _ in fx["saver"])

    # the records themselves go into the stream as JSON text; the JSON file keeps the parameters
    for kind, bulky in (("memtables", ("queries",)), ("find_file", ("files", "queries")),
                        ("versions", ("memtables", "files", "runs", "queries", "results"))):
        for rec in fx[kind]:
            for key in bulky:
                rec[key + "_at"] = keep(json.dumps(rec.pop(key), separators=(",", ":")).encode())
    fx["saver_at"] = keep(json.dumps(fx.pop("saver"), separators=(",", ":")).encode())
    fx["inflated_bytes"] = len(blob)
    packed = zlib.compress(bytes(blob), 9)
    open(os.path.join(HERE, "get_tables.bin"), "wb").write(packed)
    with open(os.path.join(HERE, "get_fixture.json"), "w") as f:
        parts = []  # one case a line
        for key, value in fx.items():
            one = json.dumps(value, separators=(",", ":"))
            if isinstance(value, list) and value and isinstance(value[0], dict):
                one = "[\n" + ",\n".join(json.dumps(v, separators=(",", ":")) for v in value) + "\n]"
            parts.append(json.dumps(key) + ":" + one)
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
    print(f"{len(fx['memtables'])} memtables, {len(fx['find_file'])} file sets, {len(fx['versions'])} versions "
          f"({len(blob)} B inflated, {len(packed)} B stored)")


if __name__ == "__main__":
    sys.exit(main())
