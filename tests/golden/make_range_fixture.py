"""Fixture of the reference's own Version::RangeQuery and TableCache::GetRange
over the sorted-table lists, for the GPU's range query (include/lsbm_range.h,
lsbm_amd/rangequery.py).

    python tests/golden/make_range_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj, as
make_buffered_fixture.py does, runs it on the cases below, and writes
tests/golden/range_fixture.json (the index) and range_tables.bin (one zlib
stream of JSON text).

Per case the driver writes small table files with TableBuilder (block_size
256, restart interval 4, a 10-bit bloom under InternalFilterPolicy), damages the
index block of the files the case names, writes a MANIFEST, runs
BasicVersionSet::Recover() and records the recovered lists.  For every query of
the case it records TableCache::GetRange's count on every file of the tree,
called directly.  Per run it sets runtime::compaction_buffer_use_length[],
config::buffered_merge, runtime::read_cursor_key_[] and runtime::read_upto_key_,
and per query gives the version a fresh TableCache over an Env that logs
NewRandomAccessFile, calls the recovered version's RangeQuery(ReadOptions(),
LookupKey(start, s), LookupKey(end, s)) and records its return value and the
log: the files it read, each once, in order.

Only bytes and results the reference produced are stored, beside the cases'
own description; no reference source.
"""
import json
import os
import struct
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

from golden import make_buffered_fixture as mbf  # noqa: E402
from golden.make_buffered_fixture import CB, DEL, INS, WB, Reader, entry, ikey, pstr  # noqa: E402

DRIVER = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>
#define private public
#define protected public
#include "lsbm/version_edit.h"
#include "lsbm/version_set.h"
#undef private
#undef protected
#include "common/filename.h"
#include "common/log_writer.h"
#include "common/table_cache.h"
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/filter_policy.h"
#include "leveldb/options.h"
#include "leveldb/params.h"
#include "leveldb/table_builder.h"
#include "table/format.h"
#include "util/coding.h"
#include "util/crc32c.h"

using namespace leveldb;

static FILE* out;
static FILE* in;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void w64(uint64_t v) { fwrite(&v, 8, 1, out); }
static void wstr(const std::string& s) { w32(s.size()); fwrite(s.data(), 1, s.size(), out); }
static uint32_t r32() { uint32_t v; if (fread(&v, 4, 1, in) != 1) exit(3); return v; }
static uint64_t r64() { uint64_t v; if (fread(&v, 8, 1, in) != 1) exit(3); return v; }
static std::string rstr() {
  std::string s(r32(), '\0');
  if (s.size() && fread(&s[0], 1, s.size(), in) != s.size()) exit(3);
  return s;
}
static InternalKey key_of(const std::string& s) { InternalKey k; k.DecodeFrom(s); return k; }

static void damage_index(std::string* file) {
  Footer footer;
  Slice tail(file->data() + file->size() - Footer::kEncodedLength, Footer::kEncodedLength);
  if (!footer.DecodeFrom(&tail).ok()) exit(8);
  const uint64_t off = footer.index_handle().offset(), n = footer.index_handle().size();
  memset(&(*file)[off + n - 4], 0xff, 4);
  const uint32_t crc = crc32c::Value(file->data() + off, n + 1);
  EncodeFixed32(&(*file)[off + n + 1], crc32c::Mask(crc));
}

// every table file opened for reading, by number, in order
class LoggingEnv : public EnvWrapper {
 public:
  explicit LoggingEnv(Env* base) : EnvWrapper(base) {}
  std::vector<uint64_t> opened;
  virtual Status NewRandomAccessFile(const std::string& fname, RandomAccessFile** result) {
    const size_t slash = fname.rfind('/');
    uint64_t number = 0;
    FileType type;
    if (ParseFileName(fname.substr(slash + 1), &number, &type) && type == kTableFile) opened.push_back(number);
    return target()->NewRandomAccessFile(fname, result);
  }
};

struct Query { std::string start, end; uint64_t snapshot; };

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const std::string dir = argv[3];
  if (!in || !out) return 2;
  LoggingEnv* env = new LoggingEnv(Env::Default());
  InternalKeyComparator icmp(BytewiseComparator());
  const FilterPolicy* bloom = NewBloomFilterPolicy(10);
  InternalFilterPolicy internal_bloom(bloom);
  const uint32_t n_cases = r32();
  for (uint32_t c = 0; c < n_cases; c++) {
    char sub[32];
    snprintf(sub, sizeof(sub), "/c%u", c);
    const std::string db = dir + sub;
    env->CreateDir(db);
    Options options;
    options.env = env;
    options.comparator = &icmp;
    options.filter_policy = &internal_bloom;
    options.compression = kNoCompression;
    options.block_size = 256;
    options.block_restart_interval = 4;
    std::map<uint64_t, uint64_t> size_of;
    const uint32_t n_files = r32();
    for (uint32_t i = 0; i < n_files; i++) {
      const uint64_t number = r64();
      const std::string name = TableFileName(db, number);
      WritableFile* wf;
      if (!env->NewWritableFile(name, &wf).ok()) return 4;
      {
        TableBuilder builder(options, wf);
        const uint32_t n = r32();
        for (uint32_t k = 0; k < n; k++) {
          const std::string key = rstr(), value = rstr();
          builder.Add(key, value);
        }
        if (!builder.Finish().ok()) return 4;
      }
      wf->Close();
      delete wf;
      std::string bytes;
      if (!ReadFileToString(env, name, &bytes).ok()) return 4;
      if (r32()) {
        damage_index(&bytes);
        if (!WriteStringToFile(env, bytes, name).ok()) return 4;
      }
      size_of[number] = bytes.size();
      wstr(bytes);
    }
    const std::string manifest = db + "/MANIFEST-000002";
    WritableFile* wf;
    if (!env->NewWritableFile(manifest, &wf).ok()) return 4;
    {
      log::Writer writer(wf);
      const uint32_t n_records = r32();
      for (uint32_t i = 0; i < n_records; i++) {
        VersionEdit edit;
        if (i == 0) {
          edit.SetComparatorName(icmp.user_comparator()->Name());
          edit.SetLogNumber(3);
          edit.SetNextFile(1000);
          edit.SetLastSequence(1000);
        }
        const uint32_t n_del = r32();
        for (uint32_t k = 0; k < n_del; k++) {
          const uint32_t t = r32(), level = r32();
          edit.DeleteFile((SortedTableType)t, level, r64());
        }
        const uint32_t n_new = r32();
        for (uint32_t k = 0; k < n_new; k++) {
          const uint32_t t = r32(), level = r32();
          const uint64_t number = r64();
          const std::string a = rstr(), b = rstr();
          edit.AddFile((SortedTableType)t, level, number, size_of.count(number) ? size_of[number] : 0, key_of(a),
                       key_of(b));
        }
        std::string rec;
        edit.EncodeTo(&rec);
        if (!writer.AddRecord(rec).ok()) return 4;
      }
    }
    wf->Close();
    delete wf;
    std::string bytes;
    if (!ReadFileToString(env, manifest, &bytes).ok()) return 4;
    wstr(bytes);
    if (!WriteStringToFile(env, "MANIFEST-000002\n", db + "/CURRENT").ok()) return 4;
    for (int i = 0; i < 4; i++) runtime::compaction_buffer_length[i] = (int)r32();
    runtime::write_cursor = 0;
    for (int i = 0; i < 4; i++) runtime::read_cursor_[i] = 0;
    TableCache* direct = new TableCache(db, &options, 1000);
    BasicVersionSet* vs = new BasicVersionSet(db, &options, direct, &icmp);  // (never deleted: its destructor asserts)
    const Status s = vs->Recover();
    wstr(s.ToString());
    if (!s.ok()) return 5;
    Version* v = vs->current();
    for (int level = 0; level < config::kNumLevels; level++) {
      for (int type = 0; type < 4; type++) {
        SortedTable* head = v->levels_[level][type];
        uint32_t n_tables = 0;
        SortedTable* cur = head;
        do { n_tables++; cur = cur->next; } while (cur != head);
        w32(n_tables);
        do {
          w32(cur->files_.size());
          for (size_t i = 0; i < cur->files_.size(); i++) w64(cur->files_[i]->number);
          cur = cur->next;
        } while (cur != head);
      }
    }
    // the queries, and GetRange of each on every file, called directly
    std::vector<Query> queries(r32());
    for (size_t q = 0; q < queries.size(); q++) {
      queries[q].start = rstr();
      queries[q].end = rstr();
      queries[q].snapshot = r64();
      LookupKey lkstart(queries[q].start, queries[q].snapshot), lkend(queries[q].end, queries[q].snapshot);
      for (std::map<uint64_t, uint64_t>::iterator it = size_of.begin(); it != size_of.end(); ++it)
        w32(direct->GetRange(ReadOptions(), BytewiseComparator(), it->first, it->second, lkstart.internal_key(),
                             lkend.internal_key()));
    }
    const uint32_t n_runs = r32();
    for (uint32_t r = 0; r < n_runs; r++) {
      for (int i = 0; i < 4; i++) runtime::compaction_buffer_use_length[i] = (int)r32();
      config::buffered_merge = r32() != 0;
      for (int i = 0; i < 4; i++) runtime::read_cursor_key_[i] = rstr();
      runtime::read_upto_key_ = rstr();
      for (size_t q = 0; q < queries.size(); q++) {
        LookupKey lkstart(queries[q].start, queries[q].snapshot), lkend(queries[q].end, queries[q].snapshot);
        TableCache* fresh = new TableCache(db, &options, 1000);  // nothing cached: every file read is opened
        const_cast<TableCache*&>(vs->table_cache_) = fresh;  // (a const pointer member)
        env->opened.clear();
        const int found = v->RangeQuery(ReadOptions(), lkstart, lkend);
        const_cast<TableCache*&>(vs->table_cache_) = direct;
        delete fresh;
        w32((uint32_t)found);
        w32(env->opened.size());
        for (size_t i = 0; i < env->opened.size(); i++) w64(env->opened[i]);
      }
    }
  }
  fclose(out);
  return 0;
}
"""


def k(i, p=b"kkkkk"):
    """An 8-byte user key: a start key may not be shorter (FindFile reads its last 8 bytes as a tag)."""
    return p + b"%03d" % i


def table(number, users, seq=10, extra=()):
    """A file's entries [(internal key, value)], sorted: every user key of
    `users` at `seq`, plus `extra` [(user, seq, type)] entries."""
    ents = [(u, seq, 1) for u in users] + list(extra)
    ents.sort(key=lambda e: (e[0], -e[1], -e[2]))
    return [(ikey(u, s, t), b"f%d" % number) for u, s, t in ents]


def rng(lo, hi, p=b"kkkkk"):
    return [k(i, p) for i in range(lo, hi)]


def run(use, merge, cursors, upto):
    return {"use_length": list(use), "buffered_merge": bool(merge), "read_cursor_keys": [bytes(c) for c in cursors],
            "read_upto_key": bytes(upto)}


LOW = (b"", b"", b"", b"")
TOP = b"kz"  # a read_upto_key above every end key here
Z8, F8 = b"\x00" * 8, b"\xff" * 8


def buffer_level(f, added, level, number, n_wb, n_cb):
    """Level `level` over k000..k029: DEL (k000..k024), INS (all), n_cb
    compaction-buffer tables and n_wb warm-up tables, added oldest first so that
    each opens a new sorted table.  The list is [sentinel, newest, .., oldest].
    The table a walk calls covering (the oldest compaction-buffer table; the
    second oldest warm-up table) holds k000..k014 only; the newest
    compaction-buffer table k005..k029; the oldest warm-up table two files with a
    gap (k010..k014)."""
    f[number] = table(number, rng(0, 25), seq=100 * level + 1)
    f[number + 1] = table(number + 1, rng(0, 30), seq=100 * level + 2)
    added += [entry(DEL, level, number, f), entry(INS, level, number + 1, f)]
    for j in range(n_cb):
        n = number + 10 + j
        lo, hi = (0, 15) if j == 0 else ((5, 30) if j == n_cb - 1 else (0, 30))
        f[n] = table(n, rng(lo, hi), seq=100 * level + 10 + j)
        added.append(entry(CB, level, n, f))
    for j in range(n_wb):
        n = number + 20 + 2 * j
        if j == 0:
            f[n] = table(n, rng(0, 10), seq=100 * level + 20)
            f[n + 1] = table(n + 1, rng(15, 30), seq=100 * level + 20)
            added += [entry(WB, level, n, f), entry(WB, level, n + 1, f)]
        else:
            f[n] = table(n, rng(0, 15) if j == 1 else rng(0, 30), seq=100 * level + 20 + j)
            added.append(entry(WB, level, n, f))


def gates_tree(shape, damaged=()):
    """shape: (n_wb, n_cb) for levels 1, 2, 3.  Level 0: three overlapping
    deletion files added out of number order, and an insertion list that is not
    in key order."""
    f, added = {}, []
    f[9] = table(9, rng(3, 13), seq=40)
    f[4] = table(4, rng(20, 28), seq=41)
    f[7] = table(7, rng(8, 23), seq=42)
    f[2] = table(2, rng(15, 30), seq=30)
    f[3] = table(3, rng(0, 11), seq=31)
    added += [entry(DEL, 0, n, f) for n in (9, 4, 7)] + [entry(INS, 0, 2, f), entry(INS, 0, 3, f)]
    for level, (n_wb, n_cb) in zip((1, 2, 3), shape):
        buffer_level(f, added, level, 100 * level, n_wb, n_cb)
    return {"files": f, "damaged": sorted(damaged), "records": [{"deleted": [], "new": added}],
            "compaction_buffer_length": [0, 20, 20, 20]}


def gates_queries():
    """(start, end, snapshot): user keys of 8 bytes at least, which is what the device accepts."""
    s = 100
    q = [(k(5), k(8), s), (k(20), k(25), s), (k(26), k(28), s), (k(0), k(29), s), (k(12), k(16), s),
         (k(10), k(10), s), (k(10) + Z8, k(12), s), (k(10) + F8, k(12) + b"\x00", s), (k(12) + Z8, k(18), s),
         (k(16) + b"\x00", k(19), s), (b"kkkkj999", k(2), s), (k(300), k(400), s), (k(0), k(5), s),
         (k(11), k(14), 1000), (k(27) + Z8, k(40), s), (k(9), b"kkkkk01\x00", s)]
    return [(bytes(a), bytes(b), n) for a, b, n in q]


def gates_runs(levels=(2,)):
    runs = []
    for use in (0, 1, 2, 3, 5):
        u = [0, 2, 2, 2]
        for level in levels:
            u[level] = use
        runs.append(run(u, True, LOW, TOP))
    # read_upto_key: empty, below and above the end keys
    for upto in (b"", k(9), k(17)):
        runs.append(run((0, 3, 3, 3), True, LOW, upto))
    # the cursor: starts below, equal to and above it
    runs.append(run((0, 3, 3, 3), True, (b"", k(0), k(10), k(12)), TOP))
    runs.append(run((0, 3, 1, 3), True, (b"", b"", k(10) + Z8, TOP), TOP))
    # no warm-up walk: buffered_merge off, use_length[L-1] 0
    runs.append(run((0, 3, 3, 3), False, LOW, TOP))
    runs.append(run((0, 0, 3, 3), True, LOW, TOP))
    runs.append(run((0, 3, 0, 3), True, LOW, TOP))
    # the warm-up walk cut at 1, 2, 3 and past the list
    for use1 in (1, 2, 3, 9):
        runs.append(run((0, use1, 3, use1), True, LOW, TOP))
        runs.append(run((0, use1, use1, 0), True, LOW, TOP))
    runs.append(run((3, 1, 1, 1), True, LOW, TOP))
    return runs


def counts_tree():
    """Level 1's insertion table holds the files the count cases read; level 0's
    deletion files hold the versions of one end key; levels 2 and 3 are empty."""
    f, added = {}, []
    a = rng(0, 200, b"aaaaa")
    f[11] = table(11, a)
    long_ = [b"c" * 39 + bytes([0x40 + i]) for i in range(24)]
    f[12] = table(12, long_)
    f[13] = table(13, [k(0, b"ddddd")])
    e = rng(0, 21, b"eeeee")
    f[14] = table(14, e[:10], seq=20, extra=[(e[10], 20, 1)])
    f[15] = table(15, e[11:], seq=5, extra=[(e[10], 5, 1)])
    added += [entry(INS, 1, n, f) for n in (11, 12, 13, 14, 15)]
    end = k(100, b"bbbbb")
    side = [k(50, b"bbbbb"), k(200, b"bbbbb")]
    f[21] = table(21, side, extra=[(end, s, 1) for s in (512, 256, 255, 1)] + [(end[:7], 10, 1)])
    f[22] = table(22, side, extra=[(end, s, 1) for s in (256, 255, 1)] + [(end + b"\x00", 10, 1)])
    f[23] = table(23, side, extra=[(end, 1, 0), (end + b"\x00", 10, 1), (end + b"\x02", 10, 1)])
    f[24] = table(24, side, extra=[(end[:7], 10, 1), (end + b"\x00", 10, 1), (end + b"\x00\x00", 700, 1),
                                   (end + b"\x02", 10, 1)])
    added += [entry(DEL, 0, n, f) for n in (21, 22, 23, 24)]
    return {"files": f, "damaged": [], "records": [{"deleted": [], "new": added}],
            "compaction_buffer_length": [0, 20, 20, 3]}


def counts_queries():
    a, b, e = (lambda i: k(i, b"aaaaa")), (lambda i: k(i, b"bbbbb")), (lambda i: k(i, b"eeeee"))
    s = 1000
    q = [(a(50) + b"\x00", a(50) + b"\x01", s),  # 0 entries
         (a(50), a(50), s), (a(50), a(112), s), (a(50), a(113), s), (a(50), a(114), s), (a(10), a(139), s),
         (a(0), a(199), s), (a(190), b"aaaab000", s),  # past the file's last entry
         (a(199) + b"\x00", a(300), s),             # a start beyond the last entry
         (a(199), a(199), s), (a(0), a(0), s), (a(63), a(64), s),
         (b(0), b(100), 256), (b(0), b(100), 255), (b(0), b(100), 1000), (b(100), b(100), 256), (b(100), b(150), 256),
         (b(0), b(100)[:7] + b"\x00", 256), (b(50), b(100) + b"\x01", 256),
         (b"c" * 39 + b"\x45", b"c" * 39 + b"\x50", s), (b"c" * 39, b"c" * 40, s), (b"c" * 39 + b"\x40", b"c" * 39 + b"\x40", s),
         (k(0, b"ddddd"), k(0, b"ddddd"), s), (b"dddddddd", b"ddddddde", s),
         (e(10), e(10), s), (e(9), e(11), s), (e(10), e(10), 10), (e(0), e(20), s),
         (b"aaaaa000", b"zzzzzzzz", s), (b"zzzzzzzz", b"zzzzzzzzz", s)]
    return [(bytes(x), bytes(y), n) for x, y, n in q]


def cases():
    out = []
    t = gates_tree(((1, 1), (3, 3), (1, 0)))
    t["queries"], t["runs"] = gates_queries(), gates_runs((2,))
    out.append(("gates", t))
    t = gates_tree(((0, 3), (0, 1), (3, 3)))
    t["queries"], t["runs"] = gates_queries(), gates_runs((1, 3))
    out.append(("gates_level3", t))
    t = gates_tree(((1, 1), (3, 3), (1, 1)), damaged=(211, 301, 3))
    t["queries"] = gates_queries()
    t["runs"] = [run(u, True, LOW, TOP) for u in ((0, 2, 0, 2), (0, 2, 3, 2), (0, 3, 5, 1))]
    out.append(("damaged", t))
    t = counts_tree()
    t["queries"] = counts_queries()
    t["runs"] = [run((0, 0, 0, 0), True, LOW, b""), run((0, 2, 2, 2), True, LOW, TOP)]
    out.append(("counts", t))
    return out


def pack_case(c):
    out = struct.pack("<I", len(c["files"]))
    for number in sorted(c["files"]):
        ents = c["files"][number]
        out += struct.pack("<QI", number, len(ents)) + b"".join(pstr(a) + pstr(b) for a, b in ents)
        out += struct.pack("<I", 1 if number in c["damaged"] else 0)
    out += struct.pack("<I", len(c["records"]))
    for rec in c["records"]:
        out += struct.pack("<I", len(rec["deleted"])) + b"".join(struct.pack("<IIQ", *d) for d in rec["deleted"])
        out += struct.pack("<I", len(rec["new"]))
        for kind, level, number, a, b in rec["new"]:
            out += struct.pack("<IIQ", kind, level, number) + pstr(a) + pstr(b)
    out += struct.pack("<4I", *c["compaction_buffer_length"])
    out += struct.pack("<I", len(c["queries"]))
    out += b"".join(pstr(a) + pstr(b) + struct.pack("<Q", s) for a, b, s in c["queries"])
    out += struct.pack("<I", len(c["runs"]))
    for r in c["runs"]:
        out += struct.pack("<4II", *r["use_length"], int(r["buffered_merge"]))
        out += b"".join(pstr(x) for x in r["read_cursor_keys"]) + pstr(r["read_upto_key"])
    return out


def build_driver(tmp):
    mbf.DRIVER = DRIVER  # (the same objects, flags and link line)
    return mbf.build_driver(tmp)


def main():
    cs = cases()
    cmd = struct.pack("<I", len(cs)) + b"".join(pack_case(c) for _, c in cs)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        open(fi, "wb").write(cmd)
        subprocess.run([exe, fi, fo, tmp], check=True, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL)
        r = Reader(open(fo, "rb").read())
    pool, body, index = {}, {"files": [], "cases": {}}, {"cases": {}}

    def pooled(b):  # (the cases share most of their files)
        if b not in pool:
            pool[b] = len(body["files"])
            body["files"].append(bytes(b).hex())
        return pool[b]

    for name, c in cs:
        numbers = sorted(c["files"])
        d = {"files": {str(n): pooled(r.bytes()) for n in numbers}, "damaged": c["damaged"],
             "manifest": r.bytes().hex(), "compaction_buffer_length": c["compaction_buffer_length"],
             "records": [{"deleted": [list(x) for x in rec["deleted"]],
                          "new": [[kind, level, number, a.hex(), b.hex()] for kind, level, number, a, b in rec["new"]]}
                         for rec in c["records"]]}
        status = r.bytes().decode()
        assert status == "OK", status
        d["lists"] = {}
        for level in range(4):
            for kind in range(4):
                d["lists"]["%d,%d" % (level, kind)] = [[r.u64() for _ in range(r.u32())] for _ in range(r.u32())]
        d["queries"] = [[a.hex(), b.hex(), s] for a, b, s in c["queries"]]
        # GetRange of every query on every file, the files by ascending number
        d["file_counts"] = [[r.u32() for _ in numbers] for _ in c["queries"]]
        d["runs"] = []
        reads = 0
        for run_ in c["runs"]:
            got = []
            for _ in c["queries"]:
                found = r.u32()
                read = [r.u64() for _ in range(r.u32())]
                assert len(set(read)) == len(read), (name, read)  # each read file once
                got.append([found, read])
                reads += len(read)
            d["runs"].append({"use_length": run_["use_length"], "buffered_merge": run_["buffered_merge"],
                              "read_cursor_keys": [x.hex() for x in run_["read_cursor_keys"]],
                              "read_upto_key": run_["read_upto_key"].hex(), "results": got})
        body["cases"][name] = d
        index["cases"][name] = {"files": len(c["files"]), "runs": len(c["runs"]), "queries": len(c["queries"]),
                                "reads": reads, "entries": max(len(e) for e in c["files"].values())}
    assert r.p == len(r.buf)
    text = json.dumps(body, sort_keys=True, separators=(",", ":")).encode()
    blob = zlib.compress(text, 9)
    index["bin"] = {"inflated": len(text), "crc32": zlib.crc32(text)}
    index["source"] = ("lsbm's TableBuilder (block_size 256, restart interval 4, InternalFilterPolicy over a 10-bit "
                       "bloom), VersionEdit::EncodeTo, log::Writer, BasicVersionSet::Recover, Version::RangeQuery "
                       "and TableCache::GetRange, built from the reference; see make_range_fixture.py")
    open(os.path.join(HERE, "range_tables.bin"), "wb").write(blob)
    with open(os.path.join(HERE, "range_fixture.json"), "w") as f:
        json.dump(index, f, sort_keys=True, indent=1)
        f.write("\n")
    print(f"wrote range_fixture.json and range_tables.bin ({len(blob)} bytes, {len(text)} inflated)")


if __name__ == "__main__":
    main()
