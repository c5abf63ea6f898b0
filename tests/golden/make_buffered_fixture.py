"""Fixture of the reference's own Builder::SaveTo and Version::Get over the
sorted-table lists, for the GPU's buffered Get (include/lsbm_probe.h,
lsbm_amd/buffered.py).

    python tests/golden/make_buffered_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(built with -DNDEBUG; everything but db_bench's main), runs it on the cases
below, and writes tests/golden/buffered_fixture.json (the index) and
buffered_tables.bin (one zlib stream of JSON text).

Per case the driver writes small table files with TableBuilder (block_size
256, restart interval 4, a 10-bit bloom under InternalFilterPolicy; every value
names its file number), damages the index block of the files the case names
(the restart count, the trailer's CRC set right again), writes a MANIFEST with
VersionEdit::EncodeTo and log::Writer plus CURRENT, sets
runtime::compaction_buffer_length[], runs BasicVersionSet::Recover() with a
real TableCache and records the recovered version's lists: per (level, type)
the file numbers of every sorted table in list order.  Per run of a case it
then sets `visible` on the named files, runtime::compaction_buffer_use_length[],
config::buffered_merge and runtime::read_cursor_key_[], calls the recovered
version's Get(ReadOptions(), LookupKey(k, s), &value) for every query and
records Status::ToString() and the value.

Only bytes and results the reference produced are stored, beside the cases'
own description; no reference source.
"""
import glob
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

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

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

// the index block's restart count becomes 0xffffffff (Block's constructor then
// sets size_ = 0: "bad block contents"), and the trailer's CRC is set right again
static void damage_index(std::string* file) {
  Footer footer;
  Slice tail(file->data() + file->size() - Footer::kEncodedLength, Footer::kEncodedLength);
  if (!footer.DecodeFrom(&tail).ok()) exit(8);
  const uint64_t off = footer.index_handle().offset(), n = footer.index_handle().size();
  memset(&(*file)[off + n - 4], 0xff, 4);
  const uint32_t crc = crc32c::Value(file->data() + off, n + 1);
  EncodeFixed32(&(*file)[off + n + 1], crc32c::Mask(crc));
}

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const std::string dir = argv[3];
  if (!in || !out) return 2;
  Env* env = Env::Default();
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
    TableCache* cache = new TableCache(db, &options, 1000);
    BasicVersionSet* vs = new BasicVersionSet(db, &options, cache, &icmp);  // (never deleted: its destructor asserts)
    const Status s = vs->Recover();
    wstr(s.ToString());
    if (!s.ok()) return 5;
    Version* v = vs->current();
    std::vector<FileMetaData*> all;
    for (int level = 0; level < config::kNumLevels; level++) {
      for (int type = 0; type < 4; type++) {
        SortedTable* head = v->levels_[level][type];
        uint32_t n_tables = 0;
        SortedTable* cur = head;
        do { n_tables++; cur = cur->next; } while (cur != head);
        w32(n_tables);
        do {
          w32(cur->files_.size());
          for (size_t i = 0; i < cur->files_.size(); i++) {
            w64(cur->files_[i]->number);
            all.push_back(cur->files_[i]);
          }
          cur = cur->next;
        } while (cur != head);
      }
    }
    const uint32_t n_runs = r32();
    for (uint32_t r = 0; r < n_runs; r++) {
      for (int i = 0; i < 4; i++) runtime::compaction_buffer_use_length[i] = (int)r32();
      config::buffered_merge = r32() != 0;
      for (int i = 0; i < 4; i++) runtime::read_cursor_key_[i] = rstr();
      for (size_t i = 0; i < all.size(); i++) all[i]->visible = true;
      const uint32_t n_inv = r32();
      for (uint32_t k = 0; k < n_inv; k++) {
        const uint32_t level = r32(), type = r32();
        const uint64_t number = r64();
        SortedTable* head = v->levels_[level][type];
        SortedTable* cur = head;
        do {
          for (size_t i = 0; i < cur->files_.size(); i++)
            if (cur->files_[i]->number == number) cur->files_[i]->visible = false;
          cur = cur->next;
        } while (cur != head);
      }
      const uint32_t nq = r32();
      for (uint32_t q = 0; q < nq; q++) {
        const std::string user = rstr();
        LookupKey lk(user, r64());
        std::string value;
        const Status gs = v->Get(ReadOptions(), lk, &value);
        wstr(gs.ToString());
        wstr(gs.ok() ? value : std::string());
      }
    }
  }
  fclose(out);
  return 0;
}
"""

TYPE_DELETION, TYPE_VALUE = 0, 1
DEL, INS, CB, WB = 0, 1, 2, 3


def ikey(user, seq, kind=TYPE_VALUE):
    return bytes(user) + struct.pack("<Q", (seq << 8) | kind)


def k(i, prefix=b"k"):
    return prefix + b"%02d" % i


def table(number, users, seq=10, without=(), extra=()):
    """A file's entries [(internal key, value)], sorted: every user key of
    `users` but those in `without` as a value naming the file, plus `extra`
    [(user, seq, type)] entries."""
    ents = [(u, seq, TYPE_VALUE) for u in users if u not in without] + list(extra)
    ents.sort(key=lambda e: (e[0], -e[1], -e[2]))
    return [(ikey(u, s, t), (b"f%d:" % number + u + b"@%d" % s) if t == TYPE_VALUE else b"") for u, s, t in ents]


def entry(kind, level, number, files, bounds=None):
    """An added entry (type, level, number, smallest, largest): the bounds are
    the file's first and last key unless given as user keys."""
    if bounds is None:
        return (kind, level, number, files[number][0][0], files[number][-1][0])
    return (kind, level, number, ikey(bounds[0], 100), ikey(bounds[1], 1))


def run(use, merge, cursors, queries, invisible=()):
    return {"use_length": list(use), "buffered_merge": bool(merge), "read_cursor_keys": [bytes(c) for c in cursors],
            "invisible": [list(i) for i in invisible], "queries": [(bytes(u), s) for u, s in queries]}


ALL = [k(i) for i in range(30)]
NO_CURSOR = (b"", b"", b"", b"")


def gates_tree(damaged=()):
    """Level 2 holds the key range k00..k29 in WB (w1, w2, w3), DEL (d1), the
    compaction buffer (c1..c4, c4 the head) and INS (i1); the values name the
    files.  Level 3 holds every key once more (the answer when level 2 passes),
    level 1 another key range (a00..a29) with a warm-up list level 1 never
    reads, level 0 three overlapping deletion files added out of number order
    and one insertion file."""
    f = {}
    # k05 everywhere; k06 not in WB; k07 not in WB, DEL, HEAD; k08 in c2 and INS; k09 in c1 and INS; k10 in INS;
    # k11 in DEL only; k12 in WB, HEAD and INS and inside DEL's range; k14 in w1, k15 in w2 beside DEL and INS;
    # k13: a deletion marker and values at different sequences; k16 in c3 and INS (c3 is what a run hides)
    f[21] = table(21, ALL, without={k(6), k(7), k(8), k(9), k(10), k(11), k(15), k(16)})                 # w1
    f[22] = table(22, ALL, without={k(6), k(7), k(8), k(9), k(10), k(11), k(14), k(16)})                 # w2
    f[23] = table(23, ALL, without={k(6), k(7), k(8), k(9), k(10), k(11), k(14), k(15), k(16)})          # w3
    f[31] = table(31, ALL, without={k(7), k(8), k(9), k(10), k(12), k(13), k(16)})                       # d1
    f[41] = table(41, ALL, without={k(7), k(8), k(10), k(11), k(12), k(13), k(14), k(15), k(16)})        # c1
    f[42] = table(42, ALL, without={k(7), k(9), k(10), k(11), k(12), k(13), k(14), k(15), k(16)})        # c2
    f[43] = table(43, ALL, without={k(8), k(9), k(10), k(11), k(12), k(13), k(14), k(15)})               # c3
    f[44] = table(44, ALL, without={k(7), k(8), k(9), k(10), k(11), k(14), k(15), k(16)},
                  extra=[(k(13), 60, TYPE_VALUE)])                                                       # c4, the head
    f[51] = table(51, ALL, without={k(11), k(13)}, extra=[(k(13), 50, TYPE_DELETION), (k(13), 30, TYPE_VALUE)])  # i1
    f[61] = table(61, ALL, seq=5)                                                                        # level 3 INS
    f[62] = table(62, [k(i) for i in range(0, 30, 3)], seq=6)                                            # level 3 DEL
    a = [k(i, b"a") for i in range(30)]
    f[11] = table(11, a, seq=20)                                                                         # level 1 INS
    f[12] = table(12, a[:10], seq=21)                                                                    # level 1 DEL
    f[13] = table(13, a, seq=22, without={a[3]})                                                         # level 1 cb
    f[14] = table(14, a + [b"zz"], seq=23)                                                               # level 1 wb
    z = [k(i, b"z") for i in range(30)]
    f[9] = table(9, z[:20], seq=40)
    f[4] = table(4, z[10:], seq=41, extra=[(z[12], 45, TYPE_DELETION)])
    f[7] = table(7, z[5:25], seq=42, without={z[12]})
    f[2] = table(2, z + [b"zz"], seq=30)
    added = [entry(DEL, 0, n, f) for n in (9, 4, 7)] + [entry(INS, 0, 2, f)]
    added += [entry(DEL, 1, 12, f), entry(INS, 1, 11, f), entry(CB, 1, 13, f), entry(WB, 1, 14, f)]
    added += [entry(DEL, 2, 31, f), entry(INS, 2, 51, f)]
    added += [entry(CB, 2, n, f) for n in (41, 42, 43, 44)] + [entry(WB, 2, n, f) for n in (21, 22, 23)]
    added += [entry(DEL, 3, 62, f), entry(INS, 3, 61, f)]
    return {"files": f, "damaged": sorted(damaged), "records": [{"deleted": [], "new": added}],
            "compaction_buffer_length": [0, 20, 20, 3]}


def gates_queries():
    q = [(k(i), 100) for i in range(5, 17)] + [(k(13), s) for s in (20, 40, 55, 70)]
    q += [(b"k", 100), (b"k30", 100), (b"a03", 100), (b"a05", 100), (b"zz", 100), (b"z12", 100), (b"z12", 43),
          (b"z07", 100), (b"z22", 100), (b"z00", 100), (b"nothing", 100), (b"", 100)]
    return q


def gates_runs():
    runs = []
    low, high = (b"", b"", b"", b""), (b"", b"", b"zzzz", b"")
    for use2 in (0, 1, 2, 3, 5, 10):
        for cursors in (low, high):
            runs.append(run((0, 2, use2, 0), True, cursors, gates_queries()))
    # the cursor itself: keys either side of it and equal to it
    runs.append(run((0, 2, 0, 0), True, (b"", b"", k(12), b""), gates_queries()))
    runs.append(run((0, 2, 1, 0), True, (b"", b"zz", k(5) + b"\x00", b"\xff"), gates_queries()))
    # no warm-up walk: use_length[L-1] = 0, buffered_merge off
    runs.append(run((0, 0, 0, 0), True, low, gates_queries()))
    runs.append(run((0, 0, 3, 0), True, low, gates_queries()))
    runs.append(run((0, 2, 0, 0), False, low, gates_queries()))
    runs.append(run((0, 2, 3, 0), False, low, gates_queries()))
    # the warm-up walk cut at 1, 2 and past the list (the sentinel last)
    for use1 in (1, 2, 3, 9):
        runs.append(run((0, use1, 0, 0), True, low, gates_queries()))
        runs.append(run((0, use1, 2, 0), True, low, gates_queries()))
    # level 1's own buffer, and level 3's use lengths
    runs.append(run((0, 3, 4, 2), True, low, gates_queries()))
    runs.append(run((3, 1, 1, 1), True, low, gates_queries()))
    # invisible files: skipped in WB and REST, still read as HEAD
    hidden = [(2, WB, 23), (2, CB, 43), (2, CB, 44)]
    for use in ((0, 2, 0, 0), (0, 2, 1, 0), (0, 2, 5, 0)):
        runs.append(run(use, True, low, gates_queries(), hidden))
    runs.append(run((0, 1, 5, 0), True, low, gates_queries(), [(2, WB, 22), (2, CB, 42), (2, DEL, 31), (2, INS, 51)]))
    return runs


def lists_case():
    """Added orders that exercise the split at :1743, the empty head rule and
    the eviction."""
    f = {}
    rng = lambda lo, hi, p=b"k": [k(i, p) for i in range(lo, hi)]
    added, deleted = [], []
    # level 1 INS: A, a dead X whose largest key makes B split off, though A and B do not overlap
    f[101] = table(101, rng(0, 10))
    f[102] = table(102, rng(15, 19))
    added += [entry(INS, 1, 101, f), entry(INS, 1, 190, f, (k(20), k(29))), entry(INS, 1, 102, f)]
    deleted.append((INS, 1, 190))
    # level 1 DEL: A, a dead X below it (a split into a head that stays empty), then B above X: no second split
    f[111] = table(111, rng(10, 20))
    f[112] = table(112, rng(5, 9))
    added += [entry(DEL, 1, 111, f), entry(DEL, 1, 191, f, (k(0), k(2))), entry(DEL, 1, 112, f)]
    deleted.append((DEL, 1, 191))
    # level 2 CB: A, a dead X below it, B below X: an empty table in the middle of the list
    f[121] = table(121, rng(10, 20))
    f[122] = table(122, rng(1, 4) + rng(10, 20))
    added += [entry(CB, 2, 121, f), entry(CB, 2, 192, f, (k(0), k(2))), entry(CB, 2, 122, f)]
    deleted.append((CB, 2, 192))
    f[123] = table(123, rng(0, 25))
    f[124] = table(124, rng(0, 25))
    added += [entry(INS, 2, 123, f), entry(DEL, 2, 124, f)]
    # level 2 WB: only dead entries: tables that are all empty
    added += [entry(WB, 2, 193, f, (k(0), k(9))), entry(WB, 2, 194, f, (k(0), k(9)))]
    deleted += [(WB, 2, 193), (WB, 2, 194)]
    # level 3 CB: six overlapping tables with compaction_buffer_length 3: the tail is evicted; two files in one table
    for i in range(6):
        f[131 + i] = table(131 + i, rng(0, 12, b"m"), seq=10 + i, without={k(j, b"m") for j in range(i)})
    f[137] = table(137, rng(15, 25, b"m"), seq=17)
    added += [entry(CB, 3, 131 + i, f) for i in range(6)] + [entry(CB, 3, 137, f)]
    f[138] = table(138, rng(0, 25, b"m"), seq=3)
    added += [entry(INS, 3, 138, f)]
    # level 3 WB: the same for the warm-up list (no eviction)
    for i in range(5):
        f[141 + i] = table(141 + i, rng(0, 12, b"m"), seq=30 + i, without={k(j, b"m") for j in range(4 - i)})
    added += [entry(WB, 3, 141 + i, f) for i in range(5)]
    # level 0: added order kept, numbers out of order; the insertion part is not sorted either
    for n, lo, hi in ((155, 0, 20), (151, 10, 30), (153, 5, 25)):
        f[n] = table(n, rng(lo, hi, b"z"), seq=n)
    f[160] = table(160, rng(0, 10, b"y"))
    f[161] = table(161, rng(10, 20, b"y"))
    added += [entry(DEL, 0, n, f) for n in (155, 151, 153)] + [entry(INS, 0, 160, f), entry(INS, 0, 161, f)]
    q = [(k(i), 100) for i in range(0, 26)] + [(k(i, b"m"), 100) for i in range(0, 26)] + \
        [(k(i, b"z"), 100) for i in range(0, 30, 3)] + [(k(i, b"y"), 100) for i in range(0, 20, 3)]
    runs = [run(use, merge, NO_CURSOR, q) for use, merge in (
        ((0, 0, 0, 0), True), ((0, 1, 1, 1), True), ((0, 2, 2, 2), True), ((0, 3, 3, 3), True), ((0, 3, 4, 4), True),
        ((0, 9, 9, 9), True), ((0, 3, 9, 0), True), ((0, 9, 9, 9), False))]
    return {"files": f, "damaged": [], "records": [{"deleted": [], "new": added}, {"deleted": deleted, "new": []}],
            "compaction_buffer_length": [0, 20, 20, 3], "runs": runs}


def empty_buffers_case():
    """No buffer entries at all: the tree Version.for_levels describes."""
    t = gates_tree()
    new = [e for e in t["records"][0]["new"] if e[0] in (DEL, INS)]
    numbers = {e[2] for e in new}
    t["files"] = {n: ents for n, ents in t["files"].items() if n in numbers}
    t["records"] = [{"deleted": [], "new": new}]
    t["runs"] = [run(use, merge, NO_CURSOR, gates_queries()) for use, merge in (((0, 0, 0, 0), True),
                                                                               ((0, 20, 20, 0), True),
                                                                               ((0, 0, 0, 0), False))]
    return t


def cases():
    out = []
    t = gates_tree()
    t["runs"] = gates_runs()
    out.append(("gates", t))
    low = NO_CURSOR
    # a walk slot with a damaged index: an error when the walk reaches it, nothing when an earlier slot decides
    t = gates_tree(damaged=(43, 22))
    t["runs"] = [run(use, True, low, gates_queries()) for use in ((0, 2, 0, 0), (0, 2, 1, 0), (0, 2, 2, 0),
                                                                  (0, 2, 3, 0), (0, 0, 3, 0), (0, 1, 5, 0))]
    out.append(("damaged_walk", t))
    # the same damage in the gates: a plain miss
    for name, numbers in (("damaged_ins", (51,)), ("damaged_del", (31,)), ("damaged_head", (44,)),
                          ("damaged_level0", (7, 2))):
        t = gates_tree(damaged=numbers)
        t["runs"] = [run(use, True, low, gates_queries()) for use in ((0, 2, 0, 0), (0, 2, 1, 0), (0, 2, 5, 0))]
        out.append((name, t))
    out.append(("lists", lists_case()))
    out.append(("empty_buffers", empty_buffers_case()))
    return out


def build_driver(tmp):
    if not os.path.isdir(OBJ):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "dbbench"], check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*", "*.o"))) if not o.endswith("lsbm/db_bench.o")]
    flags = ["-std=c++11", "-w", "-O2", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX", "-I" + REF,
             "-I" + REF + "/include", "-I" + REF + "/common"]
    src, exe = os.path.join(tmp, "buffered_driver.cc"), os.path.join(tmp, "buffered_driver")
    open(src, "w").write(DRIVER)
    subprocess.run(["g++"] + flags + ["-o", exe, src] + objs, check=True)
    return exe


def pstr(b):
    return struct.pack("<I", len(b)) + bytes(b)


class Reader:
    def __init__(self, buf):
        self.buf, self.p = buf, 0

    def u32(self):
        self.p += 4
        return struct.unpack_from("<I", self.buf, self.p - 4)[0]

    def u64(self):
        self.p += 8
        return struct.unpack_from("<Q", self.buf, self.p - 8)[0]

    def bytes(self):
        n = self.u32()
        self.p += n
        return self.buf[self.p - n:self.p]


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
    out += struct.pack("<I", len(c["runs"]))
    for r in c["runs"]:
        out += struct.pack("<4II", *r["use_length"], int(r["buffered_merge"]))
        out += b"".join(pstr(x) for x in r["read_cursor_keys"])
        out += struct.pack("<I", len(r["invisible"])) + b"".join(struct.pack("<IIQ", *i) for i in r["invisible"])
        out += struct.pack("<I", len(r["queries"])) + b"".join(pstr(u) + struct.pack("<Q", s) for u, s in r["queries"])
    return out


def main():
    cs = cases()
    cmd = struct.pack("<I", len(cs)) + b"".join(pack_case(c) for _, c in cs)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        open(fi, "wb").write(cmd)
        subprocess.run([exe, fi, fo, tmp], check=True, stderr=subprocess.DEVNULL)
        r = Reader(open(fo, "rb").read())
    pool, body, index = {}, {"files": [], "cases": {}}, {"cases": {}}

    def pooled(b):  # (the cases share most of their files)
        if b not in pool:
            pool[b] = len(body["files"])
            body["files"].append(bytes(b).hex())
        return pool[b]

    for name, c in cs:
        d = {"files": {str(n): pooled(r.bytes()) for n in sorted(c["files"])}, "damaged": c["damaged"],
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
        d["runs"], statuses = [], {}
        for run_ in c["runs"]:
            got = []
            for _ in run_["queries"]:
                status, value = r.bytes().decode("latin-1"), r.bytes().decode("latin-1")
                got.append([status, value])
                statuses[status] = statuses.get(status, 0) + 1
            d["runs"].append({"use_length": run_["use_length"], "buffered_merge": run_["buffered_merge"],
                              "read_cursor_keys": [x.hex() for x in run_["read_cursor_keys"]],
                              "invisible": run_["invisible"],
                              "queries": [[u.hex(), s] for u, s in run_["queries"]], "results": got})
        body["cases"][name] = d
        index["cases"][name] = {"files": len(c["files"]), "runs": len(c["runs"]),
                                "queries": sum(len(x["queries"]) for x in c["runs"]), "statuses": statuses}
    assert r.p == len(r.buf)
    text = json.dumps(body, sort_keys=True, separators=(",", ":")).encode()
    blob = zlib.compress(text, 9)
    index["bin"] = {"inflated": len(text), "crc32": zlib.crc32(text)}
    index["source"] = ("lsbm's TableBuilder (block_size 256, restart interval 4, InternalFilterPolicy over a 10-bit "
                       "bloom), VersionEdit::EncodeTo, log::Writer, BasicVersionSet::Recover and Version::Get, built "
                       "from the reference; see make_buffered_fixture.py")
    open(os.path.join(HERE, "buffered_tables.bin"), "wb").write(blob)
    with open(os.path.join(HERE, "buffered_fixture.json"), "w") as f:
        json.dump(index, f, sort_keys=True, indent=1)
        f.write("\n")
    print(f"wrote buffered_fixture.json and buffered_tables.bin ({len(blob)} bytes, {len(text)} inflated)")


if __name__ == "__main__":
    main()
