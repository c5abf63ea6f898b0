"""Fixture of the reference's own memtable accounting for the GPU memtable
switch (include/lsbm_memtable_cut.h).

    python tests/golden/make_memcut_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(built with -DNDEBUG; everything but db_bench's main), runs it on the
scenarios of memcut_cases.py, and writes tests/golden/memcut_fixture.json (the
index) and memcut_fixture.bin (one zlib stream of JSON text).

The driver uses the reference's MemTable, WriteBatch::Iterate,
WriteBatchInternal::InsertInto and Random.  It restates two loops only:
RecoverLogFile's (lsbm/db_impl.cc:438-473: records under 12 bytes dropped, a
memtable made when there is none, InsertInto with its status ignored, the test
after it) and MakeRoomForWrite's test before a record (:1470), and SkipList's
RandomHeight loop over the reference's Random (the listed heights, and the
index of the first insert of height 12 from the fixed seed with the draws up
to its end).  Per scenario it records, per
record, the entries WriteBatch::Iterate hands out (key length, value length,
type) and its status; per write_buffer_size and mode,
ApproximateMemoryUsage() after every record, the first record of every
memtable and the usage each ended with.

Only numbers produced by the reference are stored; no reference source.
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

from golden import memcut_cases as cases  # noqa: E402

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

DRIVER = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "common/dbformat.h"
#include "common/memtable.h"
#include "common/write_batch_internal.h"
#include "leveldb/comparator.h"
#include "leveldb/write_batch.h"
#include "util/random.h"

using namespace leveldb;

static FILE* out;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void w64(uint64_t v) { fwrite(&v, 8, 1, out); }
static uint32_t r32(FILE* f) { uint32_t v; if (fread(&v, 4, 1, f) != 1) exit(3); return v; }
static uint64_t r64(FILE* f) { uint64_t v; if (fread(&v, 8, 1, f) != 1) exit(3); return v; }

struct Lister : public WriteBatch::Handler {
  std::vector<uint32_t> v;
  virtual void Put(const Slice& key, const Slice& value) { v.push_back(key.size()); v.push_back(value.size()); v.push_back(1); }
  virtual void Delete(const Slice& key) { v.push_back(key.size()); v.push_back(0); v.push_back(0); }
};

static uint32_t code_of(const Status& s) {
  if (s.ok()) return 0;
  const std::string m = s.ToString();
  if (m.find("bad WriteBatch Put") != std::string::npos) return 2;
  if (m.find("bad WriteBatch Delete") != std::string::npos) return 3;
  if (m.find("unknown WriteBatch tag") != std::string::npos) return 4;
  if (m.find("wrong count") != std::string::npos) return 5;
  exit(4);
}

// mode 0: RecoverLogFile's loop; mode 1: MakeRoomForWrite's test before every record
static void run(const std::vector<std::string>& recs, uint64_t wbs, int mode) {
  InternalKeyComparator cmp(BytewiseComparator());
  MemTable* mem = NULL;
  uint64_t last = 0;
  std::vector<uint64_t> usage, first, ended;
  WriteBatch batch;
  for (size_t i = 0; i < recs.size(); i++) {
    if (mode == 0) {
      if (recs[i].size() < 12) { usage.push_back(last); continue; }
    } else if (mem != NULL && mem->ApproximateMemoryUsage() > wbs) {
      ended.push_back(mem->ApproximateMemoryUsage());
      mem->Unref();
      mem = NULL;
    }
    if (mem == NULL) {
      mem = new MemTable(cmp);
      mem->Ref();
      first.push_back(i);
    }
    WriteBatchInternal::SetContents(&batch, recs[i].size() < 12 ? std::string(12, '\0') : recs[i]);
    WriteBatchInternal::InsertInto(&batch, mem);
    last = mem->ApproximateMemoryUsage();
    usage.push_back(last);
    if (mode == 0 && last > wbs) {
      ended.push_back(last);
      mem->Unref();
      mem = NULL;
      last = 0;  // what a dropped record reports while there is no memtable
    }
  }
  if (mem != NULL) { ended.push_back(mem->ApproximateMemoryUsage()); mem->Unref(); }
  for (size_t i = 0; i < usage.size(); i++) w64(usage[i]);
  w32(first.size());
  for (size_t i = 0; i < first.size(); i++) w64(first[i]);
  for (size_t i = 0; i < ended.size(); i++) w64(ended[i]);
  w32(mem != NULL);
}

static void heights(uint32_t skip, uint32_t n) {  // SkipList::RandomHeight after `skip` draws
  Random rnd(0xdeadbeef);
  uint32_t state = 0xdeadbeef & 0x7fffffffu;
  for (uint32_t i = 0; i < skip; i++) state = rnd.Next();
  w32(state);
  for (uint32_t i = 0; i < n; i++) {
    int height = 1;
    while (height < 12 && ((state = rnd.Next()) % 4) == 0) height++;
    w32(height);
  }
  w32(state);
}

// the first insert of height 12 from the fixed seed: its 0-based index and the draws up to its end
static void first_height_12() {
  Random rnd(0xdeadbeef);
  uint64_t insert = 0, draws = 0;
  for (;; insert++) {
    int height = 1;
    while (height < 12 && (draws++, rnd.Next() % 4) == 0) height++;
    if (height == 12) break;
  }
  w64(insert);
  w64(draws);
}

int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const uint32_t n_heights = r32(in);
  for (uint32_t i = 0; i < n_heights; i++) { const uint32_t skip = r32(in), n = r32(in); heights(skip, n); }
  first_height_12();
  const uint32_t n_scen = r32(in);
  for (uint32_t s = 0; s < n_scen; s++) {
    const uint32_t n = r32(in);
    std::vector<std::string> recs(n);
    for (uint32_t i = 0; i < n; i++) {
      recs[i].resize(r32(in));
      if (recs[i].size() && fread(&recs[i][0], 1, recs[i].size(), in) != recs[i].size()) return 3;
    }
    for (uint32_t i = 0; i < n; i++) {
      Lister l;
      uint32_t code = 1;
      if (recs[i].size() >= 12) {
        WriteBatch b;
        WriteBatchInternal::SetContents(&b, recs[i]);
        code = code_of(b.Iterate(&l));
      }
      w32(code);
      w32(l.v.size() / 3);
      for (size_t k = 0; k < l.v.size(); k++) w32(l.v[k]);
    }
    const uint32_t n_wbs = r32(in);
    for (uint32_t k = 0; k < n_wbs; k++) {
      const uint64_t wbs = r64(in);
      run(recs, wbs, 0);
      run(recs, wbs, 1);
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
    flags = ["-std=c++11", "-w", "-O2", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX", "-I" + REF,
             "-I" + REF + "/include", "-I" + REF + "/common"]
    src, exe = os.path.join(tmp, "memcut_driver.cc"), os.path.join(tmp, "memcut_driver")
    open(src, "w").write(DRIVER)
    subprocess.run(["g++"] + flags + ["-o", exe, src] + objs, check=True)
    return exe


class Reader:
    def __init__(self, buf):
        self.buf, self.p = buf, 0

    def u32(self):
        self.p += 4
        return struct.unpack_from("<I", self.buf, self.p - 4)[0]

    def u64(self):
        self.p += 8
        return struct.unpack_from("<Q", self.buf, self.p - 8)[0]


def main():
    scen = cases.scenarios()
    height_runs = [("first_2000", 0, 2000), ("height_12", cases.HEIGHT12_DRAW - 50, 200)]
    cmd = struct.pack("<I", len(height_runs)) + b"".join(struct.pack("<II", s, n) for _, s, n in height_runs)
    cmd += struct.pack("<I", len(scen))
    for _, reps in scen:
        cmd += struct.pack("<I", len(reps)) + b"".join(struct.pack("<I", len(r)) + r for r in reps)
        cmd += struct.pack("<I", len(cases.WRITE_BUFFER_SIZES))
        cmd += b"".join(struct.pack("<Q", w) for w in cases.WRITE_BUFFER_SIZES)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        open(fi, "wb").write(cmd)
        subprocess.run([exe, fi, fo], check=True)
        r = Reader(open(fo, "rb").read())
    body, index = {"heights": {}, "scenarios": {}}, {"heights": {}, "scenarios": {}}
    for name, skip, n in height_runs:
        rnd = r.u32()
        hs = [r.u32() for _ in range(n)]
        body["heights"][name] = {"draws_before": skip, "rnd": rnd, "heights": hs, "rnd_after": r.u32()}
        index["heights"][name] = {"n": n, "max": max(hs)}
    first12 = {"insert": r.u64(), "draws": r.u64()}
    body["first_height_12"] = index["first_height_12"] = first12
    for name, reps in scen:
        status, ops = [], []
        for _ in reps:
            status.append(r.u32())
            ops.append([[r.u32(), r.u32(), r.u32()] for _ in range(r.u32())])
        cuts = {}
        for w in cases.WRITE_BUFFER_SIZES:
            for mode in ("recover", "write"):
                usage = [r.u64() for _ in reps]
                n_mem = r.u32()
                first = [r.u64() for _ in range(n_mem)]
                # every memtable either ended inside the loop or is measured after it: one usage each
                ended = [r.u64() for _ in range(n_mem)]
                cuts[f"{mode}_{w}"] = {"usage": usage, "mem_first": first, "ended": ended, "open_at_end": r.u32()}
        body["scenarios"][name] = {"status": status, "ops": ops, "cuts": cuts}
        index["scenarios"][name] = {"records": len(reps), "entries": sum(len(o) for o in ops),
                                    "memtables": {k: len(v["mem_first"]) for k, v in cuts.items()}}
    assert r.p == len(r.buf)
    text = json.dumps(body, sort_keys=True, separators=(",", ":")).encode()
    blob = zlib.compress(text, 9)
    index["bin"] = {"inflated": len(text), "crc32": zlib.crc32(text)}
    index["write_buffer_sizes"] = list(cases.WRITE_BUFFER_SIZES)
    open(os.path.join(HERE, "memcut_fixture.bin"), "wb").write(blob)
    with open(os.path.join(HERE, "memcut_fixture.json"), "w") as f:
        json.dump(index, f, sort_keys=True, indent=1)
        f.write("\n")
    print(f"wrote memcut_fixture.json and memcut_fixture.bin ({len(blob)} bytes, {len(text)} inflated)")


if __name__ == "__main__":
    main()
