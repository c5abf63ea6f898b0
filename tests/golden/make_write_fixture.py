"""Fixture of the reference's own write path for the GPU batched DB::Write
(include/lsbm_write.h).

    python tests/golden/make_write_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(built with -DNDEBUG), runs it over the cases of write_cases.py, and writes
tests/golden/write_fixture.json and write_fixture.bin.

BuildBatchGroup is private and its Writer struct lives in lsbm/db_impl.cc, so
the driver's translation unit includes lsbm/db_impl.cc in place of db_impl.o
(compiled with -fno-access-control).  For a write case it

  * makes every writer's batch with the reference's WriteBatch::Put / Delete,
  * queues one DBImpl::Writer per batch on an unopened DBImpl (writers_),
  * and runs the body of DBImpl::Write (lsbm/db_impl.cc:1338-1384) until the
    queue is empty: BuildBatchGroup, WriteBatchInternal::SetSequence,
    last_sequence += Count, log::Writer::AddRecord(Contents(updates)) into a
    string sink, tmp_batch_->Clear(), pop through last_writer.

Stored per group: its leader's index and the bytes of Contents(updates) -- the
reference's own Append / SetCount / SetSequence -- and per case the log file.
A log case is log::Writer over a string sink for payloads of given lengths.

Keys, values and payloads are write_cases.pattern (period 251); the driver
makes the same bytes.  write_fixture.bin is one zlib stream; the JSON holds
{offset, size} pairs into the inflated bytes and the cases' specs.  Only bytes
produced by the reference are stored; no reference source.
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

from golden import write_cases as wc  # noqa: E402

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

DRIVER = r"""
// Driver for tests/golden/make_write_fixture.py: DBImpl::Write's body over
// queued writers, and log::Writer over payloads, with the reference's classes.
#include "lsbm/db_impl.cc"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "log_writer.h"
using namespace leveldb;

static FILE *in, *out;
static uint32_t r32() { uint32_t v; if (fread(&v, 4, 1, in) != 1) exit(3); return v; }
static uint64_t r64() { uint64_t v; if (fread(&v, 8, 1, in) != 1) exit(3); return v; }
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void wstr(const std::string& s) { w32(s.size()); fwrite(s.data(), 1, s.size(), out); }
static std::string pattern(uint32_t seed, uint32_t n) {
  std::string s(n, '\0');
  for (uint32_t i = 0; i < n; i++) s[i] = (char)((seed + i) % 251);
  return s;
}

class StringSink : public WritableFile {
 public:
  std::string contents;
  virtual Status Append(const Slice& d) { contents.append(d.data(), d.size()); return Status::OK(); }
  virtual Status Close() { return Status::OK(); }
  virtual Status Flush() { return Status::OK(); }
  virtual Status Sync() { return Status::OK(); }
};

class NullLogger : public Logger {
 public:
  virtual void Logv(const char* format, va_list ap) {}
};

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  Options options;
  options.info_log = new NullLogger;
  DBImpl* db = new DBImpl(options, argv[3]);  // never opened: no file is touched
  int c;
  while ((c = fgetc(in)) != EOF) {
    if (c == 'W') {  // last_sequence, n_writers, per writer: sync, n_ops, (type, klen, kseed, vlen, vseed)*
      uint64_t last_sequence = r64();
      const uint32_t n = r32();
      std::vector<WriteBatch*> batches;
      std::vector<DBImpl::Writer*> ws;
      for (uint32_t i = 0; i < n; i++) {
        DBImpl::Writer* w = new DBImpl::Writer(&db->mutex_);
        w->sync = r32() != 0;
        w->done = false;
        WriteBatch* b = new WriteBatch;
        const uint32_t n_ops = r32();
        for (uint32_t j = 0; j < n_ops; j++) {
          const uint32_t type = r32(), klen = r32(), kseed = r32(), vlen = r32(), vseed = r32();
          if (type) b->Put(pattern(kseed, klen), pattern(vseed, vlen)); else b->Delete(pattern(kseed, klen));
        }
        w->batch = b;
        batches.push_back(b);
        ws.push_back(w);
        db->writers_.push_back(w);
      }
      StringSink log_file;
      log::Writer log(&log_file);
      std::vector<uint32_t> firsts;
      std::vector<std::string> reps;
      uint32_t at = 0;
      while (!db->writers_.empty()) {
        DBImpl::Writer* last_writer = db->writers_.front();
        WriteBatch* updates = db->BuildBatchGroup(&last_writer);
        WriteBatchInternal::SetSequence(updates, last_sequence + 1);
        last_sequence += WriteBatchInternal::Count(updates);
        if (!log.AddRecord(WriteBatchInternal::Contents(updates)).ok()) exit(4);
        firsts.push_back(at);
        reps.push_back(WriteBatchInternal::Contents(updates).ToString());
        if (updates == db->tmp_batch_) db->tmp_batch_->Clear();
        while (true) {
          DBImpl::Writer* ready = db->writers_.front();
          db->writers_.pop_front();
          at++;
          if (ready == last_writer) break;
        }
      }
      if (at != n) exit(5);
      w32(firsts.size());
      for (size_t g = 0; g < firsts.size(); g++) {
        w32(firsts[g]);
        wstr(reps[g]);
      }
      fwrite(&last_sequence, 8, 1, out);
      wstr(log_file.contents);
      for (uint32_t i = 0; i < n; i++) {
        delete batches[i];
        delete ws[i];
      }
    } else if (c == 'L') {  // n, (length, seed)*
      const uint32_t n = r32();
      StringSink log_file;
      log::Writer log(&log_file);
      for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = r32(), seed = r32();
        if (!log.AddRecord(pattern(seed, len)).ok()) exit(4);
      }
      wstr(log_file.contents);
    } else {
      exit(10);
    }
  }
  fclose(out);
  _exit(0);  // (the unopened DBImpl is not torn down)
}
"""


def build_driver(tmp):
    if not os.path.isdir(OBJ):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "dbbench"], check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*", "*.o")))
            if not o.endswith("lsbm/db_bench.o") and not o.endswith("lsbm/db_impl.o")]
    src = os.path.join(tmp, "write_driver.cc")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "write_driver")
    subprocess.run(["g++", "-std=c++11", "-w", "-O2", "-pthread", "-fno-access-control", "-DNDEBUG", "-DOS_LINUX",
                    "-DLEVELDB_PLATFORM_POSIX", "-I" + REF, "-I" + REF + "/include", "-I" + REF + "/common",
                    "-I" + REF + "/lsbm", "-o", exe, src] + objs, check=True)
    return exe


def p32(v):
    return struct.pack("<I", v)


def main():
    tmp = tempfile.mkdtemp(prefix="lsbm_writefx_")
    exe = build_driver(tmp)
    writes, logs = wc.write_specs(), wc.log_specs()
    cmds = []
    for _, last_sequence, writers in writes:
        cmd = b"W" + struct.pack("<Q", last_sequence) + p32(len(writers))
        for sync, ops in writers:
            cmd += p32(sync) + p32(len(ops)) + b"".join(b"".join(p32(x) for x in op) for op in ops)
        cmds.append(cmd)
    for _, payloads in logs:
        cmds.append(b"L" + p32(len(payloads)) + b"".join(p32(n) + p32(s) for n, s in payloads))
    fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(fi, "wb").write(b"".join(cmds))
    subprocess.run([exe, fi, fo, os.path.join(tmp, "db")], check=True)
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

    blob = bytearray()

    def keep(b):
        blob.extend(b)
        return [len(blob) - len(b), len(b)]

    wrecs, lrecs = [], []
    for name, last_sequence, writers in writes:
        firsts, reps = [], []
        for _ in range(u32()):
            firsts.append(u32())
            reps.append(keep(s()))
        new_last = struct.unpack_from("<Q", buf, p)[0]
        p += 8
        wrecs.append({"name": name, "last_sequence": last_sequence, "writers": writers,
                      "group_first": firsts + [len(writers)], "reps": reps, "new_last_sequence": new_last,
                      "log": keep(s())})
    for name, payloads in logs:
        lrecs.append({"name": name, "payloads": payloads, "log": keep(s())})
    assert p == len(buf)
    fx = {"source": "lsbm's WriteBatch::Put / Delete, DBImpl::BuildBatchGroup (lsbm/db_impl.cc compiled as the "
                    "driver's translation unit, Writers queued on an unopened DBImpl), WriteBatchInternal::Append / "
                    "SetSequence / Contents and log::Writer::AddRecord over a string sink, linked with the "
                    "reference's objects (oracle/Makefile dbbench, -DNDEBUG); write_fixture.bin is one zlib stream, "
                    "{offset, size} pairs index its inflated bytes; keys, values and payloads are "
                    "write_cases.pattern(seed, length)",
          "inflated_bytes": len(blob), "writes": wrecs, "logs": lrecs}
    packed = zlib.compress(bytes(blob), 9)
    open(os.path.join(HERE, "write_fixture.bin"), "wb").write(packed)
    json.dump(fx, open(os.path.join(HERE, "write_fixture.json"), "w"), indent=0)
    print(f"{len(wrecs)} write cases ({sum(len(w['reps']) for w in wrecs)} groups), {len(lrecs)} log cases "
          f"({len(blob)} B inflated, {len(packed)} B stored)")


if __name__ == "__main__":
    sys.exit(main())
