"""Fixture of the reference's own log -> memtable -> Level-0 table results for
the GPU memtable flush (include/lsbm_memtable.h).

    python tests/golden/make_memtable_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(built with -DNDEBUG; everything but db_bench's main), runs it, and writes
tests/golden/memtable_fixture.json and memtable_tables.bin.  For every case
the driver

  * makes the batches with the reference's WriteBatch::Put / Delete and
    WriteBatchInternal::SetSequence,
  * writes them to a log file with its log::Writer (a string sink),
  * reads the records back with its log::Reader (checksums on),
  * puts each into its MemTable with WriteBatchInternal::InsertInto,
  * records key() / value() of MemTable::NewIterator() from SeekToFirst until
    !Valid(),
  * writes that iteration with its TableBuilder as lsbm/builder.cc:36-48 does
    (kNoCompression, the internal-key comparator, and InternalFilterPolicy
    over NewBloomFilterPolicy(10) where the case has a filter).

Malformed payloads are given as raw bytes to WriteBatchInternal::SetContents +
InsertInto, all payloads of a case into one memtable, errors ignored as under
paranoid_checks = false; a payload under 12 bytes takes RecoverLogFile's branch
(lsbm/db_impl.cc:440-443) and is not inserted.  Stored: each returned status
string and the memtable's iteration afterwards.

memtable_tables.bin is one zlib stream of the log files, the iteration records
(u32 length + bytes for each key and each value) and the table files; the JSON
holds {offset, size} pairs into the inflated bytes, the cases' parameters and
the malformed payloads in hex.

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

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

DRIVER = r"""
// Driver for tests/golden/make_memtable_fixture.py: batches -> log file ->
// records -> memtable -> iteration -> table, with the reference's classes,
// over a command file.
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
#include "log_reader.h"
#include "log_writer.h"
#include "memtable.h"
#include "write_batch_internal.h"
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

class StringSource : public SequentialFile {
 public:
  explicit StringSource(const std::string& c) : contents_(c), at_(0) {}
  virtual Status Read(size_t n, Slice* result, char* scratch) {
    if (n > contents_.size() - at_) n = contents_.size() - at_;
    memcpy(scratch, contents_.data() + at_, n);
    *result = Slice(scratch, n);
    at_ += n;
    return Status::OK();
  }
  virtual Status Skip(uint64_t n) {
    if (n > contents_.size() - at_) n = contents_.size() - at_;
    at_ += n;
    return Status::OK();
  }
 private:
  std::string contents_;
  size_t at_;
};

struct FailReporter : public log::Reader::Reporter {
  virtual void Corruption(size_t bytes, const Status& s) { exit(8); }
};

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

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  InternalKeyComparator internal(BytewiseComparator());
  const FilterPolicy* bloom = NewBloomFilterPolicy(10);
  InternalFilterPolicy internal_bloom(bloom);
  int c;
  while ((c = fgetc(in)) != EOF) {
    MemTable* mem = new MemTable(internal);
    mem->Ref();
    if (c == 'C') {  // block_size, restart interval, filter, n_batches, per batch: seq, n_ops, (type, key, value)*
      Options o;
      o.comparator = &internal;
      o.block_size = r32();
      o.block_restart_interval = (int)r32();
      o.compression = kNoCompression;
      o.filter_policy = r32() ? &internal_bloom : NULL;
      const uint32_t n_batches = r32();
      StringSink log_file;
      {
        log::Writer writer(&log_file);
        for (uint32_t b = 0; b < n_batches; b++) {
          WriteBatch batch;
          WriteBatchInternal::SetSequence(&batch, r64());
          const uint32_t n_ops = r32();
          for (uint32_t i = 0; i < n_ops; i++) {
            const uint32_t type = r32();
            std::string k = rstr(), v = rstr();
            if (type) batch.Put(k, v); else batch.Delete(k);
          }
          if (!writer.AddRecord(WriteBatchInternal::Contents(&batch)).ok()) exit(4);
        }
      }
      wstr(log_file.contents);
      FailReporter reporter;
      StringSource* source = new StringSource(log_file.contents);
      std::vector<uint32_t> lens;
      {
        log::Reader reader(source, &reporter, true, 0);
        std::string scratch;
        Slice record;
        WriteBatch batch;
        while (reader.ReadRecord(&record, &scratch)) {
          if (record.size() < 12) exit(9);
          lens.push_back(record.size());
          WriteBatchInternal::SetContents(&batch, record);
          if (!WriteBatchInternal::InsertInto(&batch, mem).ok()) exit(5);
        }
      }
      delete source;
      if (lens.size() != n_batches) exit(6);
      w32(lens.size());
      for (size_t i = 0; i < lens.size(); i++) w32(lens[i]);
      write_iteration(mem);
      // BuildTable (lsbm/builder.cc:36-48): no file without an entry
      StringSink table;
      Iterator* it = mem->NewIterator();
      it->SeekToFirst();
      if (it->Valid()) {
        TableBuilder builder(o, &table);
        for (; it->Valid(); it->Next()) builder.Add(it->key(), it->value());
        if (!builder.Finish().ok() || builder.FileSize() != table.contents.size()) exit(7);
      }
      delete it;
      wstr(table.contents);
    } else if (c == 'B') {  // n_payloads, payload*
      const uint32_t n = r32();
      w32(n);
      for (uint32_t i = 0; i < n; i++) {
        std::string payload = rstr();
        Status s;
        if (payload.size() < 12) {
          s = Status::Corruption("log record too small");  // (lsbm/db_impl.cc:440-443: not inserted)
        } else {
          WriteBatch batch;
          WriteBatchInternal::SetContents(&batch, payload);
          s = WriteBatchInternal::InsertInto(&batch, mem);
        }
        wstr(s.ToString());
      }
      write_iteration(mem);
    } else {
      exit(10);
    }
    mem->Unref();
  }
  fclose(out);
  return 0;
}
"""


def build_driver(tmp):
    if not os.path.isdir(OBJ):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "dbbench"], check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*", "*.o"))) if not o.endswith("lsbm/db_bench.o")]
    src = os.path.join(tmp, "memtable_driver.cc")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "memtable_driver")
    subprocess.run(["g++", "-std=c++11", "-w", "-O2", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX",
                    "-I" + REF, "-I" + REF + "/include", "-I" + REF + "/common", "-o", exe, src] + objs, check=True)
    return exe


def p32(v):
    return struct.pack("<I", v)


def pstr(b):
    return p32(len(b)) + bytes(b)


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def op_bytes(op):
    t, k, v = op
    return 1 + len(varint(len(k))) + len(k) + (len(varint(len(v))) + len(v) if t else 0)


def payload_bytes(ops):
    return 12 + sum(op_bytes(op) for op in ops)


def filler(target):
    """One Put whose batch payload is exactly `target` bytes."""
    for vl in range(max(0, target - 40), target):
        ops = [(1, b"fill", b"f" * vl)]
        if payload_bytes(ops) == target:
            return ops
    raise AssertionError(target)


def rep(batches):
    """The batches' rep_ bytes, as WriteBatch makes them (to lay the log out)."""
    out = []
    for seq, ops in batches:
        b = struct.pack("<QI", seq, len(ops))
        for t, k, v in ops:
            b += bytes([t]) + varint(len(k)) + k + (varint(len(v)) + v if t else b"")
        out.append(b)
    return out


def physical_types(batches):
    sys.path.insert(0, REPO)
    from lsbm_amd.log import layout_records
    image, heads = layout_records(rep(batches))
    return [int(image[h + 6]) for h in heads], [int(h) for h in heads], len(image)


def case_specs():
    """[(name, block_size, restart_interval, filter, [(sequence, [(type, key, value)])])]."""
    rng = random.Random(0x3E37AB1E)

    def word(lo=3, hi=12, alphabet=b"abcd"):
        return bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))

    def value(lo=0, hi=20):
        return bytes(rng.randrange(256) for _ in range(rng.randint(lo, hi)))

    cases = [("no_batches", 256, 4, 0, []),
             ("empty_batch", 256, 4, 0, [(5, [])]),
             ("one_entry", 256, 4, 1, [(7, [(1, b"key", b"value")])]),
             ("one_batch", 256, 4, 1, [(100, [(rng.choice((0, 1, 1)), word(), value()) for _ in range(24)])]),
             ("batch_1000", 1024, 16, 1, [(1 << 20, [(1, word(5, 7, b"abcdefgh"), value(0, 3)) for _ in range(1000)])])]
    # three fragments (FIRST 100 bytes, MIDDLE a whole block, LAST the rest) with the 2- and 3-byte value
    # lengths; a record that ends 7 bytes before its block does (the next one opens with an empty FIRST
    # fragment); a record that ends 3 bytes before (a zero trailer follows)
    big = [(1, b"big", b"B" * 20000), (1, b"two", b"t" * 200), (1, b"none", b""), (0, b"gone", b""),
           (1, b"more", b"m" * 12800), (1, b"last", b"end")]
    batches = [(10, filler(32768 - 7 - 100 - 7)), (20, big)]
    assert physical_types(batches)[0] == [1, 2, 3, 4], physical_types(batches)
    end = physical_types(batches)[2]
    batches.append((30, filler(32768 - end % 32768 - 7 - 7)))
    assert physical_types(batches)[2] % 32768 == 32768 - 7
    batches.append((40, [(1, b"after7", b"x"), (0, b"two", b"")]))
    types, heads, end = physical_types(batches)
    assert types[-2:] == [2, 4] and heads[-1] - heads[-2] == 7, (types, heads)
    batches.append((50, filler(32768 - end % 32768 - 7 - 3)))
    assert physical_types(batches)[2] % 32768 == 32768 - 3
    batches.append((60, [(1, b"after3", b"y")]))
    types, heads, end = physical_types(batches)
    assert types[-1] == 1 and heads[-1] % 32768 == 0
    cases.append(("fragments", 4096, 16, 0, batches))
    # deletions, one of a key that was never written
    users = sorted({word() for _ in range(12)})
    b0 = [(1, u, value()) for u in users]
    b1 = [(0, u, b"") for u in users[::3]] + [(0, b"never-written", b"")]
    b2 = [(1, u, value()) for u in users[::6]]
    cases.append(("deletions", 256, 4, 0, [(1, b0), (1 + len(b0), b1), (1 + len(b0) + len(b1), b2)]))
    # one user key written 300 times across batches, neighbours around it
    batches, seq = [], 1000
    for b in range(60):
        ops = [(1 if rng.random() < 0.9 else 0, b"hot", value(0, 4)) for _ in range(5)]
        if b % 20 == 0:
            ops.append((1, rng.choice((b"ho", b"hot\x00", b"hou")), b"n"))
        batches.append((seq, ops))
        seq += len(ops)
    cases.append(("hot_key_300", 256, 4, 1, batches))
    # a key that is a prefix of the next, the empty user key, the empty value
    pre = [b"", b"a", b"ab", b"ab\x00", b"ab\x00\x00", b"abc", b"abcdefg", b"abcdefgh", b"abcdefgh\x00", b"abcdefghi"]
    order = list(pre)
    rng.shuffle(order)
    cases.append(("prefix_and_empty", 256, 4, 0,
                  [(3, [(1, k, b"" if i % 3 == 0 else value(1, 5)) for i, k in enumerate(order)]),
                   (3 + len(order), [(0, b"", b""), (1, b"ab", b"")])]))
    # 137-byte keys that differ only in the last byte and only in byte 8k-1 / 8k / 8k+1
    base = bytes(rng.choice(b"xyz") for _ in range(137))
    long_keys = {base[:-1] + bytes([b]) for b in (0x01, 0x7f, 0x80, 0xfe)}
    for k in (1, 8, 16):
        for at in (8 * k - 1, 8 * k, 8 * k + 1):
            for b in (0x00, 0x80, 0xff):
                long_keys.add(base[:at] + bytes([b]) + base[at + 1:])
    long_keys = sorted(long_keys)
    rng.shuffle(long_keys)
    batches, seq = [], 77
    for r in range(3):
        ops = [(1, k, bytes([r, i])) for i, k in enumerate(long_keys[r::3])]
        batches.append((seq, ops))
        seq += len(ops)
    cases.append(("long_keys_one_byte", 256, 4, 1, batches))
    # equal internal keys: batches with the same sequence and user key (the later one first), and a
    # Put and a Delete at one sequence (the tag's type byte orders them)
    cases.append(("equal_internal_keys", 256, 4, 0,
                  [(9, [(1, b"same", b"first"), (1, b"other", b"o1")]),
                   (9, [(1, b"same", b"second")]),
                   (9, [(0, b"same", b"")]),
                   (9, [(1, b"same", b"third"), (1, b"other", b"o2")]),
                   (10, [(1, b"other", b"o3")])]))
    # batches that arrive in descending key order
    users = sorted({word() for _ in range(40)}, reverse=True)
    cases.append(("descending_arrival", 256, 4, 0, [(500 + i, [(1, u, value(1, 6))]) for i, u in enumerate(users)]))
    return cases


def malformed_specs():
    """[(name, [payload])]: every payload of a case goes into one memtable."""
    def head(seq, count):
        return struct.pack("<QI", seq, count)

    def put(k, v):
        return b"\x01" + varint(len(k)) + k + varint(len(v)) + v

    def delete(k):
        return b"\x00" + varint(len(k)) + k

    good = head(100, 2) + put(b"good", b"1") + delete(b"gone")
    return [("length_0", [b""]),
            ("length_11", [head(1, 0)[:11]]),
            ("length_12_count_0", [head(1, 0)]),
            ("length_12_count_1", [head(1, 1)]),
            ("put_key_varint_cut", [head(5, 2) + put(b"a", b"b") + b"\x01\x80"]),
            ("delete_key_varint_cut", [head(5, 2) + put(b"a", b"b") + b"\x00\x80"]),
            ("put_ends_at_tag", [head(5, 2) + put(b"a", b"b") + b"\x01"]),
            ("key_one_past_end", [head(5, 2) + put(b"a", b"b") + b"\x01\x05four"]),
            ("delete_key_one_past_end", [head(5, 2) + delete(b"a") + b"\x00\x05four"]),
            ("value_one_past_end", [head(5, 2) + put(b"a", b"b") + b"\x01\x01k\x03vv"]),
            ("value_varint_missing", [head(5, 2) + put(b"a", b"b") + b"\x01\x01k"]),
            ("tag_2", [head(5, 3) + put(b"a", b"b") + b"\x02\x01k\x01v" + put(b"c", b"d")]),
            ("tag_255_first", [head(5, 1) + b"\xff"]),
            ("count_one_high", [head(5, 3) + put(b"a", b"b") + delete(b"c")]),
            ("count_one_low", [head(5, 1) + put(b"a", b"b") + delete(b"c")]),
            ("varint_fifth_byte_high_bits", [head(5, 2) + b"\x01\x83\x80\x80\x80\x70key" + b"\x01v" + delete(b"z")]),
            ("varint_fifth_byte_high_bits_value",
             [head(5, 1) + b"\x01\x01k" + b"\x82\x80\x80\x80\x60vv"]),
            ("varint_five_continuation_bytes", [head(5, 2) + put(b"a", b"b") + b"\x01\x80\x80\x80\x80\x80\x01k\x01v"]),
            ("varint_fifth_byte_too_long", [head(5, 1) + b"\x01\x83\x80\x80\x80\x01key\x01v"]),
            ("bad_between_good", [good, head(200, 2) + put(b"half", b"h") + b"\x02", head(300, 1) + put(b"tail", b"t")]),
            ("small_between_good", [good, b"tiny", head(300, 1) + put(b"tail", b"t")])]


def main():
    tmp = tempfile.mkdtemp(prefix="lsbm_memfx_")
    exe = build_driver(tmp)
    cases, bad = case_specs(), malformed_specs()
    cmds = []
    for _, block_size, restart_interval, filt, batches in cases:
        cmd = b"C" + p32(block_size) + p32(restart_interval) + p32(filt) + p32(len(batches))
        for seq, ops in batches:
            cmd += struct.pack("<Q", seq) + p32(len(ops)) + b"".join(p32(t) + pstr(k) + pstr(v) for t, k, v in ops)
        cmds.append(cmd)
    for _, payloads in bad:
        cmds.append(b"B" + p32(len(payloads)) + b"".join(pstr(p) for p in payloads))
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

    blob = bytearray()

    def keep(b):
        blob.extend(b)
        return [len(blob) - len(b), len(b)]

    def iteration():
        nonlocal p
        n, start = u32(), p
        for _ in range(2 * n):
            s()
        return n, keep(buf[start:p])

    recs, bads = [], []
    for name, block_size, restart_interval, filt, batches in cases:
        log = keep(s())
        lens = [u32() for _ in range(u32())]
        n, it = iteration()
        assert n == sum(len(ops) for _, ops in batches)
        table = s()
        recs.append({"name": name, "block_size": block_size, "restart_interval": restart_interval,
                     "bits_per_key": 10 if filt else None, "log": log, "record_lens": lens, "n_entries": n,
                     "iteration": it, "table": keep(table) if table else None})
    for name, payloads in bad:
        assert u32() == len(payloads)
        statuses = [s().decode() for _ in payloads]
        n, it = iteration()
        bads.append({"name": name, "payloads": [x.hex() for x in payloads], "statuses": statuses, "n_entries": n,
                     "iteration": it})
    assert p == len(buf)
    fx = {"source": "lsbm's WriteBatch, log::Writer, log::Reader, WriteBatchInternal::InsertInto, MemTable iteration "
                    "and TableBuilder (kNoCompression, internal-key comparator, InternalFilterPolicy over a 10-bit "
                    "bloom where bits_per_key is set), built from the reference's objects (oracle/Makefile dbbench, "
                    "-DNDEBUG); memtable_tables.bin is one zlib stream, {offset, size} pairs index its inflated bytes",
          "inflated_bytes": len(blob), "cases": recs, "malformed": bads}
    packed = zlib.compress(bytes(blob), 9)
    open(os.path.join(HERE, "memtable_tables.bin"), "wb").write(packed)
    json.dump(fx, open(os.path.join(HERE, "memtable_fixture.json"), "w"), indent=0)
    print(f"{len(recs)} cases, {len(bads)} malformed cases, {sum(r['n_entries'] for r in recs)} entries "
          f"({len(blob)} B inflated, {len(packed)} B stored)")


if __name__ == "__main__":
    sys.exit(main())
