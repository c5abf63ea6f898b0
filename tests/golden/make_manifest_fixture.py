"""Fixture of the reference's own VersionEdit and Recover for the GPU MANIFEST
engine (include/lsbm_manifest.h).

    python tests/golden/make_manifest_fixture.py

Compiles the small driver below (our own code) and links it with the
reference's objects that `make -C oracle dbbench` leaves in oracle/_ref/obj
(built with -DNDEBUG; everything but db_bench's main), runs it on the
scenarios of manifest_cases.py, and writes tests/golden/manifest_fixture.json
(the index) and manifest_fixture.bin (one zlib stream of JSON text).

Per record the driver zeroes runtime::write_cursor and runtime::read_cursor_,
runs VersionEdit::DecodeFrom on a fresh edit and records Status::ToString();
where that is OK, the bytes EncodeTo writes for the decoded object (which
carry the cursors the record left in the globals) and the number of new files
GetNewFiles() holds per type.  Per edit description it sets the cursor
globals, builds the edit with SetComparatorName / Set* / DeleteFile / AddFile
and records EncodeTo's bytes.  Per whole MANIFEST it writes the records with
the reference's log::Writer, damages the file as the scenario says, writes
CURRENT, and records BasicVersionSet::Recover()'s status text and, where that
is OK, LastSequence, LogNumber, PrevLogNumber, ManifestFileNumber and
AddLiveFiles.

Last, a whole database directory from the models' bytes (two Level-0 tables,
one log, MANIFEST-000002, CURRENT; manifest_cases.directory_logs) is opened by
the reference's DB::Open through oracle/_ref/db_verify --open (reference code
only): its MANIFEST's bytes, and the live entry count and digest the reference
reports for it, are recorded.

Byte strings are stored as {length, crc32} (and hex up to 64 bytes): the model
rebuilds them.  Only results produced by the reference are stored; no
reference source.
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

from golden import logreadmodel, memtablemodel, writemodel  # noqa: E402
from golden import manifest_cases as cases  # noqa: E402

REF = os.environ.get("REF_DIR", "/root/reference")
OBJ = os.path.join(REPO, "oracle", "_ref", "obj")

DRIVER = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>
#include <vector>
#define private public
#define protected public
#include "lsbm/version_edit.h"
#include "lsbm/version_set.h"
#undef private
#undef protected
#include "common/log_writer.h"
#include "leveldb/comparator.h"
#include "leveldb/env.h"
#include "leveldb/options.h"
#include "leveldb/params.h"

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
static void cursors(uint64_t wc, const uint64_t* rc) {
  runtime::write_cursor = wc;
  for (int i = 0; i < 4; i++) runtime::read_cursor_[i] = rc[i];
}
static InternalKey key_of(const std::string& s) { InternalKey k; k.DecodeFrom(s); return k; }

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const std::string dir = argv[3];
  if (!in || !out) return 2;
  const uint64_t zero[4] = {0, 0, 0, 0};
  const uint32_t n_records = r32();
  for (uint32_t i = 0; i < n_records; i++) {
    const std::string rec = rstr();
    cursors(0, zero);
    VersionEdit edit;
    const Status s = edit.DecodeFrom(rec);
    wstr(s.ToString());
    if (s.ok()) {
      std::string again;
      edit.EncodeTo(&again);
      wstr(again);
      for (int t = 0; t < 4; t++) w32(edit.GetNewFiles()[t].size());
    }
  }
  const uint32_t n_edits = r32();
  for (uint32_t i = 0; i < n_edits; i++) {
    VersionEdit edit;
    const uint32_t has = r32();
    const std::string name = rstr();
    const uint64_t log = r64(), prev = r64(), next = r64(), seq = r64(), wc = r64();
    uint64_t rc[4];
    for (int k = 0; k < 4; k++) rc[k] = r64();
    cursors(wc, rc);
    if (has & 1) edit.SetComparatorName(name);
    if (has & 2) edit.SetLogNumber(log);
    if (has & 4) edit.SetPrevLogNumber(prev);
    if (has & 8) edit.SetNextFile(next);
    if (has & 16) edit.SetLastSequence(seq);
    const uint32_t n_del = r32();
    for (uint32_t k = 0; k < n_del; k++) {
      const uint32_t t = r32(), level = r32();
      edit.DeleteFile((SortedTableType)t, level, r64());
    }
    const uint32_t n_new = r32();
    for (uint32_t k = 0; k < n_new; k++) {
      const uint32_t t = r32(), level = r32();
      const uint64_t number = r64(), size = r64();
      const std::string a = rstr(), b = rstr();
      edit.AddFile((SortedTableType)t, level, number, size, key_of(a), key_of(b));
    }
    std::string bytes;
    edit.EncodeTo(&bytes);
    wstr(bytes);
  }
  const uint32_t n_manifests = r32();
  Env* env = Env::Default();
  for (uint32_t i = 0; i < n_manifests; i++) {
    char sub[32];
    snprintf(sub, sizeof(sub), "/m%u", i);
    const std::string db = dir + sub, file = db + "/MANIFEST-000002";
    env->CreateDir(db);
    WritableFile* wf;
    if (!env->NewWritableFile(file, &wf).ok()) return 4;
    {
      log::Writer writer(wf);
      const uint32_t n = r32();
      for (uint32_t k = 0; k < n; k++)
        if (!writer.AddRecord(rstr()).ok()) return 4;
    }
    wf->Close();
    delete wf;
    const uint32_t how = r32();
    const uint64_t arg = r64();
    std::string bytes;
    if (!ReadFileToString(env, file, &bytes).ok()) return 4;
    wstr(bytes);  // as log::Writer wrote it
    if (how == 1) bytes.resize(bytes.size() - arg);
    if (how == 2) bytes[arg] ^= 0xFF;
    if (!WriteStringToFile(env, bytes, file).ok()) return 4;
    if (!WriteStringToFile(env, "MANIFEST-000002\n", db + "/CURRENT").ok()) return 4;
    cursors(0, zero);
    Options options;
    options.env = env;
    InternalKeyComparator icmp(BytewiseComparator());
    BasicVersionSet* vs = new BasicVersionSet(db, &options, NULL, &icmp);  // (never deleted: its destructor asserts)
    const Status s = vs->Recover();
    wstr(s.ToString());
    if (s.ok()) {
      w64(vs->LastSequence());
      w64(vs->LogNumber());
      w64(vs->PrevLogNumber());
      w64(vs->ManifestFileNumber());
      std::set<uint64_t> live;
      vs->AddLiveFiles(&live);
      w32(live.size());
      for (std::set<uint64_t>::iterator it = live.begin(); it != live.end(); ++it) w64(*it);
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
    src, exe = os.path.join(tmp, "manifest_driver.cc"), os.path.join(tmp, "manifest_driver")
    open(src, "w").write(DRIVER)
    subprocess.run(["g++"] + flags + ["-o", exe, src] + objs, check=True)
    return exe


def model_directory(path, crc):
    """The directory of manifest_cases.directory_logs from the models' bytes; returns the MANIFEST's bytes."""
    logs, last = cases.directory_logs()
    D = cases.DIRECTORY
    os.makedirs(path)
    files = []
    for number, recs in zip(D["table_numbers"], logs[:2]):
        at, pairs = 0, []
        for rec in recs:
            pairs.append((at, len(rec)))
            at += len(rec)
        ents = memtablemodel.entries(b"".join(recs), pairs)[0]
        table = memtablemodel.table_file(ents, D["block_size"], D["restart_interval"], None)
        open(os.path.join(path, "%06d.ldb" % number), "wb").write(table)
        files.append((0, 0, number, len(table), ents[0][0], ents[-1][0]))
    open(os.path.join(path, "%06d.log" % D["log_number"]), "wb").write(writemodel.add_records(logs[2], crc=crc)[0])
    manifest = writemodel.add_records([cases.directory_snapshot(files, last[1])], crc=crc)[0]
    open(os.path.join(path, "MANIFEST-%06d" % D["manifest_number"]), "wb").write(manifest)
    open(os.path.join(path, "CURRENT"), "wb").write(b"MANIFEST-%06d\n" % D["manifest_number"])
    return manifest


def opened_directory(tmp):
    """db_verify --open over the models' directory: {manifest, live, digest, open_error}."""
    from conftest import Oracle
    exe = os.path.join(REPO, "oracle", "_ref", "db_verify")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "dbbench_gpu"], check=True)
    so = os.path.join(REPO, "oracle", "liboracle_crc32c.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle")], check=True)
    oracle = Oracle(so)
    path = os.path.join(tmp, "db")
    manifest = model_directory(path, lambda b: logreadmodel.mask(oracle.value(b)))
    r = subprocess.run([exe, path, "--open"], capture_output=True, text=True)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert r.returncode == 0 and line["open_error"] == "", line
    return {"manifest": summary(manifest), "live": line["live"], "digest": line["digest"],
            "open_error": line["open_error"], "tables": line["tables"]}


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


def pstr(b):
    return struct.pack("<I", len(b)) + bytes(b)


def summary(b):
    """What the fixture keeps of a byte string the model rebuilds."""
    d = {"length": len(b), "crc32": zlib.crc32(b)}
    if len(b) <= 64:
        d["hex"] = bytes(b).hex()
    return d


def pack_edit(e):
    has = (1 if e["comparator"] is not None else 0) | sum(
        bit for bit, name in ((2, "log_number"), (4, "prev_log_number"), (8, "next_file"), (16, "last_sequence"))
        if e[name] is not None)
    out = struct.pack("<I", has) + pstr(e["comparator"] or b"")
    out += struct.pack("<5Q", *(e[name] or 0 for name in ("log_number", "prev_log_number", "next_file", "last_sequence",
                                                         "write_cursor")))
    out += struct.pack("<4Q", *e["read_cursors"])
    out += struct.pack("<I", len(e["deleted"])) + b"".join(struct.pack("<IIQ", *d) for d in e["deleted"])
    out += struct.pack("<I", len(e["new"]))
    for (t, level, number, size, a, b) in e["new"]:
        out += struct.pack("<IIQQ", t, level, number, size) + pstr(a) + pstr(b)
    return out


def main():
    recs, eds, mans = cases.records(), cases.edits(), cases.manifests()
    cmd = struct.pack("<I", len(recs)) + b"".join(pstr(b) for _, b in recs)
    cmd += struct.pack("<I", len(eds)) + b"".join(pack_edit(e) for _, e in eds)
    cmd += struct.pack("<I", len(mans))
    for _, payloads, how in mans:
        cmd += struct.pack("<I", len(payloads)) + b"".join(pstr(p) for p in payloads)
        cmd += struct.pack("<IQ", 0 if how is None else 1 if how[0] == "cut" else 2, 0 if how is None else how[1])
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        open(fi, "wb").write(cmd)
        subprocess.run([exe, fi, fo, tmp], check=True)
        r = Reader(open(fo, "rb").read())
        directory = opened_directory(tmp)
    body = {"records": {}, "edits": {}, "manifests": {}}
    index = {"records": len(recs), "edits": len(eds), "manifests": {}, "statuses": {}}
    for name, b in recs:
        status = r.bytes().decode()
        d = {"status": status, "input": summary(b)}
        if status == "OK":
            d["encoded"] = summary(r.bytes())
            d["new_per_type"] = [r.u32() for _ in range(4)]
        body["records"][name] = d
        index["statuses"][status] = index["statuses"].get(status, 0) + 1
    for name, _ in eds:
        body["edits"][name] = summary(r.bytes())
    for name, payloads, how in mans:
        d = {"file": summary(r.bytes()), "status": r.bytes().decode()}
        if d["status"] == "OK":
            d.update(last_sequence=r.u64(), log_number=r.u64(), prev_log_number=r.u64(), manifest_file_number=r.u64())
            d["live"] = [r.u64() for _ in range(r.u32())]
        body["manifests"][name] = d
        index["manifests"][name] = d["status"]
    assert r.p == len(r.buf)
    body["directory"] = index["directory"] = directory
    text = json.dumps(body, sort_keys=True, separators=(",", ":")).encode()
    blob = zlib.compress(text, 9)
    index["bin"] = {"inflated": len(text), "crc32": zlib.crc32(text)}
    open(os.path.join(HERE, "manifest_fixture.bin"), "wb").write(blob)
    with open(os.path.join(HERE, "manifest_fixture.json"), "w") as f:
        json.dump(index, f, sort_keys=True, indent=1)
        f.write("\n")
    print(f"wrote manifest_fixture.json and manifest_fixture.bin ({len(blob)} bytes, {len(text)} inflated)")


if __name__ == "__main__":
    main()
