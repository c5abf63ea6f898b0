"""Fixture of the reference's own Block / BlockBuilder results for the GPU block
reader (include/lsbm_block.h).

    python tests/golden/make_block_fixture.py [--sanitize]

Compiles the small driver below (our own code) against the reference's
table/block.cc, block_builder.cc, iterator.cc, util/coding.cc, comparator.cc,
status.cc and common/dbformat.cc (flags as in oracle/Makefile) into a temporary
directory, runs it, and writes tests/golden/block_fixture.json:

  * blocks built by the reference's BlockBuilder (restart intervals 16, 3, 1;
    empty keys and values; keys > 127 B and > 16383 B; a 16 KiB value;
    internal keys; the empty block), each with its bytes, entry count and the
    SHA-256 of the reference's forward iteration;
  * mutations of two of those blocks (ops over the built bytes) with the
    reference's verdict: the entries before the error and the status string;
  * Seek probes of every block with the reference's result (state, current_,
    key length, value offset and length; the found keys as one SHA-256).

--sanitize builds the driver with -fsanitize=address,undefined: the
reference itself must stay in bounds on every mutation (a mutation on which it
does not is dropped from MUTATIONS).  Only bytes and verdicts produced by the
reference are stored; no reference source.
"""
import hashlib
import json
import os
import random
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden import blockmodel as bm  # noqa: E402

REF = os.environ.get("REF_DIR", "/root/reference")
SRCS = ["table/block_builder.cc", "table/iterator.cc", "util/coding.cc", "util/comparator.cc",
        "util/status.cc", "common/dbformat.cc", "port/port_posix.cc", "util/logging.cc",
        "util/filter_policy.cc"]

DRIVER = r"""
// Driver for tests/golden/make_block_fixture.py: runs the reference's
// BlockBuilder, Block::Iter forward iteration and Seek over a command file.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "leveldb/comparator.h"
#include "leveldb/iterator.h"
#include "leveldb/options.h"
#include "leveldb/table.h"
#include "table/block_builder.h"
#include "table/format.h"
#include "dbformat.h"
#define private public  // Block::Iter and its current_
#include "table/block.cc"
#undef private
using namespace leveldb;

static FILE *in, *out;
static uint32_t r32() { uint32_t v; if (fread(&v, 4, 1, in) != 1) exit(3); return v; }
static std::string rstr() { uint32_t n = r32(); std::string s(n, '\0'); if (n && fread(&s[0], 1, n, in) != n) exit(3); return s; }
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void wstr(const std::string& s) { w32(s.size()); fwrite(s.data(), 1, s.size(), out); }

int main(int argc, char** argv) {
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  const Comparator* bytewise = BytewiseComparator();
  InternalKeyComparator internal(bytewise);
  int c;
  while ((c = fgetc(in)) != EOF) {
    if (c == 'B') {  // BlockBuilder: interval, n, (key, value)*
      // (Options' constructor lives in util/options.cc with the Env; only
      // these two fields are read by BlockBuilder)
      void* mem = calloc(1, sizeof(Options));
      Options* o = static_cast<Options*>(mem);
      o->block_restart_interval = (int)r32();
      o->comparator = bytewise;
      BlockBuilder b(o);
      uint32_t n = r32();
      for (uint32_t i = 0; i < n; i++) {
        std::string k = rstr(), v = rstr();
        b.Add(k, v);
      }
      wstr(b.Finish().ToString());
      free(mem);
      continue;
    }
    // 'W' walk / 'S' seek: an exact-size heap copy, so that a sanitizer sees
    // any read past the block
    uint32_t cmpi = r32();
    std::string blk = rstr();
    char* data = static_cast<char*>(malloc(blk.size() ? blk.size() : 1));
    memcpy(data, blk.data(), blk.size());
    const Comparator* cmp = cmpi ? static_cast<const Comparator*>(&internal) : bytewise;
    {
      Block block(data, blk.size(), false);
      if (c == 'W') {
        Iterator* it = block.NewIterator(cmp);
        std::vector<std::string> rec;
        uint32_t n = 0;
        std::string body;
        for (it->SeekToFirst(); it->Valid(); it->Next()) {
          n++;
          uint32_t kl = it->key().size(), vo = it->value().data() - data, vl = it->value().size();
          body.append(reinterpret_cast<char*>(&kl), 4);
          body.append(it->key().data(), kl);
          body.append(reinterpret_cast<char*>(&vo), 4);
          body.append(reinterpret_cast<char*>(&vl), 4);
        }
        w32(n);
        wstr(it->status().ToString());
        fwrite(body.data(), 1, body.size(), out);
        delete it;
      } else {
        uint32_t nt = r32();
        for (uint32_t i = 0; i < nt; i++) {
          std::string t = rstr();
          Iterator* it = block.NewIterator(cmp);
          it->Seek(t);
          Block::Iter* bi = dynamic_cast<Block::Iter*>(it);
          uint32_t valid = it->Valid() ? 1 : 0;
          w32(valid);
          w32(bi ? bi->current_ : 0xffffffffu);
          wstr(valid ? it->key().ToString() : std::string());
          w32(valid ? (uint32_t)(it->value().data() - data) : 0);
          w32(valid ? (uint32_t)it->value().size() : 0);
          wstr(it->status().ToString());
          delete it;
        }
      }
    }
    free(data);
  }
  fclose(out);
  return 0;
}
"""


def build_driver(tmp, sanitize):
    src = os.path.join(tmp, "block_driver.cc")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "block_driver")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++11", "-w", "-pthread", "-DNDEBUG", "-DOS_LINUX", "-DLEVELDB_PLATFORM_POSIX",
                    *flags, "-I" + REF, "-I" + REF + "/include", "-I" + REF + "/common", "-o", exe, src]
                   + [os.path.join(REF, s) for s in SRCS], check=True)
    return exe


def p32(v):
    return struct.pack("<I", v)


def pstr(b):
    return p32(len(b)) + bytes(b)


class Driver:
    """Batches commands into one run of the driver."""

    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.cmds, self.readers = exe, tmp, [], []

    def build(self, interval, entries, sink):
        self.cmds.append(b"B" + p32(interval) + p32(len(entries))
                         + b"".join(pstr(k) + pstr(v) for k, v in entries))
        self.readers.append(("B", sink))

    def walk(self, block, sink):
        self.cmds.append(b"W" + p32(0) + pstr(block))
        self.readers.append(("W", sink))

    def seek(self, block, cmp, targets, sink):
        self.cmds.append(b"S" + p32(cmp) + pstr(block) + p32(len(targets)) + b"".join(pstr(t) for t in targets))
        self.readers.append(("S", sink, len(targets)))

    def run(self):
        fi, fo = os.path.join(self.tmp, "in.bin"), os.path.join(self.tmp, "out.bin")
        open(fi, "wb").write(b"".join(self.cmds))
        subprocess.run([self.exe, fi, fo], check=True)
        buf, p = open(fo, "rb").read(), 0

        def u32():
            nonlocal p
            v = struct.unpack_from("<I", buf, p)[0]
            p += 4
            return v

        def s():
            nonlocal p
            n = u32()
            v = buf[p:p + n]
            p += n
            return v

        for rd in self.readers:
            if rd[0] == "B":
                rd[1](s())
            elif rd[0] == "W":
                n, status = u32(), s().decode()
                ents = []
                for _ in range(n):
                    k = s()
                    ents.append((k, u32(), u32()))
                rd[1](n, status, ents)
            else:
                res = []
                for _ in range(rd[2]):
                    valid, cur = u32(), u32()
                    key = s()
                    vo, vl = u32(), u32()
                    res.append((valid, cur, key, vo, vl, s().decode()))
                rd[1](res)
        assert p == len(buf)
        self.cmds, self.readers = [], []


def internal_key(user, seq, typ=1):
    return user + struct.pack("<Q", (seq << 8) | typ)


def built_specs():
    """(name, restart interval, [(key, value)], internal?) of the built blocks."""
    rng = random.Random(0xB10C)
    specs = []

    def sorted_keys(n, lo, hi, alphabet=b"abcdefgh"):
        ks = set()
        while len(ks) < n:
            ks.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))))
        return sorted(ks)

    def vals(n, lo, hi):
        return [bytes(rng.randrange(256) for _ in range(rng.randint(lo, hi))) for _ in range(n)]

    k = sorted_keys(200, 4, 18)
    specs.append(("i16_200", 16, list(zip(k, vals(200, 0, 12))), False))
    k = sorted_keys(60, 3, 12)
    specs.append(("i3_60", 3, list(zip(k, vals(60, 0, 20))), False))
    k = sorted_keys(40, 1, 9)
    specs.append(("i1_40", 1, list(zip(k, vals(40, 0, 9))), False))
    specs.append(("one_entry", 16, [(b"only", b"value")], False))
    specs.append(("empty", 16, [], False))
    specs.append(("empty_key_value_i16", 16, [(b"", b""), (b"a", b""), (b"ab", b"x"), (b"b", b"")], False))
    specs.append(("empty_key_value_i1", 1, [(b"", b""), (b"a", b""), (b"ab", b"x"), (b"b", b"")], False))
    # keys > 127 B (multi-byte varints), one > 16383 B (3-byte varints), a 16 KiB value
    pre = bytes(rng.choice(b"xyz") for _ in range(140))
    long_keys = sorted({pre + bytes(rng.choice(b"0123456789") for _ in range(rng.randint(1, 200)))
                        for _ in range(10)})
    long_keys.append(pre + b"~" * 16400)
    lv = vals(len(long_keys), 0, 300)
    lv[3] = bytes(rng.randrange(256) for _ in range(16500))
    specs.append(("long_i3", 3, list(zip(long_keys, lv)), False))
    # internal keys: several tags per user key, newest first
    users = sorted_keys(20, 2, 10)
    ik = [internal_key(u, seq) for u in users for seq in (900, 77, 3)]
    specs.append(("internal_i16", 16, list(zip(ik, vals(len(ik), 0, 10))), True))
    specs.append(("internal_i3", 3, list(zip(ik, vals(len(ik), 0, 10))), True))
    # the two bases of the mutations: 12 entries, interval 3, one-byte headers;
    # m1 ends in a 4-byte entry (1-byte delta, empty value), m2 has values >= 6 B
    mk = [b"key%02d%s" % (i, b"abcdefgh"[: 1 + i % 5]) for i in range(11)] + [b"key10ab"]
    specs.append(("m1", 3, list(zip(mk, [b"v" * (3 + i % 4) for i in range(11)] + [b""])), False))
    specs.append(("m2", 3, list(zip(mk, [bytes([65 + i]) * (6 + i % 5) for i in range(12)])), False))
    return specs


def mutations(blocks):
    """(name, base, ops): ops are ["set", offset, hex] and ["truncate", size]."""
    out = []
    m1, m2 = blocks["m1"], blocks["m2"]

    def layout(b):
        st, ents = bm.walk(b)
        assert st == bm.OK
        restarts, nr = bm.block_layout(b)
        return ents, restarts, nr

    def setb(off, data):
        return ["set", off, bytes(data).hex()]

    e1, r1, n1 = layout(m1)
    e2, r2, n2 = layout(m2)
    for n in range(4):
        out.append((f"size_{n}", "m2", [["truncate", n]]))
    out.append(("num_restarts_0", "m2", [setb(len(m2) - 4, p32(0))]))
    out.append(("num_restarts_max_plus_1", "m2", [setb(len(m2) - 4, p32((len(m2) - 4) // 4 + 1))]))
    out.append(("restart0_at_shared_entry", "m2", [setb(r2, p32(e2[1][3]))]))
    out.append(("restart0_at_restart_entry", "m2", [setb(r2, p32(e2[3][3]))]))
    out.append(("restart0_at_restarts", "m2", [setb(r2, p32(r2))]))
    out.append(("restart1_mid_entry", "m2", [setb(r2 + 4, p32(e2[3][3] + 1))]))
    out.append(("restart2_past_restarts", "m2", [setb(r2 + 8, p32(r2 + 5))]))
    out.append(("restart3_huge", "m2", [setb(r2 + 12, p32(0xFFFFFFF0))]))
    # the restart entry 3 re-encoded with shared = 4 (the key before it is
    # longer): delta 4 bytes shorter, value 4 bytes longer, the bytes stay
    p = e2[3][3]
    sh, ns, vl = m2[p], m2[p + 1], m2[p + 2]
    assert sh == 0 and ns > 4 and vl + 4 < 128
    out.append(("restart_entry_shared", "m2", [setb(p, [4, ns - 4, vl + 4])]))
    out.append(("shared_gt_prev_key", "m2", [setb(e2[1][3], [100])]))
    # a varint that runs into limit: the last entry (4 bytes) all continuation bytes
    p = e1[-1][3]
    assert r1 - p == 4
    out.append(("varint_into_limit", "m1", [setb(p, [0x80] * 4)]))
    # shared as a 5-byte varint whose last byte has bits above 2^32 (dropped):
    # 4 bytes taken from the value
    p = e2[4][3]
    sh, ns, vl = m2[p], m2[p + 1], m2[p + 2]
    assert vl >= 4 and sh < 128
    out.append(("varint5_high_bits_dropped", "m2",
                [setb(p, [0x80 | sh, 0x80, 0x80, 0x80, 0x70, ns, vl - 4])]))
    out.append(("varint5_high_bits_kept", "m2",
                [setb(p, [0x80 | sh, 0x80, 0x80, 0x80, 0x7F, ns, vl - 4])]))
    p = e2[-1][3]
    out.append(("value_past_limit", "m2", [setb(p + 2, [120])]))
    assert m2[p + 2] >= 2
    out.append(("two_bytes_before_limit", "m2", [setb(p + 2, [m2[p + 2] - 2])]))
    out.append(("one_byte_before_limit", "m2", [setb(p + 2, [m2[p + 2] - 1])]))
    return out


def apply_ops(block, ops):
    b = bytearray(block)
    for op in ops:
        if op[0] == "set":
            d = bytes.fromhex(op[2])
            b[op[1]:op[1] + len(d)] = d
        else:
            b = b[:op[1]]
    return bytes(b)


STATE = {"OK": None, "Corruption: bad entry in block": bm.SEEK_BAD_ENTRY,
         "Corruption: bad block contents": bm.SEEK_BAD_CONTENTS}


def probe_record(block, res):
    """[state, pos, key_len, value_offset, value_length] per probe + the keys' SHA-256."""
    h = hashlib.sha256()
    rows = []
    lay = bm.block_layout(block)
    for valid, cur, key, vo, vl, status in res:
        st = STATE[status]
        if st is None:
            st = bm.VALID if valid else bm.NOT_VALID
        assert not (valid and st != bm.VALID)
        if cur == 0xFFFFFFFF:  # no Block::Iter: the error iterator (0) or the empty iterator (size - 4)
            cur = 0 if lay is None else len(block) - 4
        rows.append([st, cur, len(key), vo, vl])
        h.update(struct.pack("<I", len(key)) + key)
    return {"rows": rows, "keys_sha256": h.hexdigest()}


def main():
    sanitize = "--sanitize" in sys.argv
    tmp = tempfile.mkdtemp(prefix="lsbm_block_fx_")
    drv = Driver(build_driver(tmp, sanitize), tmp)
    specs = built_specs()
    blocks = {}
    for name, interval, entries, _ in specs:
        drv.build(interval, entries, lambda b, name=name: blocks.__setitem__(name, b))
    drv.run()
    fx = {"source": "lsbm's BlockBuilder / Block::Iter (table/block_builder.cc, table/block.cc) "
                    "driven by tests/golden/make_block_fixture.py",
          "built": [], "mutated": []}
    cases = []  # (record, block bytes, probe keys, internal?)
    for name, interval, entries, internal in specs:
        rec = {"name": name, "restart_interval": interval, "internal": internal, "hex": blocks[name].hex()}
        fx["built"].append(rec)
        cases.append((rec, blocks[name], [k for k, _ in entries], internal))
    for name, base, ops in mutations(blocks):
        rec = {"name": name, "base": base, "ops": ops}
        fx["mutated"].append(rec)
        base_keys = [k for k, _ in next(s[2] for s in specs if s[0] == base)]
        cases.append((rec, apply_ops(blocks[base], ops), base_keys, False))
    for rec, blk, keys, internal in cases:
        def on_walk(n, status, ents, rec=rec, blk=blk):
            rec["entries"], rec["status"] = n, status
            rec["key_bytes"] = sum(len(k) for k, _, _ in ents)
            rec["value_bytes"] = sum(vl for _, _, vl in ents)
            rec["sha256"] = bm.entries_sha(blk, [(k, vo, vl, 0) for k, vo, vl in ents])
        drv.walk(blk, on_walk)
        targets = bm.seek_targets(keys)
        drv.seek(blk, bm.BYTEWISE, targets,
                 lambda res, rec=rec, blk=blk: rec.__setitem__("seek_bytewise", probe_record(blk, res)))
        if internal:  # (never a key or target shorter than 8 bytes: the reference asserts)
            t8 = [t for t in targets if len(t) >= 8]
            drv.seek(blk, bm.INTERNAL_KEY, t8,
                     lambda res, rec=rec, blk=blk: rec.__setitem__("seek_internal", probe_record(blk, res)))
    drv.run()
    if sanitize:
        print("sanitized run clean:", len(cases), "blocks")
        return 0
    path = os.path.join(HERE, "block_fixture.json")
    json.dump(fx, open(path, "w"), separators=(",", ":"))
    print(f"{len(fx['built'])} built + {len(fx['mutated'])} mutated blocks, {os.path.getsize(path)} B")
    return 0


if __name__ == "__main__":
    sys.exit(main())
