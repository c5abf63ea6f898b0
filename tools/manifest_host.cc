// manifest_host.cc -- the MANIFEST engine's work (include/lsbm_manifest.h) on
// the host, one thread, in the reference's shape: the alternative the device
// calls replace and tools/bench_manifest.py's baseline.  An edit is what
// VersionEdit holds (std::string keys, a std::set of deleted files and a
// std::vector of new files per type), DecodeFrom is a loop over tags with
// GetVarint / GetLengthPrefixedSlice, EncodeTo appends to one std::string, and
// Recover's fold is Builder::Apply's sets and lists with MaybeAddFile's test.
//
//   g++ -O2 -std=c++17 -shared -fPIC -o libmanifest_host.so tools/manifest_host.cc
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DMANIFEST_HOST_MAIN
//       -o manifest_host_check tools/manifest_host.cc && ./manifest_host_check
//
// With -DMANIFEST_HOST_MAIN the program encodes seeded edits, decodes them,
// encodes them again and compares, decodes every truncation of a record with
// all tags (each must fail or end at a group's end), and prints
// "manifest_host self-check ok".  tests/test_manifest_host.py compares the
// shared library with the reference's fixture.
#include <stdint.h>
#include <string.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

extern "C" {
// verdict[n], counts[3] = {new files, deleted files, key bytes} over the OK records; returns a checksum of the edits
uint64_t manifest_host_decode(const uint8_t* image, const uint64_t* records, uint64_t n, uint32_t* verdict,
                              uint64_t* counts);
// DecodeFrom, then EncodeTo of the decoded edit (cursors that are absent 0): the verdict; out_len[0] bytes in out
uint32_t manifest_host_reencode(const uint8_t* rec, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_len);
// EncodeTo of n edits from the flat shapes of lsbm_edit_encode_plan_dev; records[2 n]; returns the bytes (0: no room)
uint64_t manifest_host_encode(const uint64_t* fields, const uint8_t* names, uint64_t n, const uint64_t* del_first,
                              const uint64_t* del_items, const uint64_t* new_first, const uint64_t* new_items,
                              const uint8_t* keys, const uint64_t* key_offsets, uint8_t* out, uint64_t cap,
                              uint64_t* records);
// Recover's loop over records that a reader returned: numbers[4] = {log, previous log, next file, last sequence},
// returns the live files, or UINT64_MAX - verdict at the first record that does not decode
uint64_t manifest_host_recover(const uint8_t* image, const uint64_t* records, uint64_t n, uint64_t* numbers);
}

namespace {

constexpr uint32_t kLevels = 4, kTypes = 4, kFieldWords = 13;

struct File {
  int level;
  uint64_t number, size;
  std::string smallest, largest;
};

struct Edit {
  std::string comparator;
  uint64_t log = 0, prev_log = 0, next_file = 0, last_seq = 0, write_cursor = 0, read_cursor[kLevels] = {0, 0, 0, 0};
  bool has_comparator = false, has_log = false, has_prev_log = false, has_next_file = false, has_last_seq = false;
  std::set<std::pair<int, uint64_t>> deleted[kTypes];
  std::vector<File> added[kTypes];
};

struct Slice {
  const uint8_t* p;
  uint64_t n;
};

bool get32(Slice* in, uint32_t* v) {
  uint32_t r = 0;
  for (uint32_t shift = 0; shift <= 28 && in->n; shift += 7) {
    const uint32_t b = *in->p++;
    in->n--;
    if (b & 128) {
      r |= (b & 127) << shift;
    } else {
      *v = r | b << shift;
      return true;
    }
  }
  return false;
}

bool get64(Slice* in, uint64_t* v) {
  uint64_t r = 0;
  for (uint32_t shift = 0; shift <= 63 && in->n; shift += 7) {
    const uint64_t b = *in->p++;
    in->n--;
    if (b & 128) {
      r |= (b & 127) << shift;
    } else {
      *v = r | b << shift;
      return true;
    }
  }
  return false;
}

bool get_slice(Slice* in, std::string* s) {
  uint32_t len;
  if (!get32(in, &len) || in->n < len) return false;
  s->assign(reinterpret_cast<const char*>(in->p), len);
  in->p += len;
  in->n -= len;
  return true;
}

bool get_level(Slice* in, int* level) {
  uint32_t v;
  if (!get32(in, &v) || v >= kLevels) return false;
  *level = (int)v;
  return true;
}

uint32_t decode(Slice in, Edit* e) {
  uint32_t code = 0, tag;
  while (code == 0 && in.n) {
    if (!get32(&in, &tag)) return 11;
    uint32_t type;
    uint64_t number;
    File f;
    switch (tag) {
      case 1: if (get_slice(&in, &e->comparator)) e->has_comparator = true; else code = 1; break;
      case 2: if (get64(&in, &e->log)) e->has_log = true; else code = 2; break;
      case 9: if (get64(&in, &e->prev_log)) e->has_prev_log = true; else code = 3; break;
      case 3: if (get64(&in, &e->next_file)) e->has_next_file = true; else code = 4; break;
      case 4: if (get64(&in, &e->last_seq)) e->has_last_seq = true; else code = 5; break;
      case 6:
        if (!(get32(&in, &type) && get_level(&in, &f.level) && get64(&in, &number))) code = 6;
        else if (type >= kTypes) code = 12;
        else e->deleted[type].insert(std::make_pair(f.level, number));
        break;
      case 7:
        if (!(get32(&in, &type) && get_level(&in, &f.level) && get64(&in, &f.number) && get64(&in, &f.size) &&
              get_slice(&in, &f.smallest) && get_slice(&in, &f.largest)))
          code = 7;
        else if (type >= kTypes) code = 12;
        else e->added[type].push_back(f);
        break;
      case 10: if (!get64(&in, &e->write_cursor)) code = 8; break;
      case 11:
        if (!get64(&in, &number)) code = 9;
        else if (number >= kLevels) code = 13;
        else if (!get64(&in, &e->read_cursor[number])) code = 9;
        break;
      default: code = 10; break;
    }
  }
  return code;
}

void put(std::string* dst, uint64_t v) {
  while (v >= 128) {
    dst->push_back((char)(v | 128));
    v >>= 7;
  }
  dst->push_back((char)v);
}

void put_slice(std::string* dst, const std::string& s) {
  put(dst, s.size());
  dst->append(s);
}

void encode(const Edit& e, std::string* dst) {
  if (e.has_comparator) put(dst, 1), put_slice(dst, e.comparator);
  if (e.has_log) put(dst, 2), put(dst, e.log);
  if (e.has_prev_log) put(dst, 9), put(dst, e.prev_log);
  if (e.has_next_file) put(dst, 3), put(dst, e.next_file);
  if (e.has_last_seq) put(dst, 4), put(dst, e.last_seq);
  for (uint32_t t = 0; t < kTypes; t++) {
    for (const auto& d : e.deleted[t]) put(dst, 6), put(dst, t), put(dst, d.first), put(dst, d.second);
    for (const File& f : e.added[t]) {
      put(dst, 7), put(dst, t), put(dst, f.level), put(dst, f.number), put(dst, f.size);
      put_slice(dst, f.smallest);
      put_slice(dst, f.largest);
    }
  }
  put(dst, 10), put(dst, e.write_cursor);
  for (uint32_t i = 0; i < kLevels; i++) put(dst, 11), put(dst, i), put(dst, e.read_cursor[i]);
}

uint64_t digest(const Edit& e) {
  uint64_t h = e.log ^ e.next_file ^ e.last_seq ^ e.comparator.size();
  for (uint32_t t = 0; t < kTypes; t++) {
    for (const auto& d : e.deleted[t]) h = h * 31 + d.second;
    for (const File& f : e.added[t]) h = h * 31 + f.number + f.smallest.size() + (f.largest.empty() ? 0 : f.largest[0]);
  }
  return h;
}

}  // namespace

extern "C" {

uint64_t manifest_host_decode(const uint8_t* image, const uint64_t* records, uint64_t n, uint32_t* verdict,
                              uint64_t* counts) {
  uint64_t h = 0;
  counts[0] = counts[1] = counts[2] = 0;
  for (uint64_t r = 0; r < n; r++) {
    Edit e;
    verdict[r] = decode(Slice{image + records[2 * r], records[2 * r + 1]}, &e);
    if (verdict[r]) continue;
    for (uint32_t t = 0; t < kTypes; t++) {
      counts[1] += e.deleted[t].size();
      counts[0] += e.added[t].size();
      for (const File& f : e.added[t]) counts[2] += f.smallest.size() + f.largest.size();
    }
    h += digest(e);
  }
  return h;
}

uint32_t manifest_host_reencode(const uint8_t* rec, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  Edit e;
  const uint32_t code = decode(Slice{rec, len}, &e);
  out_len[0] = 0;
  if (code) return code;
  std::string s;
  encode(e, &s);
  out_len[0] = s.size();
  if (s.size() <= cap && !s.empty()) memcpy(out, s.data(), s.size());
  return 0;
}

uint64_t manifest_host_encode(const uint64_t* fields, const uint8_t* names, uint64_t n, const uint64_t* del_first,
                              const uint64_t* del_items, const uint64_t* new_first, const uint64_t* new_items,
                              const uint8_t* keys, const uint64_t* key_offsets, uint8_t* out, uint64_t cap,
                              uint64_t* records) {
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t* f = fields + i * kFieldWords;
    Edit e;  // built as SetComparatorName / Set* / DeleteFile / AddFile build it
    if (f[0] & 1) e.has_comparator = true, e.comparator.assign(reinterpret_cast<const char*>(names + f[11]), f[12]);
    if (f[0] & 2) e.has_log = true, e.log = f[2];
    if (f[0] & 4) e.has_prev_log = true, e.prev_log = f[3];
    if (f[0] & 8) e.has_next_file = true, e.next_file = f[4];
    if (f[0] & 16) e.has_last_seq = true, e.last_seq = f[5];
    e.write_cursor = f[6];
    for (uint32_t k = 0; k < kLevels; k++) e.read_cursor[k] = f[7 + k];
    for (uint64_t j = del_first[i]; j < del_first[i + 1]; j++) {
      const uint64_t* d = del_items + 4 * j;
      e.deleted[d[1] & 3].insert(std::make_pair((int)d[2], d[3]));
    }
    for (uint64_t j = new_first[i]; j < new_first[i + 1]; j++) {
      const uint64_t* a = new_items + 5 * j;
      const char* k = reinterpret_cast<const char*>(keys);
      File file = {(int)a[2], a[3], a[4], std::string(k + key_offsets[2 * j], k + key_offsets[2 * j + 1]),
                   std::string(k + key_offsets[2 * j + 1], k + key_offsets[2 * j + 2])};
      e.added[a[1] & 3].push_back(file);
    }
    std::string s;
    encode(e, &s);
    if (s.size() > cap - at) return 0;
    memcpy(out + at, s.data(), s.size());
    records[2 * i] = at;
    records[2 * i + 1] = s.size();
    at += s.size();
  }
  return at;
}

uint64_t manifest_host_recover(const uint8_t* image, const uint64_t* records, uint64_t n, uint64_t* numbers) {
  std::set<uint64_t> deleted[kLevels][kTypes];
  std::vector<File> added[kLevels][kTypes];
  numbers[0] = numbers[1] = numbers[2] = numbers[3] = 0;
  for (uint64_t r = 0; r < n; r++) {
    Edit e;
    const uint32_t code = decode(Slice{image + records[2 * r], records[2 * r + 1]}, &e);
    if (code) return UINT64_MAX - code;
    for (uint32_t t = 0; t < kTypes; t++) {  // Builder::Apply
      for (const auto& d : e.deleted[t]) deleted[d.first][t].insert(d.second);
      for (const File& f : e.added[t]) {
        deleted[f.level][t].erase(f.number);
        added[f.level][t].push_back(f);
      }
    }
    if (e.has_log) numbers[0] = e.log;
    if (e.has_prev_log) numbers[1] = e.prev_log;
    if (e.has_next_file) numbers[2] = e.next_file;
    if (e.has_last_seq) numbers[3] = e.last_seq;
  }
  uint64_t live = 0;
  for (uint32_t level = 0; level < kLevels; level++)
    for (uint32_t t = 0; t < kTypes; t++)
      for (const File& f : added[level][t]) live += deleted[level][t].count(f.number) == 0;  // MaybeAddFile
  return live;
}

}  // extern "C"

#ifdef MANIFEST_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

namespace {

uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rnd_state ^= rnd_state << 13;
  rnd_state ^= rnd_state >> 7;
  rnd_state ^= rnd_state << 17;
  return rnd_state;
}

void fail(const char* what, int i) {
  printf("manifest_host self-check FAILED: %s (%d)\n", what, i);
  exit(1);
}

}  // namespace

int main() {
  std::string all;
  for (int i = 0; i < 300; i++) {
    Edit e;
    if (rnd() & 1) e.has_comparator = true, e.comparator.assign(rnd() % 40, 'c');
    if (rnd() & 1) e.has_log = true, e.log = rnd() >> (rnd() % 64);
    if (rnd() & 1) e.has_prev_log = true, e.prev_log = rnd() >> (rnd() % 64);
    if (rnd() & 1) e.has_next_file = true, e.next_file = rnd() >> (rnd() % 64);
    if (rnd() & 1) e.has_last_seq = true, e.last_seq = rnd() >> (rnd() % 64);
    e.write_cursor = rnd() >> (rnd() % 64);
    for (uint32_t k = 0; k < kLevels; k++) e.read_cursor[k] = rnd() >> (rnd() % 64);
    for (uint64_t k = rnd() % 8; k; k--) e.deleted[rnd() % kTypes].insert(std::make_pair((int)(rnd() % kLevels), rnd() % 9));
    for (uint64_t k = rnd() % 8; k; k--) {
      File f = {(int)(rnd() % kLevels), rnd(), rnd() >> 20, std::string(rnd() % 50, 'a'), std::string(rnd() % 300, 'z')};
      e.added[rnd() % kTypes].push_back(f);
    }
    std::string s, again;
    encode(e, &s);
    std::vector<uint8_t> out(s.size() + 1);
    uint64_t out_len = 0;
    if (manifest_host_reencode(reinterpret_cast<const uint8_t*>(s.data()), s.size(), out.data(), out.size(), &out_len))
      fail("an encoded edit does not decode", i);
    if (out_len != s.size() || memcmp(out.data(), s.data(), s.size())) fail("decode then encode differs", i);
    if (i == 7) all = s;
    // every truncation, on a heap copy of exactly that size: a read past the end is the sanitizer's to find
    for (uint64_t cut = 0; cut < s.size() && i < 40; cut++) {
      std::vector<uint8_t> part(s.begin(), s.begin() + cut);
      Edit d;
      decode(Slice{part.data(), part.size()}, &d);
    }
  }
  const uint64_t recs[6] = {0, all.size(), all.size(), 0, 0, 3};
  uint32_t verdict[3];
  uint64_t counts[3], numbers[4];
  manifest_host_decode(reinterpret_cast<const uint8_t*>(all.data()), recs, 3, verdict, counts);
  if (verdict[0] != 0 || verdict[1] != 0) fail("verdicts", 0);
  manifest_host_recover(reinterpret_cast<const uint8_t*>(all.data()), recs, 2, numbers);
  printf("manifest_host self-check ok\n");
  return 0;
}
#endif
