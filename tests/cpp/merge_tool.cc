// merge_tool.cc -- drives include/lsbm/compaction.h for tests/test_merge.py.
//
//   merge_tool merge <command file> <out>
//   merge_tool cut   <command file> <out>
//
// The command file is a sequence of blobs, each a u64 byte count and the bytes.
//   merge: params (u64 cmp, drop, smallest_snapshot, bottom_level), keys,
//          key_offsets (u64), values (u64 {offset, length}), run_first (u64)
//       writes u64 n_out, u64 n_runs, u64 status per run, source[n_out],
//       key_offsets[n_out + 1], values[2 n_out], then the key bytes
//   cut:   params (u64 max_file_size), block_first (u64), block_bytes (u64)
//       writes u64 n_tables, table_first[n_tables + 1], table_block_first[n_tables + 1]
// Prints "status <Status::ToString()>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lsbm/compaction.h"

static std::string blob(FILE* f) {
  uint64_t n;
  if (fread(&n, 8, 1, f) != 1) exit(3);
  std::string s(n, '\0');
  if (n && fread(&s[0], 1, n, f) != n) exit(3);
  return s;
}

static std::vector<uint64_t> u64s(const std::string& s) {
  std::vector<uint64_t> v(s.size() / 8);
  if (!v.empty()) memcpy(v.data(), s.data(), v.size() * 8);
  return v;
}

static void put64(FILE* f, uint64_t v) { fwrite(&v, 8, 1, f); }
static void put64s(FILE* f, const std::vector<uint64_t>& v) {
  if (!v.empty()) fwrite(v.data(), 8, v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  if (!in) return 2;
  const std::vector<uint64_t> params = u64s(blob(in));
  lsbm::Status s;
  if (!strcmp(argv[1], "cut")) {
    const std::vector<uint64_t> first = u64s(blob(in)), bytes = u64s(blob(in));
    fclose(in);
    if (params.size() != 1 || first.size() != bytes.size() + 1) return 3;
    std::vector<uint64_t> tf, tbf;
    s = lsbm::CutTables(first.data(), bytes.data(), bytes.size(), params[0], &tf, &tbf);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    put64(out, tf.size() - 1);
    put64s(out, tf);
    put64s(out, tbf);
    fclose(out);
  } else {
    const std::string keys = blob(in);
    const std::vector<uint64_t> koff = u64s(blob(in)), values = u64s(blob(in)), runs = u64s(blob(in));
    fclose(in);
    if (params.size() != 4 || koff.empty() || values.size() != 2 * (koff.size() - 1) || runs.empty()) return 3;
    const lsbm::BlockEntries en = {keys.data(), keys.size(), koff.data(), values.data(), nullptr, 0, koff.size() - 1};
    lsbm::MergeOptions opt;
    opt.cmp = params[0] ? lsbm::kInternalKeyComparator : lsbm::kBytewiseComparator;
    opt.drop = params[1] != 0;
    opt.smallest_snapshot = params[2];
    opt.bottom_level = params[3] != 0;
    std::string out_keys;
    std::vector<uint64_t> out_koff, out_values, source;
    std::vector<uint32_t> st;
    s = lsbm::MergeRuns(0, en, runs.data(), runs.size() - 1, opt, &out_keys, &out_koff, &out_values, &source, &st);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    put64(out, source.size());
    put64(out, st.size());
    for (uint32_t v : st) put64(out, v);
    put64s(out, source);
    put64s(out, out_koff);
    put64s(out, out_values);
    fwrite(out_keys.data(), 1, out_keys.size(), out);
    fclose(out);
  }
  printf("status %s\n", s.ToString().c_str());
  return 0;
}
