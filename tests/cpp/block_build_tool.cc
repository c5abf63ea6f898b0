// block_build_tool.cc -- drives include/lsbm/block_builder.h for
// tests/test_block_build_gpu.py.
//
//   block_build_tool <command file> <out>
//
// The command file is a sequence of blobs, each a u64 byte count and the
// bytes: params (u64 mode, block_size, restart_interval, cmp), keys,
// key_offsets (u64), values (u64 {offset, length}), value image, and three
// u64 arrays a, b, c whose meaning depends on the mode:
//   mode 0 plan    a = table_first
//       writes u64 n_blocks, block_first[n_blocks + 1], block_bytes[n_blocks],
//       table_block_first[n_tables + 1], u64 status per table
//   mode 1 build   a = block_first
//   mode 2 index   a = block_first, b = table_block_first, c = data_handles
//       write u64 n, offsets[n + 1], u64 status per block, then the blocks'
//       bytes back to back
// Prints "status <Status::ToString()>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lsbm/block_builder.h"

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
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<uint64_t> params = u64s(blob(in));
  const std::string keys = blob(in);
  const std::vector<uint64_t> koff = u64s(blob(in)), values = u64s(blob(in));
  const std::string image = blob(in);
  const std::vector<uint64_t> a = u64s(blob(in)), b = u64s(blob(in)), c = u64s(blob(in));
  fclose(in);
  if (params.size() != 4 || koff.empty() || values.size() != 2 * (koff.size() - 1) || a.empty()) return 3;
  const lsbm::BlockEntries en = {keys.data(), keys.size(), koff.data(), values.data(),
                                 image.data(), image.size(), koff.size() - 1};
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  lsbm::Status s;
  std::vector<uint32_t> st;
  if (params[0] == 0) {
    std::vector<uint64_t> first, bytes, tbf;
    s = lsbm::PlanBlocks(0, en, a.data(), a.size() - 1, params[1], (uint32_t)params[2], &first, &bytes, &tbf, &st);
    put64(out, bytes.size());
    put64s(out, first);
    put64s(out, bytes);
    put64s(out, tbf);
    for (uint32_t v : st) put64(out, v);
  } else {
    std::string bytes;
    std::vector<uint64_t> offs;
    if (params[0] == 1) {
      s = lsbm::BuildBlocks(0, en, a.data(), a.size() - 1, (uint32_t)params[2], &bytes, &offs, &st);
    } else {
      if (b.empty() || c.size() != 2 * (a.size() - 1)) return 3;
      s = lsbm::BuildIndexBlocks(0, en, a.data(), a.size() - 1, b.data(), b.size() - 1, c.data(),
                                 params[3] ? lsbm::kInternalKeyComparator : lsbm::kBytewiseComparator, &bytes, &offs,
                                 &st);
    }
    put64(out, st.size());
    put64s(out, offs);
    for (uint32_t v : st) put64(out, v);
    fwrite(bytes.data(), 1, bytes.size(), out);
  }
  fclose(out);
  printf("status %s\n", s.ToString().c_str());
  return 0;
}
