// block_tool.cc -- drives include/lsbm/block_reader.h for tests/test_block.py.
//
//   block_tool scan   <image> <handles u64>
//       prints "<entries> <key bytes> <value bytes> <status>" per block, then
//       "status <Status::ToString()>"
//   block_tool decode <image> <handles u64> <out>
//       writes per block: u64 n, then per entry u64 key length, value offset,
//       value length and the key bytes; prints "status ..."
//   block_tool seek   <image> <handles u64> <targets> <target offsets u64> <cmp> <out>
//       writes per query: u64 state, pos, key length, value offset, value
//       length and the found key's bytes; prints "status ..."
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lsbm/block_reader.h"

static std::string slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  std::string s;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
  fclose(f);
  return s;
}

static std::vector<uint64_t> slurp_u64(const char* path) {
  const std::string s = slurp(path);
  std::vector<uint64_t> v(s.size() / 8);
  memcpy(v.data(), s.data(), v.size() * 8);
  return v;
}

static void put64(FILE* f, uint64_t v) { fwrite(&v, 8, 1, f); }

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string mode = argv[1];
  const std::string image = slurp(argv[2]);
  const std::vector<uint64_t> handles = slurp_u64(argv[3]);
  const size_t n = handles.size() / 2;
  lsbm::Status s;
  if (mode == "scan") {
    std::vector<lsbm::BlockCounts> counts;
    std::vector<uint32_t> st;
    s = lsbm::ScanBlocks(0, image.data(), image.size(), handles.data(), n, &counts, &st);
    if (counts.size() != n || st.size() != n) return 3;
    for (size_t i = 0; i < n; i++)
      printf("%llu %llu %llu %u\n", (unsigned long long)counts[i].entries, (unsigned long long)counts[i].key_bytes,
             (unsigned long long)counts[i].value_bytes, st[i]);
  } else if (mode == "decode" && argc == 5) {
    std::string keys;
    std::vector<uint64_t> koff, values, first;
    std::vector<uint32_t> st;
    s = lsbm::DecodeBlocks(0, image.data(), image.size(), handles.data(), n, &keys, &koff, &values, &first, &st);
    if (first.size() != n + 1) return 3;
    FILE* f = fopen(argv[4], "wb");
    for (size_t i = 0; i < n; i++) {
      put64(f, first[i + 1] - first[i]);
      for (uint64_t e = first[i]; e < first[i + 1]; e++) {
        put64(f, koff[e + 1] - koff[e]);
        put64(f, values[2 * e]);
        put64(f, values[2 * e + 1]);
        fwrite(keys.data() + koff[e], 1, koff[e + 1] - koff[e], f);
      }
    }
    fclose(f);
  } else if (mode == "seek" && argc == 8) {
    const std::string targets = slurp(argv[4]);
    const std::vector<uint64_t> toff = slurp_u64(argv[5]);
    if (toff.size() != n + 1) return 3;
    std::vector<lsbm::SeekResult> res;
    std::vector<std::string> found;
    s = lsbm::SeekBlocks(0, image.data(), image.size(), handles.data(), targets.data(), toff.data(), n,
                         atoi(argv[6]) ? lsbm::kInternalKeyComparator : lsbm::kBytewiseComparator, false, &res,
                         &found);
    if (res.size() != n || found.size() != n) return 3;
    FILE* f = fopen(argv[7], "wb");
    for (size_t q = 0; q < n; q++) {
      put64(f, res[q].state);
      put64(f, res[q].pos);
      put64(f, res[q].key_len);
      put64(f, res[q].value_offset);
      put64(f, res[q].value_size);
      if (found[q].size() != res[q].key_len) return 4;
      fwrite(found[q].data(), 1, found[q].size(), f);
    }
    fclose(f);
  } else {
    return 2;
  }
  printf("status %s\n", s.ToString().c_str());
  return 0;
}
