// memtable_flush_host_check.cc -- the host-only half of BuildLevel0
// (lsbm_amd/csrc/memtable_flush_host.cc: staging layout, status mapping,
// window sums, filter-block layout, metaindex block, footer) driven from a
// stand-alone program, to be built with the host sanitizers (DESIGN.md
// section 16).  No device is touched.
//
//   cd lsbm_amd/csrc && g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I. -I../../include -o /tmp/flush_host_check ../../tools/memtable_flush_host_check.cc \
//       memtable_flush_host.cc status.cc bloom_host.cc && /tmp/flush_host_check
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include <cstring>
#include "memtable_flush_host.h"
#include "../../include/lsbm_memtable.h"
using namespace lsbm;
int main() {
  std::vector<std::string> recs = {"", std::string(12, 'a'), std::string(40000, 'b'), "x"};
  std::vector<uint64_t> pairs;
  assert(level0::LayoutRecords(recs, &pairs) == 40013 && pairs.size() == 8 && pairs[4] == 12 && pairs[7] == 1);
  std::vector<std::string> none;
  assert(level0::LayoutRecords(none, &pairs) == 0 && pairs.empty());
  for (uint32_t s = 0; s <= 9; s++) {
    Status st = level0::RecordStatus(s, s);
    assert(st.ok() == (s == LSBM_WB_OK));
    printf("%u %s\n", s, st.ToString().c_str());
  }
  uint64_t counts[] = {3, 10, 0, 0, 1, 0};
  std::vector<uint64_t> eb, kb;
  level0::Bases(counts, 3, &eb, &kb);
  assert(eb[3] == 4 && kb[3] == 10 + 24 + 8 && eb[2] == 3);
  level0::Bases(counts, 0, &eb, &kb);
  assert(eb.size() == 1 && kb.size() == 1);
  // filter layouts: no block, one block, blocks that cross several 2 KiB windows, a block past 4 GiB windows
  level0::FilterLayout fl;
  level0::LayoutFilterBlock(nullptr, nullptr, 0, 0, 10, &fl);
  assert(fl.filter_out.empty() && fl.trailer.size() == 5);
  uint64_t start[] = {0, 100, 2048, 9000}, first[] = {0, 5, 9, 9, 20};
  level0::LayoutFilterBlock(start, first, 4, 9100, 10, &fl);
  assert(fl.filter_first.front() == 0 && fl.filter_first.back() == 20 && fl.filter_out.size() + 1 == fl.filter_first.size());
  printf("filters %zu data %llu trailer %zu\n", fl.filter_out.size(), (unsigned long long)fl.data_bytes, fl.trailer.size());
  std::string m0 = level0::MetaindexBlock(false, 0, 0), m1 = level0::MetaindexBlock(true, 1ull << 40, 300);
  assert(m0.size() == 8 && m1.size() > 8 + 33);
  std::string f = level0::Footer(~0ull, ~0ull, ~0ull, ~0ull);
  assert(f.size() == 48);
  f = level0::Footer(1, 2, 3, 4);
  assert(f.size() == 48 && (unsigned char)f[47] == 0xdb);
  std::string v;
  level0::PutVarint64(&v, 0);
  level0::PutVarint64(&v, ~0ull);
  assert(v.size() == 11);
  puts("ok");
  return 0;
}
