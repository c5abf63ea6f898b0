// memtable_tool.cc -- drives include/lsbm/memtable_flush.h for
// tests/test_memtable_gpu.py.
//
//   memtable_tool <command file> <out>
//
// The command file is a sequence of blobs, each a u64 byte count and the bytes:
//   params (u64 block_size, restart_interval, bits_per_key + 1 (0: no filter),
//           paranoid, inject), then one blob per record.
// With inject != 0 a device fault is armed (lsbm_test_fail_host_pipeline) for
// the call.  Writes u64 max_sequence, u64 n_records, u64 status per record,
// then blobs file, smallest, largest as they are after the call (they start
// as "untouched").  Prints "status <Status::ToString()>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lsbm/memtable_flush.h"
#include "lsbm_crc32c.h"

static bool blob(FILE* f, std::string* s) {
  uint64_t n;
  if (fread(&n, 8, 1, f) != 1) return false;
  s->assign(n, '\0');
  if (n && fread(&(*s)[0], 1, n, f) != n) exit(3);
  return true;
}

static void put64(FILE* f, uint64_t v) { fwrite(&v, 8, 1, f); }
static void put_blob(FILE* f, const std::string& s) {
  put64(f, s.size());
  fwrite(s.data(), 1, s.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  std::string p;
  if (!blob(in, &p) || p.size() != 5 * 8) return 3;
  uint64_t params[5];
  memcpy(params, p.data(), sizeof(params));
  std::vector<std::string> records;
  std::string r;
  while (blob(in, &r)) records.push_back(r);
  fclose(in);
  lsbm::Level0Options opt;
  opt.block_size = params[0];
  opt.block_restart_interval = (uint32_t)params[1];
  opt.bits_per_key = (int)params[2] - 1;
  opt.paranoid_checks = params[3] != 0;
  std::string file = "untouched", smallest = "untouched", largest = "untouched";
  uint64_t max_sequence = 0;
  std::vector<uint32_t> status;
  if (params[4]) (void)lsbm_test_fail_host_pipeline(0);
  const lsbm::Status s = lsbm::BuildLevel0(0, records, opt, &file, &smallest, &largest, &max_sequence, &status);
  (void)lsbm_test_fail_host_pipeline(-1);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  put64(out, max_sequence);
  put64(out, status.size());
  for (uint32_t v : status) put64(out, v);
  put_blob(out, file);
  put_blob(out, smallest);
  put_blob(out, largest);
  fclose(out);
  printf("status %s\n", s.ToString().c_str());
  return 0;
}
