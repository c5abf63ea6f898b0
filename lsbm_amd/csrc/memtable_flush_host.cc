// memtable_flush_host.cc -- memtable_flush_host.h.  No device code.
#include "memtable_flush_host.h"

#include <string.h>

#include "../../include/lsbm_bloom.h"     // lsbm_bloom_filter_bytes, LSBM_FILTER_BASE_LG
#include "../../include/lsbm_memtable.h"  // LSBM_WB_*

namespace lsbm {
namespace level0 {

uint64_t LayoutRecords(const std::vector<std::string>& records, std::vector<uint64_t>* pairs) {
  pairs->assign(2 * records.size(), 0);
  uint64_t at = 0;
  for (size_t i = 0; i < records.size(); i++) {
    (*pairs)[2 * i] = at;
    (*pairs)[2 * i + 1] = records[i].size();
    at += records[i].size();
  }
  return at;
}

Status RecordStatus(uint32_t wb_status, size_t record) {
  const std::string where = " (record " + std::to_string(record) + ")";
  switch (wb_status) {
    case LSBM_WB_OK: return Status::OK();
    case LSBM_WB_TOO_SMALL: return Status::Corruption("log record too small" + where);
    case LSBM_WB_BAD_PUT: return Status::Corruption("bad WriteBatch Put" + where);
    case LSBM_WB_BAD_DELETE: return Status::Corruption("bad WriteBatch Delete" + where);
    case LSBM_WB_UNKNOWN_TAG: return Status::Corruption("unknown WriteBatch tag" + where);
    case LSBM_WB_WRONG_COUNT: return Status::Corruption("WriteBatch has wrong count" + where);
    case LSBM_WB_BAD_INPUT: return Status::InvalidArgument("record of 4 GiB or more" + where);
    default: return Status::IOError("internal error: record window too small" + where);
  }
}

void Bases(const uint64_t* counts, size_t n_records, std::vector<uint64_t>* entry_base,
           std::vector<uint64_t>* key_base) {
  entry_base->assign(n_records + 1, 0);
  key_base->assign(n_records + 1, 0);
  for (size_t i = 0; i < n_records; i++) {
    (*entry_base)[i + 1] = (*entry_base)[i] + counts[2 * i];
    (*key_base)[i + 1] = (*key_base)[i] + counts[2 * i + 1] + 8 * counts[2 * i];
  }
}

void PutVarint64(std::string* dst, uint64_t v) {
  while (v >= 128) {
    dst->push_back(static_cast<char>((v & 127) | 128));
    v >>= 7;
  }
  dst->push_back(static_cast<char>(v));
}

namespace {

void put_fixed32(std::string* dst, uint32_t v) {
  char b[4];
  memcpy(b, &v, 4);
  dst->append(b, 4);
}

}  // namespace

void LayoutFilterBlock(const uint64_t* block_start, const uint64_t* block_first, size_t n_blocks, uint64_t end,
                       int bits_per_key, FilterLayout* out) {
  out->filter_first.clear();
  out->filter_out.clear();
  out->data_bytes = 0;
  out->trailer.clear();
  std::vector<uint32_t> offsets;  // filter_offsets_
  uint64_t lo = n_blocks ? block_first[0] : 0, hi = lo;  // the pending keys
  auto generate = [&]() {  // GenerateFilter
    offsets.push_back((uint32_t)out->data_bytes);
    if (hi > lo) {
      if (out->filter_first.empty()) out->filter_first.push_back(lo);
      out->filter_first.push_back(hi);
      out->filter_out.push_back(out->data_bytes);
      out->data_bytes += lsbm_bloom_filter_bytes(hi - lo, bits_per_key);
      lo = hi;
    }
  };
  for (size_t b = 0; b < n_blocks; b++) {
    while ((block_start[b] >> LSBM_FILTER_BASE_LG) > offsets.size()) generate();  // StartBlock
    hi = block_first[b + 1];                                                        // AddKey for the block's keys
  }
  if (n_blocks)
    while ((end >> LSBM_FILTER_BASE_LG) > offsets.size()) generate();  // the last Flush's StartBlock
  if (hi > lo) generate();                                             // Finish
  for (uint32_t o : offsets) put_fixed32(&out->trailer, o);
  put_fixed32(&out->trailer, (uint32_t)out->data_bytes);
  out->trailer.push_back((char)LSBM_FILTER_BASE_LG);
}

std::string MetaindexBlock(bool with_filter, uint64_t filter_offset, uint64_t filter_size) {
  std::string b;
  if (with_filter) {
    static const char kKey[] = "filter.leveldb.BuiltinBloomFilter";
    std::string handle;
    PutVarint64(&handle, filter_offset);
    PutVarint64(&handle, filter_size);
    PutVarint64(&b, 0);  // shared
    PutVarint64(&b, sizeof(kKey) - 1);
    PutVarint64(&b, handle.size());
    b.append(kKey, sizeof(kKey) - 1);
    b += handle;
  }
  put_fixed32(&b, 0);  // the one restart point
  put_fixed32(&b, 1);
  return b;
}

std::string Footer(uint64_t meta_offset, uint64_t meta_size, uint64_t index_offset, uint64_t index_size) {
  std::string f;
  PutVarint64(&f, meta_offset);
  PutVarint64(&f, meta_size);
  PutVarint64(&f, index_offset);
  PutVarint64(&f, index_size);
  f.resize(40, '\0');
  const uint64_t magic = 0xdb4775248b80fb57ull;  // table/format.h:81
  char b[8];
  memcpy(b, &magic, 8);
  f.append(b, 8);
  return f;
}

}  // namespace level0
}  // namespace lsbm
