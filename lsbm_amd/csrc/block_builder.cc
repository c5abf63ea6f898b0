// block_builder.cc -- include/lsbm/block_builder.h on top of the C ABI
// (include/lsbm_block_build.h).  The entries go to the device once through the
// device's HostSession (host_session.h), the blocks are planned or built
// there, and only the results come back.  The layer sizes its own windows: a
// first launch with empty windows reports every block's true size, a second
// one builds into windows of exactly that size.
#include "../../include/lsbm/block_builder.h"

#include <hip/hip_runtime_api.h>
#include <string.h>

#include "../../include/lsbm_block_build.h"
#include "../../include/lsbm_crc32c.h"
#include "host_staging.h"

namespace lsbm {

namespace {

Status build_status(uint32_t s) {
  switch (s) {
    case LSBM_BUILD_OK: return Status::OK();
    case LSBM_BUILD_BAD_INPUT: return Status::InvalidArgument("bad block builder input");
    case LSBM_BUILD_TOO_LARGE: return Status::InvalidArgument("block would reach 2^32 bytes");
    default: return Status::IOError("internal error: block window too small");
  }
}

Status first_failure(const std::vector<uint32_t>& statuses) {
  for (uint32_t s : statuses)
    if (s != LSBM_BUILD_OK) return build_status(s);
  return Status::OK();
}

struct Staged {
  uint8_t* keys;
  uint64_t* key_offsets;
  uint64_t* values;
  uint8_t* image;
};

// the entries on the device (scratch 0, 1 and 2)
Status stage_entries(Staging& st, const BlockEntries& en, bool with_values, Staged* d) {
  if (!en.key_offsets || (!en.keys && en.keys_size) || (!en.values && en.n) ||
      (with_values && !en.value_image && en.value_image_size))
    return Status::InvalidArgument("null pointer");
  Packed in;  // one buffer: key_offsets[n+1] values[2n]
  const auto f_off = in.add<uint64_t>(en.n + 1), f_val = in.add<uint64_t>(2 * en.n);
  d->keys = st.buf<uint8_t>(0, en.keys_size);
  uint8_t* d_in = st.buf<uint8_t>(1, in.bytes());
  d->key_offsets = f_off.in(d_in);
  d->values = f_val.in(d_in);
  d->image = with_values ? st.buf<uint8_t>(2, en.value_image_size) : nullptr;
  st.put(d->keys, en.keys, en.keys_size);
  st.put(d->key_offsets, en.key_offsets, en.n + 1);
  st.put(d->values, en.values, 2 * en.n);
  if (with_values) st.put(d->image, en.value_image, en.value_image_size);
  return st.ok() ? Status::OK() : st.status("staging");
}

// windows of exactly the reported sizes, back to back
void pack(const std::vector<uint64_t>& sizes, std::vector<uint64_t>* offsets, std::vector<uint64_t>* handles) {
  const size_t n = sizes.size();
  offsets->assign(n + 1, 0);
  handles->assign(2 * n, 0);
  for (size_t i = 0; i < n; i++) {
    (*handles)[2 * i] = (*offsets)[i];
    (*handles)[2 * i + 1] = sizes[i];
    (*offsets)[i + 1] = (*offsets)[i] + sizes[i];
  }
}

}  // namespace

Status PlanBlocks(int device, const BlockEntries& en, const uint64_t* table_first, size_t n_tables,
                  uint64_t block_size, uint32_t restart_interval, std::vector<uint64_t>* block_first,
                  std::vector<uint64_t>* block_bytes, std::vector<uint64_t>* table_block_first,
                  std::vector<uint32_t>* statuses) {
  if (!block_first || !block_bytes || !table_block_first || !statuses || !table_first)
    return Status::InvalidArgument("null pointer");
  if (restart_interval == 0 || block_size == 0) return Status::InvalidArgument("block_size and restart_interval must be at least 1");
  Staging st;
  Status s = st.Open(device);
  if (!s.ok()) return s;
  Staged d;
  s = stage_entries(st, en, false, &d);
  if (!s.ok()) return s;
  // a block holds at least one entry: n blocks at the most
  const uint64_t cap = en.n, scratch_bytes = lsbm_block_plan_scratch_bytes(en.n, n_tables);
  Packed res;  // one buffer: block_first[cap+1] block_bytes[cap] table_block_first[T+1] (u64) status[T] (u32)
  const auto f_bf = res.add<uint64_t>(cap + 1), f_bb = res.add<uint64_t>(cap), f_tbf = res.add<uint64_t>(n_tables + 1);
  const auto f_st = res.add<uint32_t>(n_tables);
  uint64_t* d_tf = st.buf<uint64_t>(3, n_tables + 1);
  uint8_t* d_out = st.buf<uint8_t>(4, res.bytes());
  uint8_t* d_scratch = st.buf<uint8_t>(5, scratch_bytes);
  st.put(d_tf, table_first, n_tables + 1);
  if (!st.ok()) return st.status("staging");
  if (lsbm_block_plan_dev(d.keys, en.keys_size, d.key_offsets, d.values, en.n, d_tf, n_tables, block_size,
                          restart_interval, f_bf.in(d_out), f_bb.in(d_out), cap, f_tbf.in(d_out), f_st.in(d_out),
                          d_scratch, scratch_bytes, st.stream()) != LSBM_OK)
    return Status::InvalidArgument(lsbm_crc32c_last_error());
  std::vector<uint8_t> out(res.bytes());
  st.get(out.data(), d_out, res.bytes());
  if (!st.ok()) return st.status("block plan");
  const uint64_t *bf = f_bf.in(out.data()), *bb = f_bb.in(out.data()), *tbf = f_tbf.in(out.data());
  table_block_first->assign(tbf, tbf + n_tables + 1);
  const uint64_t total = table_block_first->back();
  if (total > cap) return Status::IOError("internal error: more blocks than entries");
  block_first->assign(bf, bf + total + 1);
  block_bytes->assign(bb, bb + total);
  statuses->assign(f_st.in(out.data()), f_st.in(out.data()) + n_tables);
  return first_failure(*statuses);
}

Status BuildBlocks(int device, const BlockEntries& en, const uint64_t* block_first, size_t n_blocks,
                   uint32_t restart_interval, std::string* out, std::vector<uint64_t>* block_offsets,
                   std::vector<uint32_t>* statuses) {
  if (!out || !block_offsets || !statuses) return Status::InvalidArgument("null pointer");
  out->clear();
  block_offsets->assign(1, 0);
  statuses->clear();
  if (restart_interval == 0) return Status::InvalidArgument("restart_interval must be at least 1");
  if (n_blocks == 0) return Status::OK();
  if (!block_first) return Status::InvalidArgument("null pointer");
  Staging st;
  Status s = st.Open(device);
  if (!s.ok()) return s;
  Staged d;
  s = stage_entries(st, en, true, &d);
  if (!s.ok()) return s;
  Packed in, res;  // two buffers: block_first[n+1] handles[2n] | built[n] (u64) status[n] (u32)
  const auto f_bf = in.add<uint64_t>(n_blocks + 1), f_handles = in.add<uint64_t>(2 * n_blocks);
  const auto f_built = res.add<uint64_t>(n_blocks);
  const auto f_st = res.add<uint32_t>(n_blocks);
  uint8_t* d_in = st.buf<uint8_t>(3, in.bytes());
  uint8_t* d_res = st.buf<uint8_t>(4, res.bytes());
  uint8_t* d_out = st.buf<uint8_t>(5, 1);
  if (!st.ok()) return st.status("staging");
  std::vector<uint64_t> built(n_blocks, 0), handles(2 * n_blocks, 0);
  statuses->assign(n_blocks, 0);
  uint64_t total = 0;
  st.put(f_bf.in(d_in), block_first, n_blocks + 1);
  // pass 0: empty windows, the true sizes; pass 1: windows of those sizes
  for (int pass = 0; pass < 2 && st.ok(); pass++) {
    st.put(f_handles.in(d_in), handles.data(), 2 * n_blocks);
    if (!st.ok()) break;
    if (lsbm_block_build_dev(d.keys, en.keys_size, d.key_offsets, d.values, d.image, en.value_image_size, en.n,
                             f_bf.in(d_in), n_blocks, restart_interval, d_out, total, f_handles.in(d_in),
                             f_built.in(d_res), f_st.in(d_res), st.stream()) != LSBM_OK)
      return Status::InvalidArgument(lsbm_crc32c_last_error());
    st.get(built.data(), f_built.in(d_res), n_blocks);
    st.get(statuses->data(), f_st.in(d_res), n_blocks);
    if (!st.ok() || pass == 1) break;
    pack(built, block_offsets, &handles);
    total = block_offsets->back();
    d_out = st.buf<uint8_t>(5, total);
  }
  if (!st.ok()) return st.status("block build");
  out->assign(total, '\0');
  st.get(&(*out)[0], d_out, total);
  if (!st.ok()) return st.status("block build");
  return first_failure(*statuses);
}

Status BuildIndexBlocks(int device, const BlockEntries& en, const uint64_t* block_first, size_t n_blocks,
                        const uint64_t* table_block_first, size_t n_tables, const uint64_t* data_handles,
                        BlockComparator cmp, std::string* out, std::vector<uint64_t>* block_offsets,
                        std::vector<uint32_t>* statuses) {
  if (!out || !block_offsets || !statuses) return Status::InvalidArgument("null pointer");
  out->clear();
  block_offsets->assign(1, 0);
  statuses->clear();
  if (cmp != kBytewiseComparator && cmp != kInternalKeyComparator) return Status::InvalidArgument("unknown comparator");
  if (n_tables == 0) return Status::OK();
  if (!block_first || !table_block_first || (!data_handles && n_blocks)) return Status::InvalidArgument("null pointer");
  Staging st;
  Status s = st.Open(device);
  if (!s.ok()) return s;
  Staged d;
  BlockEntries keys_only = en;
  keys_only.value_image = nullptr;
  keys_only.value_image_size = 0;
  s = stage_entries(st, keys_only, false, &d);
  if (!s.ok()) return s;
  // two buffers: block_first[nb+1] data_handles[2nb] table_block_first[T+1] out_handles[2T] | built[T] status[T]
  Packed in, res;
  const auto f_bf = in.add<uint64_t>(n_blocks + 1), f_dh = in.add<uint64_t>(2 * n_blocks);
  const auto f_tbf = in.add<uint64_t>(n_tables + 1), f_oh = in.add<uint64_t>(2 * n_tables);
  const auto f_built = res.add<uint64_t>(n_tables);
  const auto f_st = res.add<uint32_t>(n_tables);
  uint8_t* d_in = st.buf<uint8_t>(3, in.bytes());
  uint8_t* d_res = st.buf<uint8_t>(4, res.bytes());
  uint8_t* d_out = nullptr;
  if (!st.ok()) return st.status("staging");
  st.put(f_bf.in(d_in), block_first, n_blocks + 1);
  st.put(f_dh.in(d_in), data_handles, 2 * n_blocks);
  st.put(f_tbf.in(d_in), table_block_first, n_tables + 1);
  std::vector<uint64_t> built(n_tables, 0), handles;
  statuses->assign(n_tables, 0);
  uint64_t total = 0;
  // pass 0: sizes only; pass 1: windows of those sizes
  for (int pass = 0; pass < 2 && st.ok(); pass++) {
    if (lsbm_index_block_build_dev(d.keys, en.keys_size, d.key_offsets, en.n, f_bf.in(d_in), n_blocks, f_tbf.in(d_in),
                                   n_tables, f_dh.in(d_in), (int)cmp, d_out, total, pass ? f_oh.in(d_in) : nullptr,
                                   f_built.in(d_res), f_st.in(d_res), st.stream()) != LSBM_OK)
      return Status::InvalidArgument(lsbm_crc32c_last_error());
    st.get(built.data(), f_built.in(d_res), n_tables);
    st.get(statuses->data(), f_st.in(d_res), n_tables);
    if (!st.ok() || pass == 1) break;
    pack(built, block_offsets, &handles);
    total = block_offsets->back();
    d_out = st.buf<uint8_t>(5, total);
    st.put(f_oh.in(d_in), handles.data(), 2 * n_tables);
  }
  if (!st.ok()) return st.status("index block build");
  out->assign(total, '\0');
  st.get(&(*out)[0], d_out, total);
  if (!st.ok()) return st.status("index block build");
  return first_failure(*statuses);
}

}  // namespace lsbm
