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
#include "host_session.h"

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
Status stage_entries(SessionLease& ss, const BlockEntries& en, bool with_values, Staged* d) {
  if (!en.key_offsets || (!en.keys && en.keys_size) || (!en.values && en.n) ||
      (with_values && !en.value_image && en.value_image_size))
    return Status::InvalidArgument("null pointer");
  void *k, *o, *img = nullptr;
  const size_t off_bytes = (en.n + 1) * sizeof(uint64_t), val_bytes = 2 * en.n * sizeof(uint64_t);
  hipError_t e = ss->scratch(0, en.keys_size ? en.keys_size : 1, &k);
  if (e == hipSuccess) e = ss->scratch(1, off_bytes + val_bytes, &o);
  if (e == hipSuccess && with_values) e = ss->scratch(2, en.value_image_size ? en.value_image_size : 1, &img);
  if (e == hipSuccess && en.keys_size) e = ss->upload(k, en.keys, en.keys_size);
  if (e == hipSuccess) e = ss->upload(o, en.key_offsets, off_bytes);
  if (e == hipSuccess && en.n) e = ss->upload(static_cast<uint8_t*>(o) + off_bytes, en.values, val_bytes);
  if (e == hipSuccess && with_values && en.value_image_size) e = ss->upload(img, en.value_image, en.value_image_size);
  if (e != hipSuccess) return hip_status(e, "staging");
  d->keys = static_cast<uint8_t*>(k);
  d->key_offsets = static_cast<uint64_t*>(o);
  d->values = d->key_offsets + (en.n + 1);
  d->image = static_cast<uint8_t*>(img);
  return Status::OK();
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
  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  Staged d;
  s = stage_entries(ss, en, false, &d);
  if (!s.ok()) return s;
  // a block holds at least one entry: n blocks at the most
  const uint64_t cap = en.n, scratch_bytes = lsbm_block_plan_scratch_bytes(en.n, n_tables);
  // one buffer: table_first[T+1] | block_first[cap+1] block_bytes[cap] table_block_first[T+1] (u64) status[T] (u32)
  const size_t in_bytes = (n_tables + 1) * sizeof(uint64_t);
  const size_t out_bytes = (2 * cap + n_tables + 2) * sizeof(uint64_t) + n_tables * sizeof(uint32_t);
  void *d_in, *d_out, *d_scratch;
  hipError_t e = ss->scratch(3, in_bytes, &d_in);
  if (e == hipSuccess) e = ss->scratch(4, out_bytes, &d_out);
  if (e == hipSuccess) e = ss->scratch(5, scratch_bytes, &d_scratch);
  if (e == hipSuccess) e = ss->upload(d_in, table_first, in_bytes);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint64_t* d_bf = static_cast<uint64_t*>(d_out);
  uint64_t *d_bb = d_bf + cap + 1, *d_tbf = d_bb + cap;
  uint32_t* d_st = reinterpret_cast<uint32_t*>(d_tbf + n_tables + 1);
  if (lsbm_block_plan_dev(d.keys, en.keys_size, d.key_offsets, d.values, en.n, static_cast<const uint64_t*>(d_in),
                          n_tables, block_size, restart_interval, d_bf, d_bb, cap, d_tbf, d_st, d_scratch,
                          scratch_bytes, ss->stream()) != LSBM_OK)
    return Status::InvalidArgument(lsbm_crc32c_last_error());
  std::vector<uint8_t> out(out_bytes);
  e = ss->download(out.data(), d_out, out_bytes);
  if (e != hipSuccess) return hip_status(e, "block plan");
  const uint64_t* o = reinterpret_cast<const uint64_t*>(out.data());
  table_block_first->assign(o + 2 * cap + 1, o + 2 * cap + 1 + n_tables + 1);
  const uint64_t total = table_block_first->back();
  if (total > cap) return Status::IOError("internal error: more blocks than entries");
  block_first->assign(o, o + total + 1);
  block_bytes->assign(o + cap + 1, o + cap + 1 + total);
  statuses->resize(n_tables);
  if (n_tables) memcpy(statuses->data(), o + 2 * cap + n_tables + 2, n_tables * sizeof(uint32_t));
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
  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  Staged d;
  s = stage_entries(ss, en, true, &d);
  if (!s.ok()) return s;
  // one buffer: block_first[n+1] handles[2n] | built[n] (u64) status[n] (u32)
  const size_t in_bytes = (3 * n_blocks + 1) * sizeof(uint64_t);
  const size_t res_bytes = n_blocks * (sizeof(uint64_t) + sizeof(uint32_t));
  void *d_in, *d_res, *d_out;
  hipError_t e = ss->scratch(3, in_bytes, &d_in);
  if (e == hipSuccess) e = ss->scratch(4, res_bytes, &d_res);
  if (e == hipSuccess) e = ss->scratch(5, 1, &d_out);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint64_t* d_bf = static_cast<uint64_t*>(d_in);
  uint64_t* d_handles = d_bf + n_blocks + 1;
  uint64_t* d_built = static_cast<uint64_t*>(d_res);
  uint32_t* d_st = reinterpret_cast<uint32_t*>(d_built + n_blocks);
  std::vector<uint64_t> built(n_blocks, 0), handles(2 * n_blocks, 0);
  statuses->assign(n_blocks, 0);
  uint64_t total = 0;
  e = ss->upload(d_bf, block_first, (n_blocks + 1) * sizeof(uint64_t));
  // pass 0: empty windows, the true sizes; pass 1: windows of those sizes
  for (int pass = 0; pass < 2 && e == hipSuccess; pass++) {
    e = ss->upload(d_handles, handles.data(), 2 * n_blocks * sizeof(uint64_t));
    if (e != hipSuccess) break;
    if (lsbm_block_build_dev(d.keys, en.keys_size, d.key_offsets, d.values, d.image, en.value_image_size, en.n, d_bf,
                             n_blocks, restart_interval, static_cast<uint8_t*>(d_out), total, d_handles, d_built, d_st,
                             ss->stream()) != LSBM_OK)
      return Status::InvalidArgument(lsbm_crc32c_last_error());
    e = ss->download(built.data(), d_built, n_blocks * sizeof(uint64_t));
    if (e == hipSuccess) e = ss->download(statuses->data(), d_st, n_blocks * sizeof(uint32_t));
    if (e != hipSuccess || pass == 1) break;
    pack(built, block_offsets, &handles);
    total = block_offsets->back();
    e = ss->scratch(5, total ? total : 1, &d_out);
  }
  if (e != hipSuccess) return hip_status(e, "block build");
  out->assign(total, '\0');
  if (total) e = ss->download(&(*out)[0], d_out, total);
  if (e != hipSuccess) return hip_status(e, "block build");
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
  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  Staged d;
  BlockEntries keys_only = en;
  keys_only.value_image = nullptr;
  keys_only.value_image_size = 0;
  s = stage_entries(ss, keys_only, false, &d);
  if (!s.ok()) return s;
  // one buffer: block_first[nb+1] data_handles[2nb] table_block_first[T+1] out_handles[2T] | built[T] status[T]
  const size_t in_words = 3 * n_blocks + 1 + 3 * n_tables + 1;
  const size_t res_bytes = n_tables * (sizeof(uint64_t) + sizeof(uint32_t));
  void *d_in, *d_res, *d_out = nullptr;
  hipError_t e = ss->scratch(3, in_words * sizeof(uint64_t), &d_in);
  if (e == hipSuccess) e = ss->scratch(4, res_bytes, &d_res);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint64_t* d_bf = static_cast<uint64_t*>(d_in);
  uint64_t *d_dh = d_bf + n_blocks + 1, *d_tbf = d_dh + 2 * n_blocks, *d_oh = d_tbf + n_tables + 1;
  uint64_t* d_built = static_cast<uint64_t*>(d_res);
  uint32_t* d_st = reinterpret_cast<uint32_t*>(d_built + n_tables);
  e = ss->upload(d_bf, block_first, (n_blocks + 1) * sizeof(uint64_t));
  if (e == hipSuccess && n_blocks) e = ss->upload(d_dh, data_handles, 2 * n_blocks * sizeof(uint64_t));
  if (e == hipSuccess) e = ss->upload(d_tbf, table_block_first, (n_tables + 1) * sizeof(uint64_t));
  std::vector<uint64_t> built(n_tables, 0), handles;
  statuses->assign(n_tables, 0);
  uint64_t total = 0;
  // pass 0: sizes only; pass 1: windows of those sizes
  for (int pass = 0; pass < 2 && e == hipSuccess; pass++) {
    if (lsbm_index_block_build_dev(d.keys, en.keys_size, d.key_offsets, en.n, d_bf, n_blocks, d_tbf, n_tables, d_dh,
                                   (int)cmp, static_cast<uint8_t*>(d_out), total, pass ? d_oh : nullptr, d_built, d_st,
                                   ss->stream()) != LSBM_OK)
      return Status::InvalidArgument(lsbm_crc32c_last_error());
    e = ss->download(built.data(), d_built, n_tables * sizeof(uint64_t));
    if (e == hipSuccess) e = ss->download(statuses->data(), d_st, n_tables * sizeof(uint32_t));
    if (e != hipSuccess || pass == 1) break;
    pack(built, block_offsets, &handles);
    total = block_offsets->back();
    e = ss->scratch(5, total ? total : 1, &d_out);
    if (e == hipSuccess) e = ss->upload(d_oh, handles.data(), 2 * n_tables * sizeof(uint64_t));
  }
  if (e != hipSuccess) return hip_status(e, "index block build");
  out->assign(total, '\0');
  if (total) e = ss->download(&(*out)[0], d_out, total);
  if (e != hipSuccess) return hip_status(e, "index block build");
  return first_failure(*statuses);
}

}  // namespace lsbm
