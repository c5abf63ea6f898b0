// block_reader.cc -- include/lsbm/block_reader.h on top of the C ABI
// (include/lsbm_block.h).  The image goes to the device once through the
// device's HostSession (host_session.h), the blocks are walked there, and
// only the per-block results and the decoded keys come back.  The statuses'
// mapping to the reference's messages runs on the host.
#include "../../include/lsbm/block_reader.h"

#include <hip/hip_runtime_api.h>
#include <string.h>

#include "../../include/lsbm_block.h"
#include "../../include/lsbm_crc32c.h"
#include "host_staging.h"

namespace lsbm {

namespace {

Status block_status(uint32_t s) {
  switch (s) {
    case LSBM_BLOCK_OK: return Status::OK();
    case LSBM_BLOCK_BAD_CONTENTS: return Status::Corruption("bad block contents");
    case LSBM_BLOCK_BAD_ENTRY: return Status::Corruption("bad entry in block");
    default: return Status::IOError("block window too small");
  }
}

Status seek_status(uint32_t s) {
  switch (s) {
    case LSBM_SEEK_BAD_ENTRY: return Status::Corruption("bad entry in block");
    case LSBM_SEEK_BAD_CONTENTS: return Status::Corruption("bad block contents");
    case LSBM_SEEK_BAD_HANDLE: return Status::Corruption("bad block handle");
    default: return Status::OK();
  }
}

struct Image {
  uint8_t* image;
  uint64_t* handles;
};

// image and handles on the device (scratch 0 and 1)
Image stage_image(Staging& st, const char* image, size_t image_size, const uint64_t* handles, size_t n) {
  const Image d = {st.buf<uint8_t>(0, image_size), st.buf<uint64_t>(1, 2 * n)};
  st.put(d.image, image, image_size);
  st.put(d.handles, handles, 2 * n);
  return d;
}

// lsbm_block_scan_dev into host vectors (scratch 2 and 3)
Status scan_staged(Staging& st, const Image& d, size_t image_size, size_t n, std::vector<uint64_t>* counts,
                   std::vector<uint32_t>* statuses) {
  uint64_t* d_counts = st.buf<uint64_t>(2, 3 * n);
  uint32_t* d_status = st.buf<uint32_t>(3, n);
  if (!st.ok()) return st.status("staging");
  if (lsbm_block_scan_dev(d.image, image_size, d.handles, n, d_counts, d_status, st.stream()) != LSBM_OK)
    return Status::IOError(lsbm_crc32c_last_error());
  counts->resize(3 * n);
  statuses->resize(n);
  st.get(counts->data(), d_counts, 3 * n);
  st.get(statuses->data(), d_status, n);
  return st.ok() ? Status::OK() : st.status("block scan");
}

Status first_failure(const std::vector<uint32_t>& statuses) {
  for (uint32_t s : statuses)
    if (s != LSBM_BLOCK_OK) return block_status(s);
  return Status::OK();
}

}  // namespace

Status ScanBlocks(int device, const char* image, size_t image_size, const uint64_t* handles, size_t n,
                  std::vector<BlockCounts>* counts, std::vector<uint32_t>* statuses) {
  if (!counts || !statuses) return Status::InvalidArgument("null pointer");
  counts->clear();
  statuses->clear();
  if (n == 0) return Status::OK();
  if (!handles || (!image && image_size)) return Status::InvalidArgument("null pointer");
  Staging st;
  Status s = st.Open(device);
  if (!s.ok()) return s;
  const Image d = stage_image(st, image, image_size, handles, n);
  if (!st.ok()) return st.status("staging");
  std::vector<uint64_t> c;
  s = scan_staged(st, d, image_size, n, &c, statuses);
  if (!s.ok()) return s;
  counts->resize(n);
  for (size_t i = 0; i < n; i++) (*counts)[i] = BlockCounts{c[3 * i], c[3 * i + 1], c[3 * i + 2]};
  return first_failure(*statuses);
}

Status DecodeBlocks(int device, const char* image, size_t image_size, const uint64_t* handles, size_t n,
                    std::string* keys, std::vector<uint64_t>* key_offsets, std::vector<uint64_t>* values,
                    std::vector<uint64_t>* entry_first, std::vector<uint32_t>* statuses) {
  if (!keys || !key_offsets || !values || !entry_first || !statuses) return Status::InvalidArgument("null pointer");
  keys->clear();
  key_offsets->assign(1, 0);
  values->clear();
  entry_first->assign(1, 0);
  statuses->clear();
  if (n == 0) return Status::OK();
  if (!handles || (!image && image_size)) return Status::InvalidArgument("null pointer");
  Staging st;
  Status s = st.Open(device);
  if (!s.ok()) return s;
  const Image d = stage_image(st, image, image_size, handles, n);
  if (!st.ok()) return st.status("staging");
  std::vector<uint64_t> c;
  std::vector<uint32_t> scanned;
  s = scan_staged(st, d, image_size, n, &c, &scanned);
  if (!s.ok()) return s;
  // the windows: running sums of the scan's counts
  std::vector<uint64_t> ebase(n + 1, 0), kbase(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    ebase[i + 1] = ebase[i] + c[3 * i];
    kbase[i + 1] = kbase[i] + c[3 * i + 1];
  }
  const uint64_t ne = ebase[n], nk = kbase[n];
  Packed bases;  // one buffer: entry_base[n+1] key_base[n+1]
  const auto f_ebase = bases.add<uint64_t>(n + 1), f_kbase = bases.add<uint64_t>(n + 1);
  uint8_t* d_bases = st.buf<uint8_t>(2, bases.bytes());
  uint32_t* d_status = st.buf<uint32_t>(3, n);
  uint8_t* d_keys = st.buf<uint8_t>(4, nk);
  uint64_t* d_koff = st.buf<uint64_t>(5, ne + 1);
  uint64_t* d_values = st.buf<uint64_t>(6, 2 * ne + 1);
  if (!st.ok()) return st.status("staging");
  st.put(f_ebase.in(d_bases), ebase.data(), n + 1);
  st.put(f_kbase.in(d_bases), kbase.data(), n + 1);
  if (!st.ok()) return st.status("staging");
  if (lsbm_block_decode_dev(d.image, image_size, d.handles, n, f_ebase.in(d_bases), f_kbase.in(d_bases), d_keys, nk,
                            d_koff, d_values, ne, nullptr, d_status, st.stream()) != LSBM_OK)
    return Status::IOError(lsbm_crc32c_last_error());
  keys->assign(nk, '\0');
  key_offsets->assign(ne + 1, 0);
  values->assign(2 * ne, 0);
  statuses->resize(n);
  st.get(statuses->data(), d_status, n);
  st.get(&(*keys)[0], d_keys, nk);
  st.get(key_offsets->data(), d_koff, ne + 1);
  st.get(values->data(), d_values, 2 * ne);
  if (!st.ok()) return st.status("block decode");
  *entry_first = ebase;
  return first_failure(*statuses);
}

Status SeekBlocks(int device, const char* image, size_t image_size, const uint64_t* handles,
                  const char* targets, const uint64_t* target_offsets, size_t n, BlockComparator cmp,
                  bool value_is_handle, std::vector<SeekResult>* results,
                  std::vector<std::string>* found_keys) {
  if (!results) return Status::InvalidArgument("null pointer");
  results->clear();
  if (found_keys) found_keys->clear();
  if (n == 0) return Status::OK();
  if (!handles || !target_offsets || (!image && image_size)) return Status::InvalidArgument("null pointer");
  Status s = check_offsets(target_offsets, n);
  if (!s.ok()) return s;
  const std::vector<uint64_t> toff = rebased(target_offsets, n);
  const uint64_t tbytes = toff[n];
  if (tbytes && !targets) return Status::InvalidArgument("null pointer");

  Staging st;
  s = st.Open(device);
  if (!s.ok()) return s;
  const Image d = stage_image(st, image, image_size, handles, n);
  if (!st.ok()) return st.status("staging");
  Packed res;  // results, one buffer: pos[n] key_len[n] value[2n] handle[2n] (u64), state[n] (u32)
  const auto f_pos = res.add<uint64_t>(n), f_klen = res.add<uint64_t>(n), f_value = res.add<uint64_t>(2 * n);
  const auto f_handle = res.add<uint64_t>(2 * n);
  const auto f_state = res.add<uint32_t>(n);
  uint8_t* d_targets = st.buf<uint8_t>(2, tbytes);
  uint64_t* d_toff = st.buf<uint64_t>(3, n + 1);
  uint8_t* d_out = st.buf<uint8_t>(4, res.bytes());
  st.put(d_targets, targets + target_offsets[0], tbytes);
  st.put(d_toff, toff.data(), n + 1);
  if (!st.ok()) return st.status("staging");
  const uint32_t flags = value_is_handle ? LSBM_SEEK_VALUE_IS_HANDLE : 0u;
  std::vector<uint8_t> out(res.bytes());
  std::vector<uint64_t> foff(n + 1, 0);
  std::string found;
  // found keys: a first Seek gives their lengths, a second one fills windows of that size
  for (int pass = 0; pass < (found_keys ? 2 : 1); pass++) {
    uint8_t* d_found = nullptr;
    uint64_t* d_foff = nullptr;
    if (pass == 1) {
      const uint64_t* klen = f_klen.in(out.data());
      for (size_t i = 0; i < n; i++) foff[i + 1] = foff[i] + klen[i];
      d_found = st.buf<uint8_t>(5, foff[n]);
      d_foff = st.buf<uint64_t>(6, n + 1);
      st.put(d_foff, foff.data(), n + 1);
      if (!st.ok()) return st.status("staging");
    }
    if (lsbm_block_seek_dev(d.image, image_size, d.handles, d_targets, d_toff, n, (int)cmp, flags, f_state.in(d_out),
                            f_pos.in(d_out), f_klen.in(d_out), f_value.in(d_out), f_handle.in(d_out), d_found, d_foff,
                            foff[n], st.stream()) != LSBM_OK)
      return Status::IOError(lsbm_crc32c_last_error());
    st.get(out.data(), d_out, res.bytes());
    if (pass == 1) {
      found.assign(foff[n], '\0');
      st.get(&found[0], d_found, foff[n]);
    }
    if (!st.ok()) return st.status("block seek");
  }
  const uint64_t *pos = f_pos.in(out.data()), *klen = f_klen.in(out.data());
  const uint64_t *val = f_value.in(out.data()), *hnd = f_handle.in(out.data());
  const uint32_t* state = f_state.in(out.data());
  results->resize(n);
  Status first = Status::OK();
  for (size_t i = 0; i < n; i++) {
    (*results)[i] = SeekResult{state[i], pos[i], klen[i], val[2 * i], val[2 * i + 1], hnd[2 * i], hnd[2 * i + 1]};
    if (first.ok()) first = seek_status(state[i]);
  }
  if (found_keys) {
    found_keys->resize(n);
    for (size_t i = 0; i < n; i++) (*found_keys)[i].assign(found, foff[i], foff[i + 1] - foff[i]);
  }
  return first;
}

}  // namespace lsbm
