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
#include "host_session.h"

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

// image and handles on the device (scratch 0 and 1)
Status stage_image(SessionLease& ss, const char* image, size_t image_size, const uint64_t* handles, size_t n,
                   void** d_image, void** d_handles) {
  hipError_t e = ss->scratch(0, image_size ? image_size : 1, d_image);
  if (e == hipSuccess) e = ss->scratch(1, 2 * n * sizeof(uint64_t), d_handles);
  if (e == hipSuccess && image_size) e = ss->upload(*d_image, image, image_size);
  if (e == hipSuccess) e = ss->upload(*d_handles, handles, 2 * n * sizeof(uint64_t));
  return e == hipSuccess ? Status::OK() : hip_status(e, "staging");
}

// lsbm_block_scan_dev into host vectors (scratch 2 and 3)
Status scan_staged(SessionLease& ss, const void* d_image, size_t image_size, const void* d_handles, size_t n,
                   std::vector<uint64_t>* counts, std::vector<uint32_t>* statuses) {
  void *d_counts, *d_status;
  hipError_t e = ss->scratch(2, 3 * n * sizeof(uint64_t), &d_counts);
  if (e == hipSuccess) e = ss->scratch(3, n * sizeof(uint32_t), &d_status);
  if (e != hipSuccess) return hip_status(e, "staging");
  if (lsbm_block_scan_dev(static_cast<const uint8_t*>(d_image), image_size, static_cast<const uint64_t*>(d_handles), n,
                          static_cast<uint64_t*>(d_counts), static_cast<uint32_t*>(d_status),
                          ss->stream()) != LSBM_OK)
    return Status::IOError(lsbm_crc32c_last_error());
  counts->resize(3 * n);
  statuses->resize(n);
  e = ss->download(counts->data(), d_counts, 3 * n * sizeof(uint64_t));
  if (e == hipSuccess) e = ss->download(statuses->data(), d_status, n * sizeof(uint32_t));
  return e == hipSuccess ? Status::OK() : hip_status(e, "block scan");
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
  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  void *d_image, *d_handles;
  s = stage_image(ss, image, image_size, handles, n, &d_image, &d_handles);
  if (!s.ok()) return s;
  std::vector<uint64_t> c;
  s = scan_staged(ss, d_image, image_size, d_handles, n, &c, statuses);
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
  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  void *d_image, *d_handles;
  s = stage_image(ss, image, image_size, handles, n, &d_image, &d_handles);
  if (!s.ok()) return s;
  std::vector<uint64_t> c;
  std::vector<uint32_t> scanned;
  s = scan_staged(ss, d_image, image_size, d_handles, n, &c, &scanned);
  if (!s.ok()) return s;
  // the windows: running sums of the scan's counts
  std::vector<uint64_t> ebase(n + 1, 0), kbase(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    ebase[i + 1] = ebase[i] + c[3 * i];
    kbase[i + 1] = kbase[i] + c[3 * i + 1];
  }
  const uint64_t ne = ebase[n], nk = kbase[n];
  void *d_ebase, *d_kbase, *d_keys, *d_koff, *d_values, *d_status;
  hipError_t e = ss->scratch(2, 2 * (n + 1) * sizeof(uint64_t), &d_ebase);
  if (e == hipSuccess) e = ss->scratch(3, n * sizeof(uint32_t), &d_status);
  if (e == hipSuccess) e = ss->scratch(4, nk ? nk : 1, &d_keys);
  if (e == hipSuccess) e = ss->scratch(5, (ne + 1) * sizeof(uint64_t), &d_koff);
  if (e == hipSuccess) e = ss->scratch(6, (2 * ne + 1) * sizeof(uint64_t), &d_values);
  if (e != hipSuccess) return hip_status(e, "staging");
  d_kbase = static_cast<uint64_t*>(d_ebase) + (n + 1);
  e = ss->upload(d_ebase, ebase.data(), (n + 1) * sizeof(uint64_t));
  if (e == hipSuccess) e = ss->upload(d_kbase, kbase.data(), (n + 1) * sizeof(uint64_t));
  if (e != hipSuccess) return hip_status(e, "staging");
  if (lsbm_block_decode_dev(static_cast<const uint8_t*>(d_image), image_size, static_cast<const uint64_t*>(d_handles),
                            n, static_cast<const uint64_t*>(d_ebase), static_cast<const uint64_t*>(d_kbase),
                            static_cast<uint8_t*>(d_keys), nk, static_cast<uint64_t*>(d_koff),
                            static_cast<uint64_t*>(d_values), ne, nullptr, static_cast<uint32_t*>(d_status),
                            ss->stream()) != LSBM_OK)
    return Status::IOError(lsbm_crc32c_last_error());
  keys->assign(nk, '\0');
  key_offsets->assign(ne + 1, 0);
  values->assign(2 * ne, 0);
  statuses->resize(n);
  e = ss->download(statuses->data(), d_status, n * sizeof(uint32_t));
  if (e == hipSuccess && nk) e = ss->download(&(*keys)[0], d_keys, nk);
  if (e == hipSuccess) e = ss->download(key_offsets->data(), d_koff, (ne + 1) * sizeof(uint64_t));
  if (e == hipSuccess && ne) e = ss->download(values->data(), d_values, 2 * ne * sizeof(uint64_t));
  if (e != hipSuccess) return hip_status(e, "block decode");
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
  for (size_t i = 0; i < n; i++)
    if (target_offsets[i + 1] < target_offsets[i]) return Status::InvalidArgument("offsets must not decrease");
  const uint64_t t0 = target_offsets[0], tbytes = target_offsets[n] - t0;
  if (tbytes && !targets) return Status::InvalidArgument("null pointer");
  std::vector<uint64_t> toff(n + 1);
  for (size_t i = 0; i <= n; i++) toff[i] = target_offsets[i] - t0;

  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  void *d_image, *d_handles, *d_targets, *d_toff, *d_out;
  s = stage_image(ss, image, image_size, handles, n, &d_image, &d_handles);
  if (!s.ok()) return s;
  // results, one buffer: pos[n] key_len[n] value[2n] handle[2n] (u64), state[n] (u32)
  const size_t out_bytes = 6 * n * sizeof(uint64_t) + n * sizeof(uint32_t);
  hipError_t e = ss->scratch(2, tbytes ? tbytes : 1, &d_targets);
  if (e == hipSuccess) e = ss->scratch(3, (n + 1) * sizeof(uint64_t), &d_toff);
  if (e == hipSuccess) e = ss->scratch(4, out_bytes, &d_out);
  if (e == hipSuccess && tbytes) e = ss->upload(d_targets, targets + t0, tbytes);
  if (e == hipSuccess) e = ss->upload(d_toff, toff.data(), (n + 1) * sizeof(uint64_t));
  if (e != hipSuccess) return hip_status(e, "staging");
  uint64_t* d_pos = static_cast<uint64_t*>(d_out);
  uint64_t *d_klen = d_pos + n, *d_value = d_pos + 2 * n, *d_hout = d_pos + 4 * n;
  uint32_t* d_state = reinterpret_cast<uint32_t*>(d_pos + 6 * n);
  const uint32_t flags = value_is_handle ? LSBM_SEEK_VALUE_IS_HANDLE : 0u;
  std::vector<uint8_t> out(out_bytes);
  std::vector<uint64_t> foff(n + 1, 0);
  std::string found;
  // found keys: a first Seek gives their lengths, a second one fills windows of that size
  for (int pass = 0; pass < (found_keys ? 2 : 1); pass++) {
    void *d_found = nullptr, *d_foff = nullptr;
    if (pass == 1) {
      const uint64_t* klen = reinterpret_cast<const uint64_t*>(out.data()) + n;
      for (size_t i = 0; i < n; i++) foff[i + 1] = foff[i] + klen[i];
      e = ss->scratch(5, foff[n] ? foff[n] : 1, &d_found);
      if (e == hipSuccess) e = ss->scratch(6, (n + 1) * sizeof(uint64_t), &d_foff);
      if (e == hipSuccess) e = ss->upload(d_foff, foff.data(), (n + 1) * sizeof(uint64_t));
      if (e != hipSuccess) return hip_status(e, "staging");
    }
    if (lsbm_block_seek_dev(static_cast<const uint8_t*>(d_image), image_size, static_cast<const uint64_t*>(d_handles),
                            d_targets, static_cast<const uint64_t*>(d_toff), n, (int)cmp, flags, d_state, d_pos,
                            d_klen, d_value, d_hout, static_cast<uint8_t*>(d_found),
                            static_cast<const uint64_t*>(d_foff), foff[n], ss->stream()) != LSBM_OK)
      return Status::IOError(lsbm_crc32c_last_error());
    e = ss->download(out.data(), d_out, out_bytes);
    if (e == hipSuccess && pass == 1 && foff[n]) {
      found.assign(foff[n], '\0');
      e = ss->download(&found[0], d_found, foff[n]);
    }
    if (e != hipSuccess) return hip_status(e, "block seek");
  }
  const uint64_t* o = reinterpret_cast<const uint64_t*>(out.data());
  const uint32_t* st = reinterpret_cast<const uint32_t*>(o + 6 * n);
  results->resize(n);
  Status first = Status::OK();
  for (size_t i = 0; i < n; i++) {
    (*results)[i] = SeekResult{st[i], o[i], o[n + i], o[2 * n + 2 * i], o[2 * n + 2 * i + 1],
                               o[4 * n + 2 * i], o[4 * n + 2 * i + 1]};
    if (first.ok()) first = seek_status(st[i]);
  }
  if (found_keys) {
    found_keys->resize(n);
    for (size_t i = 0; i < n; i++) (*found_keys)[i].assign(found, foff[i], foff[i + 1] - foff[i]);
  }
  return first;
}

}  // namespace lsbm
