// memtable_flush.cc -- include/lsbm/memtable_flush.h: BuildLevel0 on top of the
// C ABI.  The records go to the device once, back to back, through the
// device's HostSession (host_session.h); scan, decode, sort, gather, the block
// plan, the data blocks, the filters, the index block and the trailers run on
// its stream; the host reads the scan's counts (to size the entries), the statuses, the
// plan (to lay the file out) and the index block's size, and writes the small
// blocks TableBuilder::Finish makes itself (memtable_flush_host.cc).
#include "../../include/lsbm/memtable_flush.h"

#include <hip/hip_runtime_api.h>
#include <string.h>

#include "../../include/lsbm_block_build.h"
#include "../../include/lsbm_bloom.h"
#include "../../include/lsbm_crc32c.h"
#include "../../include/lsbm_memtable.h"
#include "../../include/lsbm_merge.h"
#include "host_session.h"
#include "memtable_flush_host.h"

namespace lsbm {

namespace {

uint64_t pad8(uint64_t n) { return (n + 7) & ~7ull; }

Status abi_error() { return Status::IOError(lsbm_crc32c_last_error()); }

}  // namespace

Status BuildLevel0(int device, const std::vector<std::string>& records, const Level0Options& opt, std::string* file,
                   std::string* smallest, std::string* largest, uint64_t* max_sequence,
                   std::vector<uint32_t>* record_status) {
  if (!file || !smallest || !largest || !max_sequence || !record_status) return Status::InvalidArgument("null pointer");
  if (opt.block_size == 0 || opt.block_restart_interval == 0)
    return Status::InvalidArgument("block_size and block_restart_interval must be at least 1");
  *max_sequence = 0;
  record_status->clear();
  const size_t R = records.size();
  std::vector<uint64_t> pairs;
  const uint64_t image_size = level0::LayoutRecords(records, &pairs);
  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  if (host_fault_point(0)) return Status::IOError("injected fault");  // (tests)
  hipStream_t stream = ss->stream();

  // 1. the one staging copy: the records back to back, and their pairs
  void *d_img_v, *d_in_v, *d_res_v;
  hipError_t e = ss->scratch(0, image_size ? image_size : 1, &d_img_v);
  // pairs[2R] entry_base[R+1] key_base[R+1] table_first[2]
  if (e == hipSuccess) e = ss->scratch(1, (4 * R + 4) * sizeof(uint64_t), &d_in_v);
  // counts[2R] max_seq sort_counts[2] (u64) | status[R] sort_status gather_status (u32)
  const size_t res_words = 2 * R + 3;
  if (e == hipSuccess) e = ss->scratch(3, res_words * 8 + (R + 2) * 4, &d_res_v);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint8_t* d_img = static_cast<uint8_t*>(d_img_v);
  uint64_t* d_pairs = static_cast<uint64_t*>(d_in_v);
  uint64_t *d_ebase = d_pairs + 2 * R, *d_kbase = d_ebase + R + 1, *d_tfirst = d_kbase + R + 1;
  uint64_t* d_counts = static_cast<uint64_t*>(d_res_v);
  uint64_t *d_maxseq = d_counts + 2 * R, *d_scounts = d_maxseq + 1;
  uint32_t* d_rstatus = reinterpret_cast<uint32_t*>(d_scounts + 2);
  uint32_t *d_sstatus = d_rstatus + R, *d_gstatus = d_sstatus + 1;
  if (image_size) {
    std::vector<HostSession::Piece> pieces;
    for (const std::string& r : records)
      if (!r.empty()) pieces.push_back({r.data(), r.size()});
    e = ss->upload_pieces(d_img, pieces.data(), pieces.size());
  }
  if (e == hipSuccess && R) e = ss->upload(d_pairs, pairs.data(), 2 * R * sizeof(uint64_t));
  if (e != hipSuccess) return hip_status(e, "staging");

  // 2. the walk; its counts size the entries
  if (lsbm_wb_scan_dev(d_img, image_size, d_pairs, R, d_counts, d_rstatus, stream) != LSBM_OK) return abi_error();
  std::vector<uint64_t> counts(2 * R + 1, 0), ebase, kbase;
  if (R) e = ss->download(counts.data(), d_counts, 2 * R * sizeof(uint64_t));
  if (e != hipSuccess) return hip_status(e, "scan");
  level0::Bases(counts.data(), R, &ebase, &kbase);
  const uint64_t n = ebase[R], key_bytes = kbase[R];
  if (n > LSBM_MEMTABLE_MAX_ENTRIES) return Status::InvalidArgument("more than 2^31 entries in one memtable");
  const uint64_t table_first[2] = {0, n};
  e = ss->upload(d_ebase, ebase.data(), (R + 1) * sizeof(uint64_t));
  if (e == hipSuccess) e = ss->upload(d_kbase, kbase.data(), (R + 1) * sizeof(uint64_t));
  if (e == hipSuccess) e = ss->upload(d_tfirst, table_first, sizeof(table_first));
  if (e != hipSuccess) return hip_status(e, "staging");

  // 3. decode, sort, gather: arrival order (scratch 2) -> iteration order (scratch 5)
  const uint64_t sort_bytes = lsbm_memtable_sort_scratch_bytes(n);
  const uint64_t plan_bytes = lsbm_block_plan_scratch_bytes(n, 1);
  void *d_arr_v, *d_tmp_v, *d_sorted_v;
  // key_offsets[n+1] values[2n] keys
  e = ss->scratch(2, (3 * n + 1) * 8 + pad8(key_bytes) + 8, &d_arr_v);
  if (e == hipSuccess) e = ss->scratch(4, (sort_bytes > plan_bytes ? sort_bytes : plan_bytes) + 8, &d_tmp_v);
  // source[n] plan_offsets[n+1] key_offsets[n+1] values[2n] keys
  if (e == hipSuccess) e = ss->scratch(5, (5 * n + 2) * 8 + pad8(key_bytes) + 8, &d_sorted_v);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint64_t* a_koff = static_cast<uint64_t*>(d_arr_v);
  uint64_t* a_vals = a_koff + n + 1;
  uint8_t* a_keys = reinterpret_cast<uint8_t*>(a_vals + 2 * n);
  uint64_t* s_source = static_cast<uint64_t*>(d_sorted_v);
  uint64_t *s_poff = s_source + n, *s_koff = s_poff + n + 1, *s_vals = s_koff + n + 1;
  uint8_t* s_keys = reinterpret_cast<uint8_t*>(s_vals + 2 * n);
  if (lsbm_wb_decode_dev(d_img, image_size, d_pairs, R, d_ebase, d_kbase, a_keys, key_bytes, a_koff, a_vals, n,
                         d_maxseq, d_rstatus, stream) != LSBM_OK ||
      lsbm_memtable_sort_dev(a_keys, key_bytes, a_koff, n, s_source, s_poff, d_scounts, d_sstatus, d_tmp_v, sort_bytes,
                             stream) != LSBM_OK ||
      lsbm_merge_gather_dev(a_keys, key_bytes, a_koff, a_vals, n, s_source, s_poff, d_scounts, s_keys, key_bytes,
                            s_koff, s_vals, n, d_gstatus, stream) != LSBM_OK)
    return abi_error();

  // the host's second read: the walk's results
  std::vector<uint8_t> res(res_words * 8 + (R + 2) * 4);
  e = ss->download(res.data(), d_res_v, res.size());
  if (e != hipSuccess) return hip_status(e, "memtable flush");
  const uint64_t* rw = reinterpret_cast<const uint64_t*>(res.data());
  const uint32_t* rs = reinterpret_cast<const uint32_t*>(rw + res_words);
  record_status->assign(rs, rs + R);
  *max_sequence = rw[2 * R];
  for (size_t r = 0; r < R; r++) {
    const uint32_t st = rs[r];
    if (st == LSBM_WB_BAD_INPUT || st == LSBM_WB_NO_ROOM || (opt.paranoid_checks && st != LSBM_WB_OK))
      return level0::RecordStatus(st, r);
  }
  if (rs[R] != LSBM_MERGE_OK || rs[R + 1] != LSBM_MERGE_OK || rw[2 * R + 1] != n || rw[2 * R + 2] != key_bytes)
    return Status::IOError("internal error: memtable sort failed");
  if (n == 0) {  // BuildTable writes no file
    file->clear();
    smallest->clear();
    largest->clear();
    return Status::OK();
  }

  // 4. the block plan of the one table
  // block_first[n+1] block_bytes[n] table_block_first[2] handles[2(n+3)] built[n+3] (u64) | plan_status
  // build_status[n+3] nbad (u32) types[n+3] (u8)
  const uint64_t cap = n, hcap = n + 3;
  const size_t lay_words = (n + 1) + n + 2 + 2 * hcap + hcap;
  void* d_lay_v;
  e = ss->scratch(6, lay_words * 8 + (hcap + 2) * 4 + hcap + 8, &d_lay_v);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint64_t* d_bfirst = static_cast<uint64_t*>(d_lay_v);
  uint64_t *d_bbytes = d_bfirst + n + 1, *d_tbf = d_bbytes + n, *d_handles = d_tbf + 2, *d_built = d_handles + 2 * hcap;
  uint32_t* d_pstatus = reinterpret_cast<uint32_t*>(d_built + hcap);
  uint32_t *d_bstatus = d_pstatus + 1, *d_nbad = d_bstatus + hcap;
  uint8_t* d_types = reinterpret_cast<uint8_t*>(d_nbad + 1);
  if (lsbm_block_plan_dev(s_keys, key_bytes, s_koff, s_vals, n, d_tfirst, 1, opt.block_size,
                          opt.block_restart_interval, d_bfirst, d_bbytes, cap, d_tbf, d_pstatus, d_tmp_v, plan_bytes,
                          stream) != LSBM_OK)
    return abi_error();
  // the third read: the plan
  std::vector<uint64_t> plan_out(2 * n + 3, 0);
  e = ss->download(plan_out.data(), d_bfirst, plan_out.size() * 8);
  uint32_t plan_status = 0;
  if (e == hipSuccess) e = ss->download(&plan_status, d_pstatus, 4);
  if (e != hipSuccess) return hip_status(e, "block plan");
  if (plan_status != LSBM_BUILD_OK) return Status::InvalidArgument("block would reach 2^32 bytes");
  const uint64_t nb = plan_out[2 * n + 2];
  if (nb == 0 || nb > cap) return Status::IOError("internal error: block plan out of range");
  const uint64_t* block_first = plan_out.data();
  const uint64_t* block_bytes = plan_out.data() + n + 1;

  // 5. the file's layout: data blocks, [filter block], metaindex block, index block, footer
  std::vector<uint64_t> handles(2 * (nb + 3), 0), starts(nb);
  uint64_t at = 0;
  for (uint64_t b = 0; b < nb; b++) {
    starts[b] = handles[2 * b] = at;
    handles[2 * b + 1] = block_bytes[b];
    at += block_bytes[b] + 5;
  }
  const bool with_filter = opt.bits_per_key >= 0;
  level0::FilterLayout fl;
  size_t nh = nb;
  uint64_t filter_at = at;
  if (with_filter) {
    level0::LayoutFilterBlock(starts.data(), block_first, nb, at, opt.bits_per_key, &fl);
    handles[2 * nh] = at;
    handles[2 * nh + 1] = fl.data_bytes + fl.trailer.size();
    at += handles[2 * nh + 1] + 5;
    nh++;
  }
  const std::string meta = level0::MetaindexBlock(with_filter, filter_at, fl.data_bytes + fl.trailer.size());
  const uint64_t meta_at = at;
  handles[2 * nh] = at;
  handles[2 * nh + 1] = meta.size();
  at += meta.size() + 5;
  nh++;
  // the index block's size: a launch without an output
  e = ss->upload(d_handles, handles.data(), 2 * nb * sizeof(uint64_t));
  if (e != hipSuccess) return hip_status(e, "staging");
  if (lsbm_index_block_build_dev(s_keys, key_bytes, s_koff, n, d_bfirst, nb, d_tbf, 1, d_handles, LSBM_CMP_INTERNAL_KEY,
                                 nullptr, 0, nullptr, d_built, d_bstatus, stream) != LSBM_OK)
    return abi_error();
  uint64_t index_size = 0;
  uint32_t index_status = 0;
  e = ss->download(&index_size, d_built, 8);
  if (e == hipSuccess) e = ss->download(&index_status, d_bstatus, 4);
  if (e != hipSuccess) return hip_status(e, "index block");
  if (index_status != LSBM_BUILD_OK) return Status::IOError("internal error: index block");
  const uint64_t index_at = at;
  handles[2 * nh] = at;
  handles[2 * nh + 1] = index_size;
  at += index_size + 5;
  nh++;
  const std::string footer = level0::Footer(meta_at, meta.size(), index_at, index_size);
  const uint64_t file_size = at + footer.size();

  // 6. every block into its place, the trailers, the footer
  void* d_file_v;
  e = ss->scratch(7, file_size, &d_file_v);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint8_t* d_file = static_cast<uint8_t*>(d_file_v);
  e = hipMemsetAsync(d_file, 0, file_size, stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_types, 0, hcap, stream);  // kNoCompression
  if (e == hipSuccess) e = hipMemsetAsync(d_nbad, 0, 4, stream);
  if (e != hipSuccess) return hip_status(e, "memset");
  e = ss->upload(d_handles, handles.data(), 2 * nh * sizeof(uint64_t));
  if (e != hipSuccess) return hip_status(e, "staging");
  if (lsbm_block_build_dev(s_keys, key_bytes, s_koff, s_vals, d_img, image_size, n, d_bfirst, nb,
                           opt.block_restart_interval, d_file, file_size, d_handles, d_built, d_bstatus,
                           stream) != LSBM_OK)
    return abi_error();
  if (with_filter) {
    const size_t nf = fl.filter_out.size();
    if (nf) {
      // filter_first[nf+1] filter_out[nf], the latter as offsets in the file
      std::vector<uint64_t> fin(fl.filter_first);
      for (uint64_t o : fl.filter_out) fin.push_back(filter_at + o);
      void* d_fin_v;  // (the sort's scratch is free again; the plan's too)
      e = ss->scratch(4, fin.size() * 8, &d_fin_v);
      if (e == hipSuccess) e = ss->upload(d_fin_v, fin.data(), fin.size() * 8);
      if (e != hipSuccess) return hip_status(e, "staging");
      const uint64_t* d_fin = static_cast<const uint64_t*>(d_fin_v);
      if (lsbm_bloom_build_dev(s_keys, s_koff, LSBM_INTERNAL_KEY_SUFFIX, d_fin, d_fin + nf + 1, nf, opt.bits_per_key,
                               d_file, stream) != LSBM_OK)
        return abi_error();
    }
    e = ss->upload(d_file + filter_at + fl.data_bytes, fl.trailer.data(), fl.trailer.size());
    if (e != hipSuccess) return hip_status(e, "staging");
  }
  e = ss->upload(d_file + meta_at, meta.data(), meta.size());
  if (e == hipSuccess) e = ss->upload(d_file + at, footer.data(), footer.size());
  if (e != hipSuccess) return hip_status(e, "staging");
  if (lsbm_index_block_build_dev(s_keys, key_bytes, s_koff, n, d_bfirst, nb, d_tbf, 1, d_handles, LSBM_CMP_INTERNAL_KEY,
                                 d_file, file_size, d_handles + 2 * (nh - 1), d_built + nb, d_bstatus + nb,
                                 stream) != LSBM_OK ||
      lsbm_sst_seal_dev(d_file, file_size, d_handles, d_types, nh, d_nbad, stream) != LSBM_OK)
    return abi_error();
  std::vector<uint32_t> bst(nb + 2, 0);
  e = ss->download(bst.data(), d_bstatus, (nb + 1) * 4);
  if (e == hipSuccess) e = ss->download(&bst[nb + 1], d_nbad, 4);
  if (e != hipSuccess) return hip_status(e, "table build");
  for (uint32_t v : bst)
    if (v != 0) return Status::IOError("internal error: table build failed");

  // 7. the file and its key range come back; nothing the caller sees has changed before this point
  std::string out(file_size, '\0');
  std::vector<uint64_t> ends(2);  // key_offsets[1], key_offsets[n - 1]
  e = ss->download(&out[0], d_file, file_size);
  if (e == hipSuccess) e = ss->download(&ends[0], s_koff + 1, 8);
  if (e == hipSuccess) e = ss->download(&ends[1], s_koff + (n - 1), 8);
  if (e != hipSuccess) return hip_status(e, "table download");
  if (ends[0] > key_bytes || ends[1] > key_bytes) return Status::IOError("internal error: key offsets out of range");
  std::string lo(ends[0], '\0'), hi(key_bytes - ends[1], '\0');
  e = ss->download(&lo[0], s_keys, lo.size());
  if (e == hipSuccess) e = ss->download(&hi[0], s_keys + ends[1], hi.size());
  if (e != hipSuccess) return hip_status(e, "table download");
  file->swap(out);
  smallest->swap(lo);
  largest->swap(hi);
  return Status::OK();
}

}  // namespace lsbm
