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
#include "host_staging.h"
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
  Staging st;
  Status s = st.Open(device);
  if (!s.ok()) return s;
  if (host_fault_point(0)) return Status::IOError("injected fault");  // (tests)
  hipStream_t stream = st.stream();

  // 1. the one staging copy: the records back to back, and their pairs
  Packed in, res;
  // pairs[2R] entry_base[R+1] key_base[R+1] table_first[2]
  const auto f_pairs = in.add<uint64_t>(2 * R), f_ebase = in.add<uint64_t>(R + 1), f_kbase = in.add<uint64_t>(R + 1);
  const auto f_tfirst = in.add<uint64_t>(2);
  // counts[2R] max_seq sort_counts[2] (u64) | status[R] sort_status gather_status (u32)
  const auto f_counts = res.add<uint64_t>(2 * R), f_maxseq = res.add<uint64_t>(1), f_scounts = res.add<uint64_t>(2);
  const auto f_rstatus = res.add<uint32_t>(R), f_sstatus = res.add<uint32_t>(1), f_gstatus = res.add<uint32_t>(1);
  uint8_t* d_img = st.buf<uint8_t>(0, image_size);
  uint8_t* d_in = st.buf<uint8_t>(1, in.bytes());
  uint8_t* d_res = st.buf<uint8_t>(3, res.bytes());
  if (!st.ok()) return st.status("staging");
  uint64_t *d_pairs = f_pairs.in(d_in), *d_ebase = f_ebase.in(d_in), *d_kbase = f_kbase.in(d_in);
  uint64_t *d_tfirst = f_tfirst.in(d_in), *d_scounts = f_scounts.in(d_res);
  uint32_t* d_rstatus = f_rstatus.in(d_res);
  if (image_size) {
    std::vector<HostSession::Piece> pieces;
    for (const std::string& r : records)
      if (!r.empty()) pieces.push_back({r.data(), r.size()});
    st.put_pieces(d_img, pieces);
  }
  st.put(d_pairs, pairs.data(), 2 * R);
  if (!st.ok()) return st.status("staging");

  // 2. the walk; its counts size the entries
  if (lsbm_wb_scan_dev(d_img, image_size, d_pairs, R, f_counts.in(d_res), d_rstatus, stream) != LSBM_OK)
    return abi_error();
  std::vector<uint64_t> counts(2 * R + 1, 0), ebase, kbase;
  st.get(counts.data(), f_counts.in(d_res), 2 * R);
  if (!st.ok()) return st.status("scan");
  level0::Bases(counts.data(), R, &ebase, &kbase);
  const uint64_t n = ebase[R], key_bytes = kbase[R];
  if (n > LSBM_MEMTABLE_MAX_ENTRIES) return Status::InvalidArgument("more than 2^31 entries in one memtable");
  const uint64_t table_first[2] = {0, n};
  st.put(d_ebase, ebase.data(), R + 1);
  st.put(d_kbase, kbase.data(), R + 1);
  st.put(d_tfirst, table_first, 2);
  if (!st.ok()) return st.status("staging");

  // 3. decode, sort, gather: arrival order (scratch 2) -> iteration order (scratch 5)
  const uint64_t sort_bytes = lsbm_memtable_sort_scratch_bytes(n);
  const uint64_t plan_bytes = lsbm_block_plan_scratch_bytes(n, 1);
  Packed arr, sorted;
  // key_offsets[n+1] values[2n] keys
  const auto fa_koff = arr.add<uint64_t>(n + 1), fa_vals = arr.add<uint64_t>(2 * n);
  const auto fa_keys = arr.add<uint8_t>(pad8(key_bytes));
  // source[n] plan_offsets[n+1] key_offsets[n+1] values[2n] keys
  const auto fs_source = sorted.add<uint64_t>(n), fs_poff = sorted.add<uint64_t>(n + 1);
  const auto fs_koff = sorted.add<uint64_t>(n + 1), fs_vals = sorted.add<uint64_t>(2 * n);
  const auto fs_keys = sorted.add<uint8_t>(pad8(key_bytes));
  uint8_t* d_arr = st.buf<uint8_t>(2, arr.bytes() + 8);
  uint8_t* d_tmp = st.buf<uint8_t>(4, (sort_bytes > plan_bytes ? sort_bytes : plan_bytes) + 8);
  uint8_t* d_sorted = st.buf<uint8_t>(5, sorted.bytes() + 8);
  if (!st.ok()) return st.status("staging");
  uint64_t *a_koff = fa_koff.in(d_arr), *a_vals = fa_vals.in(d_arr);
  uint8_t* a_keys = fa_keys.in(d_arr);
  uint64_t *s_source = fs_source.in(d_sorted), *s_poff = fs_poff.in(d_sorted);
  uint64_t *s_koff = fs_koff.in(d_sorted), *s_vals = fs_vals.in(d_sorted);
  uint8_t* s_keys = fs_keys.in(d_sorted);
  if (lsbm_wb_decode_dev(d_img, image_size, d_pairs, R, d_ebase, d_kbase, a_keys, key_bytes, a_koff, a_vals, n,
                         f_maxseq.in(d_res), d_rstatus, stream) != LSBM_OK ||
      lsbm_memtable_sort_dev(a_keys, key_bytes, a_koff, n, s_source, s_poff, d_scounts, f_sstatus.in(d_res), d_tmp,
                             sort_bytes, stream) != LSBM_OK ||
      lsbm_merge_gather_dev(a_keys, key_bytes, a_koff, a_vals, n, s_source, s_poff, d_scounts, s_keys, key_bytes,
                            s_koff, s_vals, n, f_gstatus.in(d_res), stream) != LSBM_OK)
    return abi_error();

  // the host's second read: the walk's results
  std::vector<uint8_t> host(res.bytes());
  st.get(host.data(), d_res, res.bytes());
  if (!st.ok()) return st.status("memtable flush");
  const uint8_t* h = host.data();
  const uint32_t* rs = f_rstatus.in(h);
  record_status->assign(rs, rs + R);
  *max_sequence = *f_maxseq.in(h);
  for (size_t r = 0; r < R; r++)
    if (rs[r] == LSBM_WB_BAD_INPUT || rs[r] == LSBM_WB_NO_ROOM || (opt.paranoid_checks && rs[r] != LSBM_WB_OK))
      return level0::RecordStatus(rs[r], r);
  if (*f_sstatus.in(h) != LSBM_MERGE_OK || *f_gstatus.in(h) != LSBM_MERGE_OK || f_scounts.in(h)[0] != n ||
      f_scounts.in(h)[1] != key_bytes)
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
  Packed lay;
  const auto f_bfirst = lay.add<uint64_t>(n + 1), f_bbytes = lay.add<uint64_t>(n), f_tbf = lay.add<uint64_t>(2);
  const size_t plan_words = lay.bytes() / 8;  // the plan's outputs come first: one read brings them back
  const auto f_handles = lay.add<uint64_t>(2 * hcap), f_built = lay.add<uint64_t>(hcap);
  const auto f_pstatus = lay.add<uint32_t>(1), f_bstatus = lay.add<uint32_t>(hcap), f_nbad = lay.add<uint32_t>(1);
  const auto f_types = lay.add<uint8_t>(hcap);
  uint8_t* d_lay = st.buf<uint8_t>(6, lay.bytes() + 8);
  if (!st.ok()) return st.status("staging");
  uint64_t *d_bfirst = f_bfirst.in(d_lay), *d_tbf = f_tbf.in(d_lay), *d_handles = f_handles.in(d_lay);
  uint64_t* d_built = f_built.in(d_lay);
  uint32_t *d_pstatus = f_pstatus.in(d_lay), *d_bstatus = f_bstatus.in(d_lay), *d_nbad = f_nbad.in(d_lay);
  uint8_t* d_types = f_types.in(d_lay);
  if (lsbm_block_plan_dev(s_keys, key_bytes, s_koff, s_vals, n, d_tfirst, 1, opt.block_size,
                          opt.block_restart_interval, d_bfirst, f_bbytes.in(d_lay), cap, d_tbf, d_pstatus, d_tmp,
                          plan_bytes, stream) != LSBM_OK)
    return abi_error();
  // the third read: the plan
  std::vector<uint64_t> plan_out(plan_words, 0);
  st.get(plan_out.data(), d_bfirst, plan_words);
  uint32_t plan_status = 0;
  st.get(&plan_status, d_pstatus, 1);
  if (!st.ok()) return st.status("block plan");
  if (plan_status != LSBM_BUILD_OK) return Status::InvalidArgument("block would reach 2^32 bytes");
  const uint64_t nb = f_tbf.in(plan_out.data())[1];
  if (nb == 0 || nb > cap) return Status::IOError("internal error: block plan out of range");
  const uint64_t* block_first = f_bfirst.in(plan_out.data());
  const uint64_t* block_bytes = f_bbytes.in(plan_out.data());

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
  st.put(d_handles, handles.data(), 2 * nb);
  if (!st.ok()) return st.status("staging");
  if (lsbm_index_block_build_dev(s_keys, key_bytes, s_koff, n, d_bfirst, nb, d_tbf, 1, d_handles, LSBM_CMP_INTERNAL_KEY,
                                 nullptr, 0, nullptr, d_built, d_bstatus, stream) != LSBM_OK)
    return abi_error();
  uint64_t index_size = 0;
  uint32_t index_status = 0;
  st.get(&index_size, d_built, 1);
  st.get(&index_status, d_bstatus, 1);
  if (!st.ok()) return st.status("index block");
  if (index_status != LSBM_BUILD_OK) return Status::IOError("internal error: index block");
  const uint64_t index_at = at;
  handles[2 * nh] = at;
  handles[2 * nh + 1] = index_size;
  at += index_size + 5;
  nh++;
  const std::string footer = level0::Footer(meta_at, meta.size(), index_at, index_size);
  const uint64_t file_size = at + footer.size();

  // 6. every block into its place, the trailers, the footer
  uint8_t* d_file = st.buf<uint8_t>(7, file_size);
  if (!st.ok()) return st.status("staging");
  st.note(hipMemsetAsync(d_file, 0, file_size, stream));
  if (st.ok()) st.note(hipMemsetAsync(d_types, 0, hcap, stream));  // kNoCompression
  if (st.ok()) st.note(hipMemsetAsync(d_nbad, 0, 4, stream));
  if (!st.ok()) return st.status("memset");
  st.put(d_handles, handles.data(), 2 * nh);
  if (!st.ok()) return st.status("staging");
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
      uint64_t* d_fin = st.buf<uint64_t>(4, fin.size());  // (the sort's scratch is free again; the plan's too)
      st.put(d_fin, fin.data(), fin.size());
      if (!st.ok()) return st.status("staging");
      if (lsbm_bloom_build_dev(s_keys, s_koff, LSBM_INTERNAL_KEY_SUFFIX, d_fin, d_fin + nf + 1, nf, opt.bits_per_key,
                               d_file, stream) != LSBM_OK)
        return abi_error();
    }
    st.put(d_file + filter_at + fl.data_bytes, fl.trailer.data(), fl.trailer.size());
    if (!st.ok()) return st.status("staging");
  }
  st.put(d_file + meta_at, meta.data(), meta.size());
  st.put(d_file + at, footer.data(), footer.size());
  if (!st.ok()) return st.status("staging");
  if (lsbm_index_block_build_dev(s_keys, key_bytes, s_koff, n, d_bfirst, nb, d_tbf, 1, d_handles, LSBM_CMP_INTERNAL_KEY,
                                 d_file, file_size, d_handles + 2 * (nh - 1), d_built + nb, d_bstatus + nb,
                                 stream) != LSBM_OK ||
      lsbm_sst_seal_dev(d_file, file_size, d_handles, d_types, nh, d_nbad, stream) != LSBM_OK)
    return abi_error();
  std::vector<uint32_t> bst(nb + 2, 0);
  st.get(bst.data(), d_bstatus, nb + 1);
  st.get(&bst[nb + 1], d_nbad, 1);
  if (!st.ok()) return st.status("table build");
  for (uint32_t v : bst)
    if (v != 0) return Status::IOError("internal error: table build failed");

  // 7. the file and its key range come back; nothing the caller sees has changed before this point
  std::string out(file_size, '\0');
  std::vector<uint64_t> ends(2);  // key_offsets[1], key_offsets[n - 1]
  st.get(&out[0], d_file, file_size);
  st.get(&ends[0], s_koff + 1, 1);
  st.get(&ends[1], s_koff + (n - 1), 1);
  if (!st.ok()) return st.status("table download");
  if (ends[0] > key_bytes || ends[1] > key_bytes) return Status::IOError("internal error: key offsets out of range");
  std::string lo(ends[0], '\0'), hi(key_bytes - ends[1], '\0');
  st.get(&lo[0], s_keys, lo.size());
  st.get(&hi[0], s_keys + ends[1], hi.size());
  if (!st.ok()) return st.status("table download");
  file->swap(out);
  smallest->swap(lo);
  largest->swap(hi);
  return Status::OK();
}

}  // namespace lsbm
