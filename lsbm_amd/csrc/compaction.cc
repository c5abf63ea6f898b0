// compaction.cc -- include/lsbm/compaction.h: MergeRuns on top of the C ABI
// (include/lsbm_merge.h) and the host-side table cut.  The keys and offsets go
// to the device once through the device's HostSession (host_session.h), plan
// and gather run back to back on its stream with input-sized outputs (no host
// read between them), and only the results come back.
#include "../../include/lsbm/compaction.h"

#include <hip/hip_runtime_api.h>
#include <string.h>

#include "../../include/lsbm_crc32c.h"
#include "../../include/lsbm_merge.h"
#include "host_staging.h"

namespace lsbm {

Status CutTables(const uint64_t* block_first, const uint64_t* block_bytes, size_t n_blocks, uint64_t max_file_size,
                 std::vector<uint64_t>* table_first, std::vector<uint64_t>* table_block_first) {
  if (!table_first || !table_block_first || !block_first || (!block_bytes && n_blocks))
    return Status::InvalidArgument("null pointer");
  table_first->assign(1, block_first[0]);
  table_block_first->assign(1, 0);
  uint64_t file_size = 0;
  for (size_t b = 0; b < n_blocks; b++) {
    if (block_first[b + 1] < block_first[b]) return Status::InvalidArgument("block_first decreases");
    const uint64_t add = block_bytes[b] + 5;  // WriteRawBlock: the block and its trailer
    file_size = file_size + add < file_size ? ~0ull : file_size + add;
    if (file_size >= max_file_size || b + 1 == n_blocks) {
      table_first->push_back(block_first[b + 1]);
      table_block_first->push_back(b + 1);
      file_size = 0;
    }
  }
  return Status::OK();
}

namespace {

Status merge_status(uint32_t s, size_t run) {
  const std::string where = " (run " + std::to_string(run) + ")";
  switch (s) {
    case LSBM_MERGE_OK: return Status::OK();
    case LSBM_MERGE_BAD_INPUT: return Status::InvalidArgument("bad merge input" + where);
    case LSBM_MERGE_UNSORTED: return Status::InvalidArgument("run is not sorted" + where);
    default: return Status::IOError("internal error: merge output window too small");
  }
}

}  // namespace

Status MergeRuns(int device, const BlockEntries& en, const uint64_t* run_first, size_t n_runs, const MergeOptions& opt,
                 std::string* keys, std::vector<uint64_t>* key_offsets, std::vector<uint64_t>* values,
                 std::vector<uint64_t>* source, std::vector<uint32_t>* run_statuses) {
  if (!keys || !key_offsets || !values || !source || !run_statuses) return Status::InvalidArgument("null pointer");
  keys->clear();
  key_offsets->assign(1, 0);
  values->clear();
  source->clear();
  run_statuses->clear();
  if (!run_first || !en.key_offsets || (!en.keys && en.keys_size) || (!en.values && en.n))
    return Status::InvalidArgument("null pointer");
  if (n_runs > LSBM_MERGE_MAX_RUNS) return Status::InvalidArgument("more than 64 runs");
  if (opt.cmp != kBytewiseComparator && opt.cmp != kInternalKeyComparator) return Status::InvalidArgument("unknown comparator");
  if (opt.drop && opt.cmp != kInternalKeyComparator) return Status::InvalidArgument("the drop rule needs internal keys");
  Staging st;
  Status s = st.Open(device);
  if (!s.ok()) return s;
  const size_t n = en.n;
  const uint64_t scratch_bytes = lsbm_merge_scratch_bytes(n, n_runs);
  // scratch 0: keys | 1: key_offsets values run_first | 2: plan's scratch
  // 3: source[n] plan_offsets[n+1] counts[2] out_offsets[n+1] out_values[2n] (u64) run_status[R] status (u32)
  // 4: out keys
  Packed in, res;
  const auto f_koff = in.add<uint64_t>(n + 1), f_vals = in.add<uint64_t>(2 * n), f_runs = in.add<uint64_t>(n_runs + 1);
  const auto f_source = res.add<uint64_t>(n), f_poff = res.add<uint64_t>(n + 1), f_counts = res.add<uint64_t>(2);
  const auto f_ooff = res.add<uint64_t>(n + 1), f_ovals = res.add<uint64_t>(2 * n);
  const auto f_rst = res.add<uint32_t>(n_runs), f_gst = res.add<uint32_t>(1);
  uint8_t* d_k = st.buf<uint8_t>(0, en.keys_size);
  uint8_t* d_o = st.buf<uint8_t>(1, in.bytes());
  uint8_t* d_s = st.buf<uint8_t>(2, scratch_bytes);
  uint8_t* d_r = st.buf<uint8_t>(3, res.bytes());
  uint8_t* d_ok = st.buf<uint8_t>(4, en.keys_size);
  st.put(d_k, en.keys, en.keys_size);
  st.put(f_koff.in(d_o), en.key_offsets, n + 1);
  st.put(f_vals.in(d_o), en.values, 2 * n);
  st.put(f_runs.in(d_o), run_first, n_runs + 1);
  if (!st.ok()) return st.status("staging");
  const uint32_t flags = (opt.drop ? LSBM_MERGE_DROP : 0u) | (opt.bottom_level ? LSBM_MERGE_BOTTOM_LEVEL : 0u);
  if (lsbm_merge_plan_dev(d_k, en.keys_size, f_koff.in(d_o), n, f_runs.in(d_o), n_runs, (int)opt.cmp, flags,
                          opt.smallest_snapshot, f_source.in(d_r), f_poff.in(d_r), f_counts.in(d_r), f_rst.in(d_r), d_s,
                          scratch_bytes, st.stream()) != LSBM_OK ||
      lsbm_merge_gather_dev(d_k, en.keys_size, f_koff.in(d_o), f_vals.in(d_o), n, f_source.in(d_r), f_poff.in(d_r),
                            f_counts.in(d_r), d_ok, en.keys_size, f_ooff.in(d_r), f_ovals.in(d_r), n, f_gst.in(d_r),
                            st.stream()) != LSBM_OK)
    return Status::InvalidArgument(lsbm_crc32c_last_error());
  std::vector<uint8_t> host(res.bytes());
  st.get(host.data(), d_r, res.bytes());
  if (!st.ok()) return st.status("merge");
  const uint8_t* h = host.data();
  const uint32_t* rst = f_rst.in(h);
  run_statuses->assign(rst, rst + n_runs);
  for (size_t r = 0; r < n_runs; r++)
    if (rst[r] != LSBM_MERGE_OK) return merge_status(rst[r], r);
  if (*f_gst.in(h) != LSBM_MERGE_OK) return Status::IOError("internal error: merge gather failed");
  const uint64_t n_out = f_counts.in(h)[0], key_bytes = f_counts.in(h)[1];
  if (n_out > n || key_bytes > en.keys_size) return Status::IOError("internal error: merge output larger than its input");
  source->assign(f_source.in(h), f_source.in(h) + n_out);
  key_offsets->assign(f_ooff.in(h), f_ooff.in(h) + n_out + 1);
  values->assign(f_ovals.in(h), f_ovals.in(h) + 2 * n_out);
  keys->assign(key_bytes, '\0');
  st.get(&(*keys)[0], d_ok, key_bytes);
  if (!st.ok()) return st.status("merge");
  return Status::OK();
}

}  // namespace lsbm
