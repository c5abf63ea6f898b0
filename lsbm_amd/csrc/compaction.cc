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
#include "host_session.h"

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
  SessionLease ss;
  Status s = ss.Open(device);
  if (!s.ok()) return s;
  const size_t n = en.n;
  const size_t off_bytes = (n + 1) * sizeof(uint64_t), val_bytes = 2 * n * sizeof(uint64_t);
  const size_t run_bytes = (n_runs + 1) * sizeof(uint64_t);
  const uint64_t scratch_bytes = lsbm_merge_scratch_bytes(n, n_runs);
  // scratch 0: keys | 1: key_offsets values run_first | 2: plan's scratch
  // 3: source[n] plan_offsets[n+1] counts[2] out_offsets[n+1] out_values[2n] (u64) run_status[R] status (u32)
  // 4: out keys
  const size_t res_words = 5 * n + 4;
  const size_t res_bytes = res_words * sizeof(uint64_t) + (n_runs + 1) * sizeof(uint32_t);
  void *d_k, *d_o, *d_s, *d_r, *d_ok;
  hipError_t e = ss->scratch(0, en.keys_size ? en.keys_size : 1, &d_k);
  if (e == hipSuccess) e = ss->scratch(1, off_bytes + val_bytes + run_bytes, &d_o);
  if (e == hipSuccess) e = ss->scratch(2, scratch_bytes, &d_s);
  if (e == hipSuccess) e = ss->scratch(3, res_bytes, &d_r);
  if (e == hipSuccess) e = ss->scratch(4, en.keys_size ? en.keys_size : 1, &d_ok);
  if (e == hipSuccess && en.keys_size) e = ss->upload(d_k, en.keys, en.keys_size);
  if (e == hipSuccess) e = ss->upload(d_o, en.key_offsets, off_bytes);
  uint64_t* d_koff = static_cast<uint64_t*>(d_o);
  uint64_t *d_vals = d_koff + n + 1, *d_runs = d_vals + 2 * n;
  if (e == hipSuccess && n) e = ss->upload(d_vals, en.values, val_bytes);
  if (e == hipSuccess) e = ss->upload(d_runs, run_first, run_bytes);
  if (e != hipSuccess) return hip_status(e, "staging");
  uint64_t* d_source = static_cast<uint64_t*>(d_r);
  uint64_t *d_poff = d_source + n, *d_counts = d_poff + n + 1, *d_ooff = d_counts + 2, *d_ovals = d_ooff + n + 1;
  uint32_t* d_rst = reinterpret_cast<uint32_t*>(d_ovals + 2 * n);
  uint32_t* d_gst = d_rst + n_runs;
  const uint32_t flags = (opt.drop ? LSBM_MERGE_DROP : 0u) | (opt.bottom_level ? LSBM_MERGE_BOTTOM_LEVEL : 0u);
  if (lsbm_merge_plan_dev(static_cast<uint8_t*>(d_k), en.keys_size, d_koff, n, d_runs, n_runs, (int)opt.cmp, flags,
                          opt.smallest_snapshot, d_source, d_poff, d_counts, d_rst, d_s, scratch_bytes,
                          ss->stream()) != LSBM_OK ||
      lsbm_merge_gather_dev(static_cast<uint8_t*>(d_k), en.keys_size, d_koff, d_vals, n, d_source, d_poff, d_counts,
                            static_cast<uint8_t*>(d_ok), en.keys_size, d_ooff, d_ovals, n, d_gst,
                            ss->stream()) != LSBM_OK)
    return Status::InvalidArgument(lsbm_crc32c_last_error());
  std::vector<uint8_t> res(res_bytes);
  e = ss->download(res.data(), d_r, res_bytes);
  if (e != hipSuccess) return hip_status(e, "merge");
  const uint64_t* w = reinterpret_cast<const uint64_t*>(res.data());
  const uint32_t* st = reinterpret_cast<const uint32_t*>(w + res_words);
  run_statuses->assign(st, st + n_runs);
  for (size_t r = 0; r < n_runs; r++)
    if (st[r] != LSBM_MERGE_OK) return merge_status(st[r], r);
  if (st[n_runs] != LSBM_MERGE_OK) return Status::IOError("internal error: merge gather failed");
  const uint64_t n_out = w[2 * n + 1], key_bytes = w[2 * n + 2];
  if (n_out > n || key_bytes > en.keys_size) return Status::IOError("internal error: merge output larger than its input");
  source->assign(w, w + n_out);
  key_offsets->assign(w + 2 * n + 3, w + 2 * n + 3 + n_out + 1);
  values->assign(w + 3 * n + 4, w + 3 * n + 4 + 2 * n_out);
  keys->assign(key_bytes, '\0');
  if (key_bytes) e = ss->download(&(*keys)[0], d_ok, key_bytes);
  if (e != hipSuccess) return hip_status(e, "merge");
  return Status::OK();
}

}  // namespace lsbm
