// log_read_engine.cc -- the device entry points of include/lsbm_log_read.h.
//
// Validates arguments, carves the scratch, zeroes the call's status word and
// launches log_read_kernels.hip on the caller's stream.  Never walks a log on
// the CPU: without a usable device every entry point returns
// LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_log_read.h"
#include "engine_internal.h"
#include "log_read_types.h"

namespace lsbm {

// launchers (log_read_kernels.hip)
hipError_t launch_log_walk(const LrWalkArgs& a, int block_grid, int lane_grid, hipStream_t stream);
hipError_t launch_log_plan(const LrPlan& p, int check_grid, hipStream_t stream);
hipError_t launch_log_emit(const LrEmitArgs& a, int move_grid, hipStream_t stream);

namespace {

constexpr uint64_t kMaxBytes = 1ull << 62;  // sizes, caps, offsets: below this
constexpr uint64_t kWgsPerCu = 8;
constexpr uint64_t kWalkWgsPerCu = 4;  // 32 KiB of LDS each

uint64_t tiles_of(uint64_t n) { return (n + kLrThreads - 1) / kLrThreads; }
uint64_t first_block_of(uint64_t initial_offset) {  // SkipToInitialBlock, common/log_reader.cc:35-45
  const uint64_t in_block = initial_offset % kLrBlock;
  return initial_offset / kLrBlock + (in_block > kLrBlock - 6 ? 1 : 0);
}
uint64_t blocks_of(uint64_t log_bytes, uint64_t initial_offset) {
  const uint64_t start = first_block_of(initial_offset) * kLrBlock;
  return start >= log_bytes ? 0 : (log_bytes - start + kLrBlock - 1) / kLrBlock;
}
uint64_t walk_scratch(uint64_t n_blocks) { return 8 * (3 * n_blocks + 1); }
uint64_t plan_words(uint64_t n_headers, uint64_t n_blocks) {
  const uint64_t slots = n_headers + n_blocks + 1;
  return kHdrWords + n_blocks + 8 * slots + (slots + 1) / 2 + 6 * (tiles_of(slots) + 1) + 3 * n_headers;
}

bool scratch_ok(const void* p, uint64_t have, uint64_t need) {
  return p && have >= need && !(reinterpret_cast<uint64_t>(p) & 7u);
}

void carve(LrPlan& p, void* d_scratch) {
  uint64_t* w = static_cast<uint64_t*>(d_scratch);
  const uint64_t s = p.n_slots;
  p.hdr = w, w += kHdrWords;
  p.cut = w, w += p.n_blocks;
  p.off = w, w += s;
  p.end = w, w += s;
  p.setter = w, w += s;
  p.mex = w, w += s;
  p.scr1 = w, w += s;
  p.done = w, w += s;
  p.sidex = w, w += s;
  p.fragex = w, w += s;
  p.lk = reinterpret_cast<uint32_t*>(w), w += (s + 1) / 2;
  p.tiles = w, w += 6 * (p.n_tiles + 1);
  p.ftab = w;
}

// what every step checks of the log's place in the image
const char* log_fault(const uint8_t* d_image, uint64_t image_size, uint64_t log_at, uint64_t log_bytes,
                      uint64_t initial_offset, uint64_t n_blocks) {
  if (image_size >= kMaxBytes || initial_offset >= kMaxBytes) return "image or offset too large";
  if (log_at > image_size || log_bytes > image_size - log_at) return "the log reaches outside the image";
  if (!d_image && image_size) return "null pointer";
  if (n_blocks != blocks_of(log_bytes, initial_offset)) return "n_blocks is not lsbm_log_read_blocks()";
  return nullptr;
}

int finish(hipError_t e, const char* what) { return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, what); }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_log_read_blocks(uint64_t log_bytes, uint64_t initial_offset) {
  return blocks_of(log_bytes, initial_offset);
}

__attribute__((visibility("default"))) uint64_t lsbm_log_read_plan_scratch_bytes(uint64_t n_headers,
                                                                                  uint64_t n_blocks) {
  return 8 * plan_words(n_headers, n_blocks);
}

__attribute__((visibility("default"))) uint64_t lsbm_log_read_scratch_bytes(uint64_t log_bytes) {
  const uint64_t n_blocks = blocks_of(log_bytes, 0);
  return std::max(walk_scratch(n_blocks), 8 * plan_words(log_bytes / kLrHeader, n_blocks));
}

__attribute__((visibility("default"))) int lsbm_log_read_walk_dev(
    const uint8_t* d_image, uint64_t image_size, uint64_t log_at, uint64_t log_bytes, uint64_t initial_offset,
    uint64_t* d_block_first, uint64_t* d_block_end, uint64_t n_blocks, uint64_t* d_headers, uint64_t headers_cap,
    uint64_t* d_n_headers, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (const char* f = log_fault(d_image, image_size, log_at, log_bytes, initial_offset, n_blocks))
    return engine_fail(LSBM_ERR_INVALID, f);
  if (headers_cap >= kMaxBytes / 8) return engine_fail(LSBM_ERR_INVALID, "cap too large");
  if (!d_block_first || !d_n_headers || !d_status || (n_blocks && !d_block_end))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, walk_scratch(n_blocks)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_log_read_scratch_bytes)");
  const uint64_t list = d_headers ? 8 * headers_cap : 0;
  const Range outs[] = {{d_block_first, 8 * (n_blocks + 1)}, {d_block_end, 16 * n_blocks}, {d_headers, list},
                        {d_n_headers, 8}, {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_image ? d_image + log_at : nullptr, log_bytes}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  LrWalkArgs a = {};
  a.image = d_image;
  a.log_at = log_at;
  a.log_bytes = log_bytes;
  a.first_block = first_block_of(initial_offset);
  a.n_blocks = n_blocks;
  a.block_first = d_block_first;
  a.block_end = d_block_end;
  a.headers = d_headers;
  a.headers_cap = headers_cap;
  a.n_headers = d_n_headers;
  a.status = d_status;
  a.counts = static_cast<uint64_t*>(d_scratch);
  a.ends = a.counts + n_blocks + 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess)
    e = launch_log_walk(a, grid_for(cus, n_blocks, 1, kWalkWgsPerCu), grid_for(cus, n_blocks + 1, kLrThreads, kWgsPerCu),
                        s);
  return finish(e, "log read walk kernels");
}

__attribute__((visibility("default"))) int lsbm_log_read_plan_dev(
    const uint8_t* d_image, uint64_t image_size, uint64_t log_at, uint64_t log_bytes, uint64_t initial_offset,
    const uint64_t* d_block_first, const uint64_t* d_block_end, uint64_t n_blocks, const uint64_t* d_headers,
    uint64_t n_headers, const uint8_t* d_ok, uint64_t* d_totals, uint32_t* d_status, void* d_scratch,
    uint64_t scratch_bytes, void* stream) {
  if (const char* f = log_fault(d_image, image_size, log_at, log_bytes, initial_offset, n_blocks))
    return engine_fail(LSBM_ERR_INVALID, f);
  if (n_headers > log_bytes / kLrHeader) return engine_fail(LSBM_ERR_INVALID, "more headers than the log can hold");
  if (!d_block_first || !d_totals || !d_status || (n_blocks && !d_block_end) || (n_headers && (!d_headers || !d_ok)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * plan_words(n_headers, n_blocks)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_log_read_plan_scratch_bytes)");
  const Range outs[] = {{d_totals, 32}, {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_image ? d_image + log_at : nullptr, log_bytes}, {d_block_first, 8 * (n_blocks + 1)},
                       {d_block_end, 16 * n_blocks}, {d_headers, 8 * n_headers}, {d_ok, n_headers}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  LrPlan p = {};
  p.image = d_image;
  p.log_at = log_at;
  p.log_bytes = log_bytes;
  p.initial_offset = initial_offset;
  p.first_block = first_block_of(initial_offset);
  p.n_blocks = n_blocks;
  p.block_first = d_block_first;
  p.block_end = d_block_end;
  p.headers = d_headers;
  p.n_headers = n_headers;
  p.ok = d_ok;
  p.totals = d_totals;
  p.status = d_status;
  p.n_slots = n_headers + n_blocks + 1;
  p.n_tiles = tiles_of(p.n_slots);
  carve(p, d_scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess) e = launch_log_plan(p, grid_for(cus, std::max(n_headers, n_blocks), kLrThreads, kWgsPerCu), s);
  return finish(e, "log read plan kernels");
}

__attribute__((visibility("default"))) int lsbm_log_read_emit_dev(
    uint8_t* d_image, uint64_t image_size, uint64_t log_at, uint64_t log_bytes, uint64_t initial_offset,
    uint64_t n_blocks, uint64_t n_headers, uint64_t side_at, uint64_t side_cap, uint64_t* d_records,
    uint64_t records_cap, uint64_t* d_last_record_offset, uint64_t* d_events, uint64_t events_cap, uint32_t* d_status,
    void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (const char* f = log_fault(d_image, image_size, log_at, log_bytes, initial_offset, n_blocks))
    return engine_fail(LSBM_ERR_INVALID, f);
  if (n_headers > log_bytes / kLrHeader) return engine_fail(LSBM_ERR_INVALID, "more headers than the log can hold");
  if (records_cap >= kMaxBytes / 16 || events_cap >= kMaxBytes / 32) return engine_fail(LSBM_ERR_INVALID, "cap too large");
  if (side_at > image_size || side_cap > image_size - side_at)
    return engine_fail(LSBM_ERR_INVALID, "the side area reaches outside the image");
  if (!d_status || (records_cap && (!d_records || !d_last_record_offset)) || (events_cap && !d_events))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * plan_words(n_headers, n_blocks)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_log_read_plan_scratch_bytes)");
  const uint8_t* side = d_image ? d_image + side_at : nullptr;
  const Range outs[] = {{side, side_cap}, {d_records, 16 * records_cap}, {d_last_record_offset, 8 * records_cap},
                        {d_events, 32 * events_cap}, {d_status, 4}};
  const Range ins[] = {{d_image ? d_image + log_at : nullptr, log_bytes}, {d_scratch, scratch_bytes}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  LrEmitArgs a = {};
  a.p.image = d_image;
  a.p.log_at = log_at;
  a.p.log_bytes = log_bytes;
  a.p.initial_offset = initial_offset;
  a.p.first_block = first_block_of(initial_offset);
  a.p.n_blocks = n_blocks;
  a.p.n_headers = n_headers;
  a.p.status = d_status;
  a.p.n_slots = n_headers + n_blocks + 1;
  a.p.n_tiles = tiles_of(a.p.n_slots);
  carve(a.p, d_scratch);
  a.out_image = d_image;
  a.side_at = side_at;
  a.side_cap = side_cap;
  a.records = d_records;
  a.records_cap = records_cap;
  a.last_record_offset = d_last_record_offset;
  a.events = d_events;
  a.events_cap = events_cap;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess) e = launch_log_emit(a, grid_for(cus, side_cap / kLrChunk + 2, kLrThreads, kWgsPerCu), s);
  return finish(e, "log read emit kernels");
}

}  // extern "C"
