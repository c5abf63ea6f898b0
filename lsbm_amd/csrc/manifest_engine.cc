// manifest_engine.cc -- the device entry points of include/lsbm_manifest.h.
//
// Validates arguments, carves the scratch, zeroes the call's status word and
// launches manifest_kernels.hip on the caller's stream.  Never parses or
// writes an edit on the CPU: without a usable device every entry point
// returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_manifest.h"
#include "engine_internal.h"
#include "manifest_types.h"

namespace lsbm {

// launchers (manifest_kernels.hip)
hipError_t launch_edit_decode_plan(const MfDecode& a, int lane_grid, int rec_grid, hipStream_t stream);
hipError_t launch_edit_decode_emit(const MfDecode& a, hipStream_t stream);
hipError_t launch_edit_encode_plan(const MfEncode& a, int grid, hipStream_t stream);
hipError_t launch_edit_encode_emit(const MfEncode& a, int grid, hipStream_t stream);

namespace {

constexpr uint64_t kMaxBytes = 1ull << 62;          // sizes, caps, offsets: below this
constexpr uint64_t kMaxSpan = (1ull << 32) - 64;    // positions and terminals are 32-bit words
constexpr uint64_t kMaxCount = 1ull << 31;
constexpr uint64_t kWgsPerCu = 8;

uint64_t tiles_of(uint64_t n) { return (n + kMfThreads - 1) / kMfThreads; }

uint64_t decode_words(uint64_t n, uint64_t span) {
  return kMhWords + (n + 1) + kMfSlots * n + 3 * (tiles_of(span) + 1) + (n + 1) / 2 + 2 * ((span + 1) / 2) +
         (span + 7) / 8;
}
uint64_t encode_words(uint64_t n, uint64_t n_del, uint64_t n_new) {
  return kMhWords + (n + 1) + (n_del + 1) + (n_new + 1) + tiles_of(std::max(n, std::max(n_del, n_new))) + 1;
}

bool scratch_ok(const void* p, uint64_t have, uint64_t need) {
  return p && have >= need && !(reinterpret_cast<uint64_t>(p) & 7u);
}

void carve(MfDecode& a, void* d_scratch) {
  uint64_t* w = static_cast<uint64_t*>(d_scratch);
  a.n_tiles = tiles_of(a.span_cap);
  a.hdr = w, w += kMhWords;
  a.rec_first = w, w += a.n + 1;
  a.win = w, w += kMfSlots * a.n;
  a.tiles = w, w += 3 * (a.n_tiles + 1);
  a.ver = reinterpret_cast<uint32_t*>(w), w += (a.n + 1) / 2;
  a.nxt_a = reinterpret_cast<uint32_t*>(w), w += (a.span_cap + 1) / 2;
  a.nxt_b = reinterpret_cast<uint32_t*>(w), w += (a.span_cap + 1) / 2;
  a.kind = reinterpret_cast<uint8_t*>(w);
}

void carve(MfEncode& a, void* d_scratch) {
  uint64_t* w = static_cast<uint64_t*>(d_scratch);
  a.hdr = w, w += kMhWords;
  a.pe = w, w += a.n + 1;
  a.pd = w, w += a.n_del + 1;
  a.pn = w, w += a.n_new + 1;
  a.tiles = w;
}

// The smallest tag group is 2 bytes: a record of `longest` bytes is a chain of
// at most longest / 2 groups, which ceil(log2(longest / 2)) doublings cover;
// one more brings the chain's end to its first position.
uint32_t rounds_for(uint64_t longest) {
  uint32_t k = 0;
  while ((1ull << k) < std::max<uint64_t>(longest / 2, 1)) k++;
  return k + 1;
}

const char* decode_fault(const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n,
                         uint64_t span_cap) {
  if (image_size >= kMaxBytes) return "image too large";
  if (n >= kMaxCount) return "too many records";
  if (span_cap > kMaxSpan) return "span_cap is 2^32 - 64 or more";
  if ((!d_image && image_size) || (n && !d_records)) return "null pointer";
  return nullptr;
}

const char* encode_fault(const uint64_t* d_fields, const uint8_t* d_names, uint64_t names_size, uint64_t n,
                         const uint64_t* d_del_first, const uint64_t* d_del_items, uint64_t n_del,
                         const uint64_t* d_new_first, const uint64_t* d_new_items, uint64_t n_new, const uint8_t* d_keys,
                         const uint64_t* d_key_offsets, uint64_t keys_size, uint64_t out_at) {
  if (names_size >= kMaxBytes || keys_size >= kMaxBytes || out_at >= kMaxBytes) return "size or offset too large";
  if (n >= kMaxCount || n_del >= kMaxBytes / 64 || n_new >= kMaxBytes / 64) return "too many edits or items";
  if (!d_del_first || !d_new_first || !d_key_offsets || (n && !d_fields) || (names_size && !d_names) ||
      (n_del && !d_del_items) || (n_new && !d_new_items) || (keys_size && !d_keys))
    return "null pointer";
  return nullptr;
}

int finish(hipError_t e, const char* what) { return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, what); }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_edit_decode_scratch_bytes(uint64_t n, uint64_t span_cap) {
  return 8 * decode_words(n, span_cap);
}

__attribute__((visibility("default"))) uint64_t lsbm_edit_encode_scratch_bytes(uint64_t n, uint64_t n_del,
                                                                                uint64_t n_new) {
  return 8 * encode_words(n, n_del, n_new);
}

__attribute__((visibility("default"))) int lsbm_edit_decode_plan_dev(
    const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n, uint64_t span_cap,
    uint64_t longest_cap, uint32_t* d_verdict, uint64_t* d_fields, uint64_t* d_new_first, uint64_t* d_del_first,
    uint64_t* d_totals, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (const char* f = decode_fault(d_image, image_size, d_records, n, span_cap)) return engine_fail(LSBM_ERR_INVALID, f);
  if (!d_new_first || !d_del_first || !d_totals || !d_status || (n && (!d_verdict || !d_fields)))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * decode_words(n, span_cap)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_edit_decode_scratch_bytes)");
  const Range outs[] = {{d_verdict, 4 * n}, {d_fields, 8 * kMfFieldWords * n}, {d_new_first, 8 * (n + 1)},
                        {d_del_first, 8 * (n + 1)}, {d_totals, 24}, {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_image, image_size}, {d_records, 16 * n}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  MfDecode a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.records = d_records;
  a.n = n;
  a.span_cap = span_cap;
  a.longest_cap = std::min(longest_cap, span_cap);
  a.rounds = rounds_for(a.longest_cap);
  a.verdict = d_verdict;
  a.fields = d_fields;
  a.new_first = d_new_first;
  a.del_first = d_del_first;
  a.totals = d_totals;
  a.status = d_status;
  carve(a, d_scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess)
    e = launch_edit_decode_plan(a, grid_for(cus, std::max(span_cap, kMfSlots * n), kMfThreads, kWgsPerCu),
                                grid_for(cus, n, kMfThreads, kWgsPerCu), s);
  return finish(e, "edit decode plan kernels");
}

__attribute__((visibility("default"))) int lsbm_edit_decode_emit_dev(
    const uint8_t* d_image, uint64_t image_size, const uint64_t* d_records, uint64_t n, uint64_t span_cap,
    uint64_t* d_new_items, uint64_t new_cap, uint64_t* d_key_offsets, uint8_t* d_keys, uint64_t keys_cap,
    uint64_t* d_del_items, uint64_t del_cap, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
    void* stream) {
  if (const char* f = decode_fault(d_image, image_size, d_records, n, span_cap)) return engine_fail(LSBM_ERR_INVALID, f);
  if (new_cap >= kMaxBytes / 64 || del_cap >= kMaxBytes / 64 || keys_cap >= kMaxBytes)
    return engine_fail(LSBM_ERR_INVALID, "cap too large");
  if (!d_key_offsets || !d_status || (new_cap && !d_new_items) || (keys_cap && !d_keys) || (del_cap && !d_del_items))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * decode_words(n, span_cap)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_edit_decode_scratch_bytes)");
  const Range outs[] = {{d_new_items, 8 * kNewWords * new_cap}, {d_key_offsets, 8 * (2 * new_cap + 1)},
                        {d_keys, keys_cap}, {d_del_items, 8 * kDelWords * del_cap}, {d_status, 4}};
  const Range ins[] = {{d_image, image_size}, {d_records, 16 * n}, {d_scratch, scratch_bytes}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  MfDecode a = {};
  a.image = d_image;
  a.image_size = image_size;
  a.records = d_records;
  a.n = n;
  a.span_cap = span_cap;
  a.status = d_status;
  a.new_items = d_new_items;
  a.new_cap = new_cap;
  a.key_offsets = d_key_offsets;
  a.keys = d_keys;
  a.keys_cap = keys_cap;
  a.del_items = d_del_items;
  a.del_cap = del_cap;
  carve(a, d_scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess) e = launch_edit_decode_emit(a, s);
  return finish(e, "edit decode emit kernels");
}

__attribute__((visibility("default"))) int lsbm_edit_encode_plan_dev(
    const uint64_t* d_fields, const uint8_t* d_names, uint64_t names_size, uint64_t n, const uint64_t* d_del_first,
    const uint64_t* d_del_items, uint64_t n_del, const uint64_t* d_new_first, const uint64_t* d_new_items,
    uint64_t n_new, const uint8_t* d_keys, const uint64_t* d_key_offsets, uint64_t keys_size, uint64_t out_at,
    uint64_t* d_records, uint64_t* d_totals, uint32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
    void* stream) {
  if (const char* f = encode_fault(d_fields, d_names, names_size, n, d_del_first, d_del_items, n_del, d_new_first,
                                   d_new_items, n_new, d_keys, d_key_offsets, keys_size, out_at))
    return engine_fail(LSBM_ERR_INVALID, f);
  if (!d_totals || !d_status || (n && !d_records)) return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * encode_words(n, n_del, n_new)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_edit_encode_scratch_bytes)");
  const Range outs[] = {{d_records, 16 * n}, {d_totals, 8}, {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_fields, 8 * kMfFieldWords * n}, {d_names, names_size}, {d_del_first, 8 * (n + 1)},
                       {d_del_items, 8 * kDelWords * n_del}, {d_new_first, 8 * (n + 1)},
                       {d_new_items, 8 * kNewWords * n_new}, {d_keys, keys_size}, {d_key_offsets, 8 * (2 * n_new + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  MfEncode a = {};
  a.fields = d_fields;
  a.names = d_names;
  a.names_size = names_size;
  a.n = n;
  a.del_first = d_del_first;
  a.del_items = d_del_items;
  a.n_del = n_del;
  a.new_first = d_new_first;
  a.new_items = d_new_items;
  a.n_new = n_new;
  a.keys = d_keys;
  a.key_offsets = d_key_offsets;
  a.keys_size = keys_size;
  a.out_at = out_at;
  a.records = d_records;
  a.totals = d_totals;
  a.status = d_status;
  carve(a, d_scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess)
    e = launch_edit_encode_plan(a, grid_for(cus, std::max(n, std::max(n_del, n_new)), kMfThreads, kWgsPerCu), s);
  return finish(e, "edit encode plan kernels");
}

__attribute__((visibility("default"))) int lsbm_edit_encode_emit_dev(
    const uint64_t* d_fields, const uint8_t* d_names, uint64_t names_size, uint64_t n, const uint64_t* d_del_first,
    const uint64_t* d_del_items, uint64_t n_del, const uint64_t* d_new_first, const uint64_t* d_new_items,
    uint64_t n_new, const uint8_t* d_keys, const uint64_t* d_key_offsets, uint64_t keys_size, uint8_t* d_image,
    uint64_t image_size, uint64_t out_at, uint64_t out_cap, uint32_t* d_status, void* d_scratch,
    uint64_t scratch_bytes, void* stream) {
  if (const char* f = encode_fault(d_fields, d_names, names_size, n, d_del_first, d_del_items, n_del, d_new_first,
                                   d_new_items, n_new, d_keys, d_key_offsets, keys_size, out_at))
    return engine_fail(LSBM_ERR_INVALID, f);
  if (image_size >= kMaxBytes || out_at > image_size || out_cap > image_size - out_at)
    return engine_fail(LSBM_ERR_INVALID, "the output reaches outside the image");
  if (!d_status || (out_cap && !d_image)) return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * encode_words(n, n_del, n_new)))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_edit_encode_scratch_bytes)");
  const Range outs[] = {{d_image ? d_image + out_at : nullptr, out_cap}, {d_status, 4}};
  const Range ins[] = {{d_fields, 8 * kMfFieldWords * n}, {d_names, names_size}, {d_del_first, 8 * (n + 1)},
                       {d_del_items, 8 * kDelWords * n_del}, {d_new_first, 8 * (n + 1)},
                       {d_new_items, 8 * kNewWords * n_new}, {d_keys, keys_size}, {d_key_offsets, 8 * (2 * n_new + 1)},
                       {d_scratch, scratch_bytes}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  MfEncode a = {};
  a.fields = d_fields;
  a.names = d_names;
  a.names_size = names_size;
  a.n = n;
  a.del_first = d_del_first;
  a.del_items = d_del_items;
  a.n_del = n_del;
  a.new_first = d_new_first;
  a.new_items = d_new_items;
  a.n_new = n_new;
  a.keys = d_keys;
  a.key_offsets = d_key_offsets;
  a.keys_size = keys_size;
  a.out_at = out_at;
  a.status = d_status;
  a.image = d_image;
  a.out_cap = out_cap;
  carve(a, d_scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess)
    e = launch_edit_encode_emit(a, grid_for(cus, std::max(n, std::max(n_del, n_new)), kMfThreads, kWgsPerCu), s);
  return finish(e, "edit encode emit kernels");
}

}  // extern "C"
