// probe_engine.cc -- the device entry points of include/lsbm_probe.h.
//
// Validates arguments and launches probe_kernels.hip on the caller's stream.
// Never plans anything on the CPU: without a usable device every entry point
// returns LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/lsbm_probe.h"
#include "engine_internal.h"
#include "probe_types.h"

namespace lsbm {

// launchers (probe_kernels.hip)
hipError_t launch_probe_plan(const ProbeArgs& a, hipStream_t stream);
hipError_t launch_probe_emit(const ProbeArgs& a, hipStream_t stream);

namespace {

constexpr uint64_t kMaxQueries = 1ull << 31;  // per call
constexpr uint64_t kMaxSlots = 1ull << 20;
constexpr uint64_t kMaxPairs = 1ull << 36;  // (query, slot) pairs

static_assert(kProbeLevels == LSBM_PROBE_LEVELS, "probe_types.h and lsbm_probe.h disagree");

// the checks both calls share; fills every input field of `a`
int probe_args(const uint8_t* d_cand, uint64_t n_slots, const uint32_t* d_slot_info, const uint32_t* d_use_len,
               const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys, uint64_t cursor_keys_size,
               const uint64_t* d_cursor_offsets, const uint8_t* d_keys, uint64_t keys_size,
               const uint64_t* d_key_offsets, uint64_t n_queries, uint32_t* d_status, ProbeArgs* a) {
  if (n_queries > kMaxQueries || n_slots > kMaxSlots || (n_slots && n_queries > kMaxPairs / n_slots))
    return engine_fail(LSBM_ERR_INVALID, "too many queries or slots");
  if (!d_status || !d_use_len || !d_wb_enabled || !d_cursor_offsets || (!d_cursor_keys && cursor_keys_size) ||
      (!d_keys && keys_size) || (n_slots && !d_slot_info) || (n_slots && n_queries && !d_cand) ||
      (n_queries && !d_key_offsets))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  *a = {};
  a->cand = d_cand;
  a->n_slots = n_slots;
  a->slot_info = d_slot_info;
  a->use_len = d_use_len;
  a->wb_enabled = d_wb_enabled;
  a->cursor_keys = d_cursor_keys;
  a->cursor_size = cursor_keys_size;
  a->cursor_offsets = d_cursor_offsets;
  a->keys = d_keys;
  a->keys_size = keys_size;
  a->key_offsets = d_key_offsets;
  a->n = n_queries;
  a->status = d_status;
  return LSBM_OK;
}

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) int lsbm_probe_plan_dev(
    const uint8_t* d_cand, uint64_t n_slots, const uint32_t* d_slot_info, const uint32_t* d_use_len,
    const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys, uint64_t cursor_keys_size,
    const uint64_t* d_cursor_offsets, const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
    uint64_t n_queries, uint32_t* d_count, uint32_t* d_status, void* stream) {
  ProbeArgs a;
  int rc = probe_args(d_cand, n_slots, d_slot_info, d_use_len, d_wb_enabled, d_cursor_keys, cursor_keys_size,
                      d_cursor_offsets, d_keys, keys_size, d_key_offsets, n_queries, d_status, &a);
  if (rc != LSBM_OK) return rc;
  if (n_queries && !d_count) return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_count, 4 * n_queries}, {d_status, 4}};
  const Range ins[] = {{d_cand, n_slots * n_queries}, {d_slot_info, 4 * n_slots}, {d_use_len, 4 * kProbeLevels},
                       {d_wb_enabled, 4 * kProbeLevels}, {d_cursor_keys, cursor_keys_size},
                       {d_cursor_offsets, 8 * (kProbeLevels + 1)}, {d_keys, keys_size},
                       {d_key_offsets, 8 * (n_queries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  a.count = d_count;
  const hipError_t e = launch_probe_plan(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "probe_count_kernel");
}

__attribute__((visibility("default"))) int lsbm_probe_emit_dev(
    const uint8_t* d_cand, uint64_t n_slots, const uint32_t* d_slot_info, const uint32_t* d_use_len,
    const uint32_t* d_wb_enabled, const uint8_t* d_cursor_keys, uint64_t cursor_keys_size,
    const uint64_t* d_cursor_offsets, const uint8_t* d_keys, uint64_t keys_size, const uint64_t* d_key_offsets,
    uint64_t n_queries, const uint64_t* d_probe_first, uint32_t* d_probe_slot, uint64_t probe_cap,
    uint32_t* d_status, void* stream) {
  ProbeArgs a;
  int rc = probe_args(d_cand, n_slots, d_slot_info, d_use_len, d_wb_enabled, d_cursor_keys, cursor_keys_size,
                      d_cursor_offsets, d_keys, keys_size, d_key_offsets, n_queries, d_status, &a);
  if (rc != LSBM_OK) return rc;
  if (probe_cap > kMaxPairs) return engine_fail(LSBM_ERR_INVALID, "too many probes");
  if (!d_probe_first || (probe_cap && !d_probe_slot)) return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const Range outs[] = {{d_probe_slot, 4 * probe_cap}, {d_status, 4}};
  const Range ins[] = {{d_cand, n_slots * n_queries}, {d_slot_info, 4 * n_slots}, {d_use_len, 4 * kProbeLevels},
                       {d_wb_enabled, 4 * kProbeLevels}, {d_cursor_keys, cursor_keys_size},
                       {d_cursor_offsets, 8 * (kProbeLevels + 1)}, {d_keys, keys_size},
                       {d_key_offsets, 8 * (n_queries + 1)}, {d_probe_first, 8 * (n_queries + 1)}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs");
  rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  a.probe_first = d_probe_first;
  a.probe_slot = d_probe_slot;
  a.probe_cap = probe_cap;
  const hipError_t e = launch_probe_emit(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, "probe_emit_kernel");
}

}  // extern "C"
