// memcut_engine.cc -- the device entry points of include/lsbm_memtable_cut.h.
//
// Validates arguments, carves the scratch, sets the call's status word and
// launches memcut_kernels.hip on the caller's stream.  Never does the
// accounting on the CPU: without a usable device every entry point returns
// LSBM_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lsbm_memtable_cut.h"
#include "engine_internal.h"
#include "memcut_types.h"

namespace lsbm {

// launchers (memcut_kernels.hip)
hipError_t launch_heights(const McHeightsArgs& a, hipStream_t stream);
hipError_t launch_memcut(const McCutArgs& a, int lane_grid, hipStream_t stream);

namespace {

constexpr uint64_t kMaxEntries = 1ull << 31;  // LSBM_MEMTABLE_MAX_ENTRIES
constexpr uint64_t kWgsPerCu = 8;

// 11 n draws always hold n inserts: the cap ends an insert after 11 successes
uint64_t heights_wgs(uint64_t n) { return std::max<uint64_t>(1, (11 * n + kMcWgDraws - 1) / kMcWgDraws); }
uint64_t heights_words(uint64_t n) { return 4 * heights_wgs(n); }  // runs (16 bytes each), link (2 words each)

struct CutLayout {
  uint64_t hdr, words, uout, mem_slot, mem_use, r0, r1, h0, h1, heights, total;  // in uint64 words
};
CutLayout cut_layout(uint64_t n_entries, uint64_t n_records) {
  const uint64_t slots = n_entries + n_records;
  CutLayout l = {};
  uint64_t w = 0;
  l.hdr = w, w += kMcHdrWords;
  l.words = w, w += slots;
  l.uout = w, w += slots;
  l.mem_slot = w, w += n_records + 1;
  l.mem_use = w, w += n_records + 1;
  l.r0 = w, w += (n_entries + 1) / 2;
  l.r1 = w, w += (n_entries + 1) / 2;
  l.h0 = w, w += (n_entries + 7) / 8;
  l.h1 = w, w += (n_entries + 7) / 8;
  l.heights = w, w += heights_words(n_entries);
  l.total = w;
  return l;
}

bool scratch_ok(const void* p, uint64_t have, uint64_t need) {
  return p && have >= need && !(reinterpret_cast<uint64_t>(p) & 7u);
}

int finish(hipError_t e, const char* what) { return e == hipSuccess ? LSBM_OK : engine_fail_hip(e, what); }

}  // namespace
}  // namespace lsbm

using namespace lsbm;

extern "C" {

__attribute__((visibility("default"))) uint64_t lsbm_skiplist_heights_scratch_bytes(uint64_t n) {
  return 8 * heights_words(std::min(n, kMaxEntries));
}

__attribute__((visibility("default"))) uint64_t lsbm_memtable_cut_scratch_bytes(uint64_t n_entries,
                                                                                 uint64_t n_records) {
  return 8 * cut_layout(std::min(n_entries, kMaxEntries), std::min(n_records, kMaxEntries)).total;
}

__attribute__((visibility("default"))) int lsbm_skiplist_heights_dev(uint64_t rnd_in, uint64_t n, uint8_t* d_heights,
                                                                     uint64_t* d_rnd_out, void* d_scratch,
                                                                     uint64_t scratch_bytes, void* stream) {
  if (rnd_in == 0 || rnd_in >= kMcM) return engine_fail(LSBM_ERR_INVALID, "rnd_in is not a state of the generator");
  if (n > kMaxEntries) return engine_fail(LSBM_ERR_INVALID, "more than 2^31 inserts");
  if ((n && !d_heights) || !d_rnd_out) return engine_fail(LSBM_ERR_INVALID, "null pointer");
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * heights_words(n)))
    return engine_fail(LSBM_ERR_INVALID,
                       "scratch too small or not 8-byte aligned (lsbm_skiplist_heights_scratch_bytes)");
  const Range outs[] = {{d_heights, n}, {d_rnd_out, 8}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{nullptr, 0}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias each other");
  const int rc = engine_ready();
  if (rc != LSBM_OK) return rc;
  McHeightsArgs a = {};
  a.rnd = rnd_in;
  a.n = n;
  a.n_wgs = heights_wgs(n);
  a.heights = d_heights;
  a.rnd_out = d_rnd_out;
  a.runs = static_cast<McRun*>(d_scratch);
  a.link = static_cast<uint64_t*>(d_scratch) + 2 * a.n_wgs;
  return finish(launch_heights(a, static_cast<hipStream_t>(stream)), "skiplist heights kernels");
}

__attribute__((visibility("default"))) int lsbm_memtable_cut_dev(
    const uint64_t* d_key_offsets, uint64_t n_entries, uint64_t key_extra, const uint64_t* d_values,
    const uint8_t* d_types, const uint64_t* d_entry_base, uint64_t n_records, const uint32_t* d_rec_status,
    uint32_t mode, uint64_t write_buffer_size, const uint64_t* d_state_in, uint64_t* d_usage, uint64_t* d_mem_first,
    uint64_t* d_mem_usage, uint64_t mem_cap, uint64_t* d_counts, uint64_t* d_state_out, uint32_t* d_status,
    void* d_scratch, uint64_t scratch_bytes, void* stream) {
  if (n_entries > kMaxEntries || n_records > kMaxEntries || mem_cap > kMaxEntries)
    return engine_fail(LSBM_ERR_INVALID, "more than 2^31 entries, records or memtables");
  if (mode != kMcRecover && mode != kMcWrite) return engine_fail(LSBM_ERR_INVALID, "mode is not RECOVER or WRITE");
  if (key_extra != 0 && key_extra != 8) return engine_fail(LSBM_ERR_INVALID, "key_extra is not 0 or 8");
  if (!d_key_offsets || !d_entry_base || !d_mem_first || !d_counts || !d_state_out || !d_status ||
      (n_entries && !d_values) || (n_records && !d_usage) || (mem_cap && !d_mem_usage))
    return engine_fail(LSBM_ERR_INVALID, "null pointer");
  const CutLayout l = cut_layout(n_entries, n_records);
  if (!scratch_ok(d_scratch, scratch_bytes, 8 * l.total))
    return engine_fail(LSBM_ERR_INVALID, "scratch too small or not 8-byte aligned (lsbm_memtable_cut_scratch_bytes)");
  const Range outs[] = {{d_usage, 8 * n_records}, {d_mem_first, 8 * (mem_cap + 1)}, {d_mem_usage, 8 * mem_cap},
                        {d_counts, 16}, {d_state_out, 48}, {d_status, 4}, {d_scratch, scratch_bytes}};
  const Range ins[] = {{d_key_offsets, 8 * (n_entries + 1)}, {d_values, 16 * n_entries},
                       {d_types, d_types ? n_entries : 0}, {d_entry_base, 8 * (n_records + 1)},
                       {d_rec_status, d_rec_status ? 4 * n_records : 0}, {d_state_in, d_state_in ? 48u : 0u}};
  if (aliased(outs, ins)) return engine_fail(LSBM_ERR_INVALID, "outputs alias inputs or each other");
  int cus = 0;
  const int rc = engine_current_cus(&cus);
  if (rc != LSBM_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (write_buffer_size < kMcFresh)  // a fresh memtable is already larger
    return finish(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_status), (int)kMcBadInput, 1, s),
                  "memtable cut status");
  uint64_t* w = static_cast<uint64_t*>(d_scratch);
  McHeightsArgs h = {};
  h.n = n_entries;
  h.n_wgs = heights_wgs(n_entries);
  h.runs = reinterpret_cast<McRun*>(w + l.heights);
  h.link = w + l.heights + 2 * h.n_wgs;
  McCutArgs a = {};
  a.key_offsets = d_key_offsets;
  a.key_extra = key_extra;
  a.values = d_values;
  a.types = d_types;
  a.entry_base = d_entry_base;
  a.rec_status = d_rec_status;
  a.n_entries = n_entries;
  a.n_records = n_records;
  a.n_slots = n_entries + n_records;
  a.mode = mode;
  const char* walk = getenv("LSBM_MEMCUT_WALK");  // "lane": the one-lane walk (a diagnostic, for A/B measurements)
  a.one_lane = walk && !strcmp(walk, "lane");
  a.write_buffer_size = write_buffer_size;
  a.state_in = d_state_in;
  a.usage = d_usage;
  a.mem_first = d_mem_first;
  a.mem_usage = d_mem_usage;
  a.mem_cap = mem_cap;
  a.counts = d_counts;
  a.state_out = d_state_out;
  a.status = d_status;
  a.hdr = w + l.hdr;
  a.words = w + l.words;
  a.uout = w + l.uout;
  a.mem_slot = w + l.mem_slot;
  a.mem_use = w + l.mem_use;
  a.h0 = reinterpret_cast<const uint8_t*>(w + l.h0);
  a.r0 = reinterpret_cast<const uint32_t*>(w + l.r0);
  // Both tables are made for all n_entries, which is more than any run needs (a memtable that begins at entry k
  // takes at most n_entries - k heights, the state's memtable those up to its end): the walk decides where
  // memtables begin, so the tables are made before it, once, at 5 bytes of scratch an entry each and about 0.04 ms
  // per million entries.  A caller short of scratch can cut a long input in two calls through the state.
  hipError_t e = hipMemsetAsync(d_status, 0, 4, s);
  if (e == hipSuccess && n_entries) {  // the heights of a new memtable's inserts
    h.rnd = kMcSeed;
    h.heights = reinterpret_cast<uint8_t*>(w + l.h0);
    h.rnd_after = reinterpret_cast<uint32_t*>(w + l.r0);
    e = launch_heights(h, s);
  }
  if (e == hipSuccess && n_entries && d_state_in) {  // and of the memtable the state carries in
    h.d_rnd = d_state_in + 4;
    h.heights = reinterpret_cast<uint8_t*>(w + l.h1);
    h.rnd_after = reinterpret_cast<uint32_t*>(w + l.r1);
    e = launch_heights(h, s);
  }
  if (d_state_in) {
    a.h1 = reinterpret_cast<const uint8_t*>(w + l.h1);
    a.r1 = reinterpret_cast<const uint32_t*>(w + l.r1);
  }
  if (e == hipSuccess)
    e = launch_memcut(a, grid_for(cus, std::max(a.n_slots, n_records + 1), kMcThreads, kWgsPerCu), s);
  return finish(e, "memtable cut kernels");
}

}  // extern "C"
