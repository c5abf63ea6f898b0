// engine_internal.h -- what the engines' entry points (*_engine.cc) share:
// the per-thread error text behind lsbm_crc32c_last_error(), the per-device
// initialisation (one std::call_once per device; LSBM_ERR_NO_DEVICE without a
// usable device), and the small argument checks and grid sizing every engine
// needs.  A new engine includes this header instead of copying them.
// Hidden symbols: not part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace lsbm {

int engine_fail(int code, const char* what);            // records `what`, returns code
int engine_fail_hip(hipError_t e, const char* what);    // LSBM_ERR_HIP
int engine_current_cus(int* cus);  // initialises the current device; its CU count
// lsbm_sst_seal_dev in one pass, the trailers stored in place as plain byte
// stores (never the compare-and-swap merge): for an image the kernel reads
// and writes over PCIe (table_checksum.cc's zero copy), where device atomics
// on host memory are not to be relied on.
int sst_seal_in_place(uint8_t* d_file, uint64_t file_bytes, const uint64_t* d_handles, const uint8_t* d_types,
                      uint64_t n_blocks, hipStream_t stream);

// initialises the current device for an entry point that sizes no grid
inline int engine_ready() {
  int cus = 0;
  return engine_current_cus(&cus);
}

// grid-stride: no more workgroups than are resident at once
inline int grid_for(int cus, uint64_t items, uint64_t per_wg, uint64_t wgs_per_cu) {
  const uint64_t wgs = (items + per_wg - 1) / per_wg;
  return (int)std::max<uint64_t>(1, std::min<uint64_t>(wgs, (uint64_t)cus * wgs_per_cu));
}

// [p, p + n) and [q, q + m) share a byte
inline bool overlap(const void* p, uint64_t n, const void* q, uint64_t m) {
  if (!p || !q || !n || !m) return false;
  const uint64_t a = reinterpret_cast<uint64_t>(p), b = reinterpret_cast<uint64_t>(q);
  return a < b + m && b < a + n;
}

struct Range {
  const void* p;
  uint64_t n;
};

// an output shares a byte with an input
template <size_t NO, size_t NI>
inline bool any_overlap(const Range (&outs)[NO], const Range (&ins)[NI]) {
  for (const Range& o : outs)
    for (const Range& i : ins)
      if (overlap(o.p, o.n, i.p, i.n)) return true;
  return false;
}

// an output shares a byte with an input or with another output
template <size_t NO, size_t NI>
inline bool aliased(const Range (&outs)[NO], const Range (&ins)[NI]) {
  for (size_t i = 0; i < NO; i++) {
    for (const Range& in : ins)
      if (overlap(outs[i].p, outs[i].n, in.p, in.n)) return true;
    for (size_t j = i + 1; j < NO; j++)
      if (overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) return true;
  }
  return false;
}

}  // namespace lsbm
