// range_host.cc -- a one-thread host loop shaped like TableCache::GetRange, for
// tools/bench_range_query.py: per (query, table) pair a lower bound of the
// start key in the table's sorted keys, then a count of entries up to the first
// one that is bytewise past the end lookup key.  Our own code over plain sorted
// arrays of fixed-length internal keys (no table format, no block cache, no
// iterator objects): a floor for the host, not the reference.
//
//   g++ -O2 -std=c++17 -fPIC -shared -o build/librangehost.so tools/range_host.cc
#include <stdint.h>
#include <string.h>

#include <chrono>

extern "C" {

// keys: every table's internal keys (ikey_len bytes each: user key, 8-byte
// tag), table t's at [table_first[t], table_first[t + 1]), sorted.  Query q has
// the lookup keys start[q], end[q] (ikey_len bytes each) and the pairs
// [pair_first[q], pair_first[q + 1]) of pair_table.  Every tag in a table is
// below the lookup keys' tag, so the internal comparator's lower bound is the
// user keys'.  counts[p] gets the pair's count.  Returns the seconds the loop took.
double range_host_count(const uint8_t* keys, uint64_t ikey_len, const uint64_t* table_first, const uint8_t* start,
                        const uint8_t* end, const uint64_t* pair_first, const int32_t* pair_table, uint64_t n_queries,
                        uint32_t* counts) {
  const uint64_t ulen = ikey_len - 8;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t q = 0; q < n_queries; q++) {
    const uint8_t* s = start + q * ikey_len;
    const uint8_t* e = end + q * ikey_len;
    for (uint64_t p = pair_first[q]; p < pair_first[q + 1]; p++) {
      const uint64_t first = table_first[pair_table[p]], last = table_first[pair_table[p] + 1];
      uint64_t lo = first, hi = last;
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (memcmp(keys + mid * ikey_len, s, ulen) < 0) {
          lo = mid + 1;
        } else {
          hi = mid;
        }
      }
      uint64_t at = lo;
      while (at < last && memcmp(keys + at * ikey_len, e, ikey_len) <= 0) at++;
      counts[p] = (uint32_t)(at - lo);
    }
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // extern "C"
