// buffered_host.cc -- a host loop of our own, one thread, shaped like lsbm's
// Version::Get over the sorted-table lists (lsbm/version_set.cc:349-623), for
// tools/bench_buffered_get.py.  A sorted table is one file: fixed-length user
// keys in order (every entry a value at one sequence).  FindFile is the range
// test of the one file; ContainKey and the table read are a binary search with
// memcmp.  There is no filter, so no false positive: where a filter's false
// positive opens a gate (covered_by_head lets the warm-up walk run), the
// reference and the GPU may take another table's entry than this loop; the
// bench reports the share of equal answers.  The walk, its gates and its
// counters are the reference's.  Built by the bench into build/.
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <vector>

namespace {

struct Table {
  const uint8_t* keys;
  uint64_t n;
};

struct Tree {
  const Table* tables;
  uint64_t klen;
  const int32_t* level0;  // table ids in probe order
  uint64_t n_level0;
  const int32_t* del;       // [4] table id or -1
  const int32_t* ins;       // [4]
  const int32_t* cb;        // the lists from their heads, -1 an empty table
  const uint64_t* cb_first;  // [5]
  const int32_t* wb;
  const uint64_t* wb_first;  // [5]
  const int32_t* use_len;    // [4]
  int buffered_merge;
};

inline bool offered(const Tree& t, int32_t id, const uint8_t* q) {
  if (id < 0) return false;
  const Table& f = t.tables[id];
  return f.n && memcmp(q, f.keys, t.klen) >= 0 && memcmp(q, f.keys + (f.n - 1) * t.klen, t.klen) <= 0;
}

inline bool contains(const Tree& t, int32_t id, const uint8_t* q) {
  const Table& f = t.tables[id];
  uint64_t lo = 0, hi = f.n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (memcmp(f.keys + mid * t.klen, q, t.klen) < 0) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo < f.n && memcmp(f.keys + lo * t.klen, q, t.klen) == 0;
}

// the walk of one list from `start` round to `stop`: `checked++ > limit` ends it
inline void walk(const Tree& t, const int32_t* list, uint64_t len, uint64_t start, uint64_t stop, int checked,
                 int limit, const uint8_t* q, std::vector<int32_t>* files) {
  uint64_t cur = start;
  do {
    if (checked++ > limit) break;
    if (offered(t, list[cur], q)) files->push_back(list[cur]);
    cur = (cur + 1) % len;
  } while (cur != stop);
}

int32_t get(const Tree& t, const uint8_t* q, std::vector<int32_t>* files) {
  for (uint64_t i = 0; i < t.n_level0; i++)
    if (offered(t, t.level0[i], q) && contains(t, t.level0[i], q)) return t.level0[i];
  for (int level = 1; level < 4; level++) {
    const bool checkwb = t.buffered_merge && level > 1 && t.use_len[level - 1] > 0;  // (the cursor keys are empty)
    const int32_t* cb = t.cb + t.cb_first[level];
    const uint64_t cb_len = t.cb_first[level + 1] - t.cb_first[level];
    const int32_t* wb = t.wb + t.wb_first[level];
    const uint64_t wb_len = t.wb_first[level + 1] - t.wb_first[level];
    const uint64_t head = 1 % cb_len;
    files->clear();
    const bool covered_by_del = t.use_len[level] == 0 && offered(t, t.del[level], q);
    if (covered_by_del && contains(t, t.del[level], q)) {
      if (checkwb) walk(t, wb, wb_len, 1 % wb_len, 1 % wb_len, 0, t.use_len[level - 1], q, files);
      files->push_back(t.del[level]);
      for (int32_t f : *files)
        if (contains(t, f, q)) return f;
    }
    files->clear();
    if (offered(t, t.ins[level], q) && contains(t, t.ins[level], q)) {
      if (!covered_by_del) {
        bool covered_by_head = false;
        if (t.use_len[level] > 0 && cb[head] >= 0)
          covered_by_head = offered(t, cb[head], q) && contains(t, cb[head], q);
        if ((t.use_len[level] == 0 || covered_by_head) && checkwb)
          walk(t, wb, wb_len, 1 % wb_len, 1 % wb_len, 0, t.use_len[level - 1], q, files);
        if (covered_by_head) files->push_back(cb[head]);
      }
      walk(t, cb, cb_len, (head + 1) % cb_len, head, 2, t.use_len[level], q, files);
      files->push_back(t.ins[level]);
      for (int32_t f : *files)
        if (contains(t, f, q)) return f;
    }
  }
  return -1;
}

}  // namespace

// Seconds for n_queries lookups on one thread; where[q] = the table that
// holds the answer, or -1.
extern "C" double buffered_host_get(const uint8_t* keys, uint64_t klen, const uint64_t* table_first, uint64_t n_tables,
                                    const int32_t* level0, uint64_t n_level0, const int32_t* del, const int32_t* ins,
                                    const int32_t* cb, const uint64_t* cb_first, const int32_t* wb,
                                    const uint64_t* wb_first, const int32_t* use_len, int buffered_merge,
                                    const uint8_t* queries, uint64_t n_queries, int32_t* where) {
  std::vector<Table> tables(n_tables);
  for (uint64_t i = 0; i < n_tables; i++)
    tables[i] = {keys + table_first[i] * klen, table_first[i + 1] - table_first[i]};
  const Tree t = {tables.data(), klen, level0, n_level0, del, ins, cb, cb_first, wb, wb_first, use_len, buffered_merge};
  std::vector<int32_t> files;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t q = 0; q < n_queries; q++) where[q] = get(t, queries + q * klen, &files);
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
