// get_host.cc -- host baseline of tools/bench_get.py: the lookups of a batched
// DB::Get by plain binary searches and std::string compares, on one thread and
// on several.  Our own code, C++ as tools/memtable_host.cc is.
//
// A source is a sorted run of internal keys of one length (a memtable's
// entries, or a table file's): user key ascending, tag descending.  A run holds
// sources in key order; a run flagged 1 (LEVEL0) holds one source that is
// probed when the user key is inside its range, any other run is probed at the
// source FindFile picks.  Per query the runs are walked in order and the first
// source whose Seek lands on the query's user key decides: where[q] = the run,
// or -1.  The strings are made before the clock starts.
//
//   g++ -O2 -std=c++17 -fPIC -shared -pthread -o build/libgethost.so tools/get_host.cc
//   g++ -g -O1 -std=c++17 -pthread -fsanitize=address,undefined -DGET_HOST_MAIN -o get_host_check tools/get_host.cc
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace {

uint64_t tag_of(const std::string& k) {
  uint64_t t;
  memcpy(&t, k.data() + k.size() - 8, 8);
  return t;
}

// InternalKeyComparator::Compare
int icmp(const std::string& a, const std::string& b) {
  const int c = a.compare(0, a.size() - 8, b, 0, b.size() - 8);
  if (c) return c;
  const uint64_t ta = tag_of(a), tb = tag_of(b);
  return ta > tb ? -1 : (ta < tb ? 1 : 0);
}

int ucmp(const std::string& a, const std::string& b) { return a.compare(0, a.size() - 8, b, 0, b.size() - 8); }

struct Tree {
  std::vector<std::vector<std::string>> sources;
  std::vector<uint64_t> run_first;
  std::vector<uint32_t> run_flags;
};

int32_t lookup(const Tree& t, const std::string& key) {
  for (size_t r = 0; r + 1 < t.run_first.size(); r++) {
    const uint64_t first = t.run_first[r], last = t.run_first[r + 1];
    if (first == last) continue;
    uint64_t f = first;
    if (t.run_flags[r] & 1) {
      const std::vector<std::string>& s = t.sources[f];
      if (s.empty() || ucmp(key, s.front()) < 0 || ucmp(key, s.back()) > 0) continue;
    } else {  // FindFile over the largest keys, then the smallest-key test
      uint64_t left = first, right = last;
      while (left < right) {
        const uint64_t mid = (left + right) / 2;
        if (t.sources[mid].empty() || icmp(t.sources[mid].back(), key) < 0) {
          left = mid + 1;
        } else {
          right = mid;
        }
      }
      f = right;
      if (f >= last || ucmp(key, t.sources[f].front()) < 0) continue;
    }
    const std::vector<std::string>& s = t.sources[f];
    const auto it = std::lower_bound(s.begin(), s.end(), key,
                                     [](const std::string& a, const std::string& b) { return icmp(a, b) < 0; });
    if (it != s.end() && ucmp(*it, key) == 0) return (int32_t)r;
  }
  return -1;
}

}  // namespace

// keys: every source's internal keys, key_len bytes each, source s owning keys
// [source_first[s], source_first[s + 1]).  queries: n_queries lookup keys of
// query_len bytes.  Returns the seconds the lookups took, or -1.
extern "C" double get_host_lookup(const uint8_t* keys, uint64_t key_len, const uint64_t* source_first,
                                  uint64_t n_sources, const uint64_t* run_first, const uint32_t* run_flags,
                                  uint64_t n_runs, const uint8_t* queries, uint64_t query_len, uint64_t n_queries,
                                  int threads, int32_t* where) {
  if (key_len < 8 || query_len < 8 || threads < 1) return -1;
  Tree t;
  t.sources.resize(n_sources);
  for (uint64_t s = 0; s < n_sources; s++) {
    t.sources[s].reserve(source_first[s + 1] - source_first[s]);
    for (uint64_t e = source_first[s]; e < source_first[s + 1]; e++)
      t.sources[s].emplace_back(reinterpret_cast<const char*>(keys) + e * key_len, key_len);
  }
  t.run_first.assign(run_first, run_first + n_runs + 1);
  t.run_flags.assign(run_flags, run_flags + n_runs);
  if (t.run_first.back() > n_sources) return -1;
  std::vector<std::string> qs;
  qs.reserve(n_queries);
  for (uint64_t q = 0; q < n_queries; q++)
    qs.emplace_back(reinterpret_cast<const char*>(queries) + q * query_len, query_len);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> pool;
  for (int w = 0; w < threads; w++) {
    pool.emplace_back([&, w]() {
      const uint64_t lo = n_queries * w / threads, hi = n_queries * (w + 1) / threads;
      for (uint64_t q = lo; q < hi; q++) where[q] = lookup(t, qs[q]);
    });
  }
  for (std::thread& th : pool) th.join();
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

#ifdef GET_HOST_MAIN
// Stand-alone check (for a sanitizer build): a small tree against a linear scan.
int main() {
  const uint64_t key_len = 12;  // 4-byte user keys
  std::vector<std::vector<std::string>> sources(6);
  uint32_t x = 12345;
  auto next = [&]() { return x = x * 1664525u + 1013904223u; };
  auto make = [&](uint32_t user, uint64_t seq) {
    char u[5];
    snprintf(u, sizeof u, "%04u", user % 10000);
    const uint64_t tag = seq << 8 | 1;
    std::string k(u, 4);
    k.append(reinterpret_cast<const char*>(&tag), 8);
    return k;
  };
  for (size_t s = 0; s < 2; s++)  // two overlapping sources
    for (int i = 0; i < 300; i++) sources[s].push_back(make(next() >> 8, 100 + s));
  for (size_t s = 2; s < 6; s++)  // two runs of two sources that split the key space
    for (int i = 0; i < 300; i++) sources[s].push_back(make((next() >> 8) % 5000 + (s % 2) * 5000, 10 + s));
  std::vector<uint8_t> keys;
  std::vector<uint64_t> source_first(1, 0);
  for (auto& s : sources) {
    std::sort(s.begin(), s.end(), [](const std::string& a, const std::string& b) { return icmp(a, b) < 0; });
    s.erase(std::unique(s.begin(), s.end()), s.end());
    for (const std::string& k : s) keys.insert(keys.end(), k.begin(), k.end());
    source_first.push_back(source_first.back() + s.size());
  }
  const uint64_t run_first[] = {0, 1, 2, 2, 4, 6};
  const uint32_t run_flags[] = {1, 1, 0, 0, 0};
  std::vector<uint8_t> queries;
  const uint64_t n_queries = 4000;
  for (uint64_t q = 0; q < n_queries; q++) {
    const std::string k = make(next() >> 8, 1000);
    queries.insert(queries.end(), k.begin(), k.end());
  }
  std::vector<int32_t> one(n_queries), many(n_queries);
  if (get_host_lookup(keys.data(), key_len, source_first.data(), 6, run_first, run_flags, 5, queries.data(), key_len,
                      n_queries, 1, one.data()) < 0 ||
      get_host_lookup(keys.data(), key_len, source_first.data(), 6, run_first, run_flags, 5, queries.data(), key_len,
                      n_queries, 7, many.data()) < 0)
    return 1;
  int found = 0;
  for (uint64_t q = 0; q < n_queries; q++) {
    const std::string user(reinterpret_cast<const char*>(queries.data()) + q * key_len, 4);
    int32_t want = -1;  // the first run with a source that holds the user key
    for (int r = 0; r < 5 && want < 0; r++)
      for (uint64_t s = run_first[r]; s < run_first[r + 1] && want < 0; s++)
        for (const std::string& k : sources[s])
          if (k.compare(0, 4, user) == 0) want = r;
    if (one[q] != want || many[q] != want) {
      printf("query %llu: %d / %d, want %d\n", (unsigned long long)q, one[q], many[q], want);
      return 1;
    }
    found += want >= 0;
  }
  printf("get_host: %llu lookups agree with the linear scan (%d found)\n", (unsigned long long)n_queries, found);
  return found > 0 && found < (int)n_queries ? 0 : 1;
}
#endif
