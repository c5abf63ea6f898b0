// scan_host.cc -- host baseline of tools/bench_scan.py: a batched range scan as
// the reference shapes it, a k-way merge of sorted runs (MergingIterator) and a
// port of DBIter (lsbm/db_iter.cc: Seek, SeekToFirst, SeekToLast, Next, Prev,
// FindNextUserEntry, FindPrevUserEntry, ParseKey) over the merged keys, on one
// thread and on several over the queries.  Our own code, C++ as
// tools/get_host.cc is.
//
// Entries are internal keys (user key ascending, tag descending inside a run);
// run r owns entries [run_first[r], run_first[r+1]).  A query is the half-open
// user-key interval [lo, hi) with either bound optional, a limit and a
// direction, answered with the idioms of include/lsbm_iter.h by a fresh
// iterator; per query the count, the status (1: ParseKey met a corrupt key) and
// the merged positions of the first and the last entry taken come back.  The
// strings are made before the clock starts.
//
//   g++ -O2 -std=c++17 -fPIC -shared -pthread -o build/libscanhost.so tools/scan_host.cc
//   g++ -g -O1 -std=c++17 -pthread -fsanitize=address,undefined -DSCAN_HOST_MAIN -o scan_host_check tools/scan_host.cc
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <queue>
#include <string>
#include <thread>
#include <vector>

namespace {

uint64_t tag_of(const std::string& k) {
  uint64_t t;
  memcpy(&t, k.data() + k.size() - 8, 8);
  return t;
}

int ucmp(const std::string& a, size_t alen, const std::string& b, size_t blen) { return a.compare(0, alen, b, 0, blen); }

// InternalKeyComparator::Compare
int icmp(const std::string& a, const std::string& b) {
  const int c = ucmp(a, a.size() - 8, b, b.size() - 8);
  if (c) return c;
  const uint64_t ta = tag_of(a), tb = tag_of(b);
  return ta > tb ? -1 : (ta < tb ? 1 : 0);
}

// the merged order of the runs: the smallest key first, among equal keys the lowest run (table/merger.cc)
std::vector<std::string> merge_runs(const std::vector<std::string>& keys, const std::vector<uint64_t>& run_first) {
  struct Head {
    uint64_t at;
    uint32_t run;
  };
  auto after = [&](const Head& x, const Head& y) {
    const int c = icmp(keys[x.at], keys[y.at]);
    return c > 0 || (c == 0 && x.run > y.run);
  };
  std::priority_queue<Head, std::vector<Head>, decltype(after)> heap(after);
  for (uint32_t r = 0; r + 1 < run_first.size(); r++)
    if (run_first[r] < run_first[r + 1]) heap.push({run_first[r], r});
  std::vector<std::string> out;
  out.reserve(keys.size());
  while (!heap.empty()) {
    Head h = heap.top();
    heap.pop();
    out.push_back(keys[h.at]);
    if (++h.at < run_first[h.run + 1]) heap.push(h);
  }
  return out;
}

// db_iter.cc's DBIter over the merged keys; iter_ is a position, valid inside [0, n)
class DBIter {
 public:
  DBIter(const std::vector<std::string>& e, uint64_t sequence)
      : e_(e), n_((int64_t)e.size()), p_(n_), sequence_(sequence), forward_(true), valid_(false), corrupt_(false),
        saved_at_(-1) {}
  bool Valid() const { return valid_; }
  bool corrupt() const { return corrupt_; }
  // the merged position whose user key and value the iterator shows
  int64_t at() const { return forward_ ? p_ : saved_at_; }
  const std::string& key_holder() const { return e_[at()]; }

  void Seek(const std::string& user) {
    forward_ = true;
    std::string target = user;
    const uint64_t tag = (sequence_ << 8) | 1;
    target.append(reinterpret_cast<const char*>(&tag), 8);
    int64_t lo = 0, hi = n_;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (icmp(e_[mid], target) < 0) lo = mid + 1; else hi = mid;
    }
    p_ = lo;
    if (iter_valid()) FindNextUserEntry(false, -1); else valid_ = false;
  }
  void SeekToFirst() {
    forward_ = true;
    p_ = 0;
    if (iter_valid()) FindNextUserEntry(false, -1); else valid_ = false;
  }
  void SeekToLast() {
    forward_ = false;
    p_ = n_ - 1;
    FindPrevUserEntry();
  }
  void Next() {
    int64_t skip;
    if (!forward_) {
      forward_ = true;
      if (!iter_valid()) p_ = 0; else p_++;
      if (!iter_valid()) {
        valid_ = false;
        return;
      }
      skip = saved_at_;
    } else {
      skip = p_;
    }
    FindNextUserEntry(true, skip);
  }
  void Prev() {
    if (forward_) {
      const int64_t saved = p_;
      while (true) {
        p_--;
        if (!iter_valid()) {
          valid_ = false;
          return;
        }
        if (ucmp(e_[p_], e_[p_].size() - 8, e_[saved], e_[saved].size() - 8) < 0) break;
      }
      forward_ = false;
      saved_at_ = saved;
    }
    FindPrevUserEntry();
  }

 private:
  bool iter_valid() const { return p_ >= 0 && p_ < n_; }
  bool ParseKey(uint64_t* seq, uint32_t* type) {
    const uint64_t tag = tag_of(e_[p_]);
    *seq = tag >> 8;
    *type = (uint32_t)(tag & 0xff);
    if (*type > 1) {
      corrupt_ = true;
      return false;
    }
    return true;
  }
  // skip: the position whose user key hides what follows it (-1: none)
  void FindNextUserEntry(bool skipping, int64_t skip) {
    do {
      uint64_t seq;
      uint32_t type;
      if (ParseKey(&seq, &type) && seq <= sequence_) {
        if (type == 0) {
          skip = p_;
          skipping = true;
        } else if (!(skipping && ucmp(e_[p_], e_[p_].size() - 8, e_[skip], e_[skip].size() - 8) <= 0)) {
          valid_ = true;
          return;
        }
      }
      p_++;
    } while (iter_valid());
    valid_ = false;
  }
  void FindPrevUserEntry() {
    uint32_t value_type = 0;
    if (iter_valid()) {
      do {
        uint64_t seq;
        uint32_t type;
        if (ParseKey(&seq, &type) && seq <= sequence_) {
          if (value_type != 0 && ucmp(e_[p_], e_[p_].size() - 8, e_[saved_at_], e_[saved_at_].size() - 8) < 0) break;
          value_type = type;
          if (value_type != 0) saved_at_ = p_;
        }
        p_--;
      } while (iter_valid());
    }
    if (value_type == 0) {
      valid_ = false;
      forward_ = true;
    } else {
      valid_ = true;
    }
  }

  const std::vector<std::string>& e_;
  const int64_t n_;
  int64_t p_;
  const uint64_t sequence_;
  bool forward_, valid_, corrupt_;
  int64_t saved_at_;  // saved_key_ / saved_value_ as the position they were taken from
};

struct Query {
  bool has_lo, has_hi;
  std::string lo, hi;
  uint64_t limit;
};

struct Answer {
  uint64_t count;
  uint32_t status;
  int64_t first, last;
};

int user_vs(const std::string& ikey, const std::string& user) { return ikey.compare(0, ikey.size() - 8, user); }

Answer scan_one(const std::vector<std::string>& merged, uint64_t snapshot, const Query& q, bool reverse) {
  Answer a = {0, 0, -1, -1};
  if (q.limit == 0) return a;
  DBIter it(merged, snapshot);
  if (!reverse) {
    if (q.has_lo) it.Seek(q.lo); else it.SeekToFirst();
    while (a.count < q.limit && it.Valid() && (!q.has_hi || user_vs(it.key_holder(), q.hi) < 0)) {
      if (a.count == 0) a.first = it.at();
      a.last = it.at();
      if (++a.count == q.limit) break;
      it.Next();
    }
  } else {
    if (q.has_hi) {
      it.Seek(q.hi);
      if (it.Valid()) it.Prev(); else it.SeekToLast();
    } else {
      it.SeekToLast();
    }
    while (a.count < q.limit && it.Valid() && (!q.has_lo || user_vs(it.key_holder(), q.lo) >= 0)) {
      if (a.count == 0) a.first = it.at();
      a.last = it.at();
      if (++a.count == q.limit) break;
      it.Prev();
    }
  }
  a.status = it.corrupt() ? 1 : 0;
  return a;
}

double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

#define SCAN_HOST_API extern "C" __attribute__((visibility("default")))

// The merged keys of the runs, kept for any number of scan_host_scan calls.
// *merge_seconds = the k-way merge alone (the strings are made before).
SCAN_HOST_API void* scan_host_open(const uint8_t* keys, const uint64_t* key_offsets, uint64_t n_entries,
                                   const uint64_t* run_first, uint64_t n_runs, double* merge_seconds) {
  std::vector<std::string> entries(n_entries);
  for (uint64_t e = 0; e < n_entries; e++)
    entries[e].assign(reinterpret_cast<const char*>(keys) + key_offsets[e], key_offsets[e + 1] - key_offsets[e]);
  const std::vector<uint64_t> firsts(run_first, run_first + n_runs + 1);
  const double t0 = now();
  std::vector<std::string>* merged = new std::vector<std::string>(merge_runs(entries, firsts));
  *merge_seconds = now() - t0;
  return merged;
}

SCAN_HOST_API uint64_t scan_host_entries(const void* store) {
  return static_cast<const std::vector<std::string>*>(store)->size();
}

SCAN_HOST_API void scan_host_close(void* store) { delete static_cast<std::vector<std::string>*>(store); }

// Answers the queries on `threads` threads; returns the seconds they took.
SCAN_HOST_API double scan_host_scan(const void* store, uint64_t snapshot, const uint8_t* lo, const uint64_t* lo_offsets,
                                    const uint8_t* lo_present, const uint8_t* hi, const uint64_t* hi_offsets,
                                    const uint8_t* hi_present, uint64_t n_queries, uint64_t limit, int reverse,
                                    int threads, uint64_t* count, uint32_t* status, int64_t* first, int64_t* last) {
  const std::vector<std::string>& merged = *static_cast<const std::vector<std::string>*>(store);
  std::vector<Query> queries(n_queries);
  for (uint64_t q = 0; q < n_queries; q++) {
    Query& x = queries[q];
    x.has_lo = lo_present ? lo_present[q] != 0 : lo_offsets != nullptr;
    x.has_hi = hi_present ? hi_present[q] != 0 : hi_offsets != nullptr;
    if (x.has_lo) x.lo.assign(reinterpret_cast<const char*>(lo) + lo_offsets[q], lo_offsets[q + 1] - lo_offsets[q]);
    if (x.has_hi) x.hi.assign(reinterpret_cast<const char*>(hi) + hi_offsets[q], hi_offsets[q + 1] - hi_offsets[q]);
    x.limit = limit;
  }
  if (threads < 1) threads = 1;
  const double t0 = now();
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++)
    pool.emplace_back([&, t] {
      for (uint64_t q = t; q < n_queries; q += threads) {
        const Answer a = scan_one(merged, snapshot, queries[q], reverse != 0);
        count[q] = a.count;
        status[q] = a.status;
        first[q] = a.first;
        last[q] = a.last;
      }
    });
  for (std::thread& th : pool) th.join();
  return now() - t0;
}

// open, scan, close in one call.  seconds[0] = the merge, seconds[1] = the
// queries.  Returns the merged entry count.
SCAN_HOST_API uint64_t scan_host_run(const uint8_t* keys, const uint64_t* key_offsets, uint64_t n_entries,
                                     const uint64_t* run_first, uint64_t n_runs, uint64_t snapshot, const uint8_t* lo,
                                     const uint64_t* lo_offsets, const uint8_t* lo_present, const uint8_t* hi,
                                     const uint64_t* hi_offsets, const uint8_t* hi_present, uint64_t n_queries,
                                     uint64_t limit, int reverse, int threads, uint64_t* count, uint32_t* status,
                                     int64_t* first, int64_t* last, double* seconds) {
  void* store = scan_host_open(keys, key_offsets, n_entries, run_first, n_runs, &seconds[0]);
  seconds[1] = scan_host_scan(store, snapshot, lo, lo_offsets, lo_present, hi, hi_offsets, hi_present, n_queries, limit,
                              reverse, threads, count, status, first, last);
  const uint64_t n = scan_host_entries(store);
  scan_host_close(store);
  return n;
}

#ifdef SCAN_HOST_MAIN
// Stand-alone check: seeded histories with deletions and error keys, split
// over runs; every answer against a direct statement of what a DBIter yields
// (the newest visible version of each user key, if it is a value).
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd(uint64_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state % n;
}

std::string ikey(const std::string& user, uint64_t seq, uint32_t type) {
  std::string k = user;
  const uint64_t tag = (seq << 8) | type;
  k.append(reinterpret_cast<const char*>(&tag), 8);
  return k;
}

}  // namespace

int main() {
  int checked = 0, corrupt_seen = 0;
  for (int round = 0; round < 200; round++) {
    const uint64_t n_users = 1 + rnd(8), n_runs = 1 + rnd(4);
    std::vector<std::string> users;
    for (uint64_t i = 0; i < n_users; i++) users.push_back(std::string(rnd(4), (char)('a' + rnd(3))));
    std::vector<std::vector<std::string>> runs(n_runs);
    const uint64_t n = rnd(60);
    for (uint64_t i = 0; i < n; i++) {
      uint32_t type = rnd(3) ? 1 : 0;
      if (rnd(8) == 0) type = rnd(2) ? 2 : 255;
      runs[rnd(n_runs)].push_back(ikey(users[rnd(n_users)], 1 + rnd(30), type));
    }
    std::string blob;
    std::vector<uint64_t> offsets(1, 0), run_first(1, 0);
    for (auto& r : runs) {
      std::sort(r.begin(), r.end(), [](const std::string& a, const std::string& b) { return icmp(a, b) < 0; });
      for (const std::string& k : r) {
        blob += k;
        offsets.push_back(blob.size());
      }
      run_first.push_back(offsets.size() - 1);
    }
    // the merged order, independently: a stable sort of the concatenation
    std::vector<std::string> all;
    for (auto& r : runs) all.insert(all.end(), r.begin(), r.end());
    std::stable_sort(all.begin(), all.end(), [](const std::string& a, const std::string& b) { return icmp(a, b) < 0; });
    for (uint64_t snapshot : {(uint64_t)0, (uint64_t)1 + rnd(30), (uint64_t)((1ull << 56) - 1)}) {
      // what a DBIter yields: per user key the first visible entry, if it is a value
      std::vector<int64_t> live;
      for (size_t p = 0; p < all.size(); p++) {
        const uint64_t tag = tag_of(all[p]);
        if ((tag & 0xff) > 1 || (tag >> 8) > snapshot) continue;
        bool head = true;
        for (size_t b = p; b-- > 0;) {
          if (ucmp(all[b], all[b].size() - 8, all[p], all[p].size() - 8) != 0) break;
          const uint64_t t = tag_of(all[b]);
          if ((t & 0xff) <= 1 && (t >> 8) <= snapshot) head = false;
        }
        if (head && (tag & 0xff) == 1) live.push_back((int64_t)p);
      }
      std::string lo_blob, hi_blob;
      std::vector<uint64_t> lo_off(1, 0), hi_off(1, 0);
      std::vector<uint8_t> lo_p, hi_p;
      const uint64_t nq = 12;
      for (uint64_t q = 0; q < nq; q++) {
        lo_blob += users[rnd(n_users)];
        hi_blob += users[rnd(n_users)];
        lo_off.push_back(lo_blob.size());
        hi_off.push_back(hi_blob.size());
        lo_p.push_back(rnd(4) != 0);
        hi_p.push_back(rnd(4) != 0);
      }
      for (uint64_t limit : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1000})
        for (int reverse = 0; reverse < 2; reverse++)
          for (int threads : {1, 3}) {
            std::vector<uint64_t> count(nq);
            std::vector<uint32_t> status(nq);
            std::vector<int64_t> first(nq), last(nq);
            double seconds[2];
            const uint64_t merged = scan_host_run(
                reinterpret_cast<const uint8_t*>(blob.data()), offsets.data(), offsets.size() - 1, run_first.data(),
                n_runs, snapshot, reinterpret_cast<const uint8_t*>(lo_blob.data()), lo_off.data(), lo_p.data(),
                reinterpret_cast<const uint8_t*>(hi_blob.data()), hi_off.data(), hi_p.data(), nq, limit, reverse,
                threads, count.data(), status.data(), first.data(), last.data(), seconds);
            if (merged != all.size()) return 1;
            for (uint64_t q = 0; q < nq; q++) {
              std::vector<int64_t> want;
              for (int64_t p : live) {
                const std::string lo = lo_blob.substr(lo_off[q], lo_off[q + 1] - lo_off[q]);
                const std::string hi = hi_blob.substr(hi_off[q], hi_off[q + 1] - hi_off[q]);
                if (lo_p[q] && user_vs(all[p], lo) < 0) continue;
                if (hi_p[q] && user_vs(all[p], hi) >= 0) continue;
                want.push_back(p);
              }
              if (reverse) std::reverse(want.begin(), want.end());
              if (want.size() > limit) want.resize(limit);
              if (count[q] != want.size()) return 2;
              if (!want.empty() && (first[q] != want.front() || last[q] != want.back())) return 3;
              if (want.empty() && (first[q] != -1 || last[q] != -1)) return 4;
              if (limit == 0 && status[q] != 0) return 5;
              checked++;
              corrupt_seen += status[q];
            }
          }
    }
  }
  if (corrupt_seen == 0) return 6;
  printf("scan_host check ok: %d answers, %d with a corrupt key met\n", checked, corrupt_seen);
  return 0;
}
#endif
