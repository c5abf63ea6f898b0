// memcut_host.cc -- the accounting of include/lsbm_memtable_cut.h on the host,
// one thread: the alternative the device call replaces (copy the two length
// arrays to the host, run this loop) and tools/bench_memcut.py's baseline.
//
//   g++ -O2 -std=c++17 -shared -fPIC -o libmemcut_host.so tools/memcut_host.cc
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DMEMCUT_HOST_MAIN
//       -o memcut_host_check tools/memcut_host.cc && ./memcut_host_check
//
// With -DMEMCUT_HOST_MAIN the program compares memcut_host() with a
// brute-force restatement (an arena that really allocates its blocks, keeps
// them in a std::vector<char*> and reports that vector's capacity; a generator
// that divides) on seeded inputs, in both modes, in one call and split in two
// through the state, and prints "memcut_host self-check ok".
#include <stdint.h>

extern "C" {

enum { MEMCUT_RECOVER = 0, MEMCUT_WRITE = 1 };
enum { MEMCUT_OK = 0, MEMCUT_NO_ROOM = 1, MEMCUT_BAD_INPUT = 2 };

// state: {have_mem, remaining, n_blocks, blocks_memory, rnd, entries_in_mem}; null: no memtable.
// ikl[e] the internal key length, vl[e] the value length (0 for a deletion).
int memcut_host(const uint32_t* ikl, const uint32_t* vl, uint64_t n_entries, const uint64_t* entry_base,
                uint64_t n_records, const uint32_t* rec_status, uint32_t mode, uint64_t write_buffer_size,
                const uint64_t* state_in, uint64_t* usage, uint64_t* mem_first, uint64_t* mem_usage, uint64_t mem_cap,
                uint64_t* counts, uint64_t* state_out);
}

namespace {

constexpr uint64_t kM = 2147483647ull, kA = 16807ull, kSeed = 0xdeadbeefull & 0x7fffffffull;
constexpr uint64_t kBlock = 4096, kHead = 8 + 8 * 12, kFresh = kBlock + 8;

inline uint64_t varint_length(uint64_t v) {
  uint64_t n = 1;
  for (; v >= 128; v >>= 7) n++;
  return n;
}

inline uint64_t next(uint64_t x) {
  const uint64_t p = x * kA;
  x = (p >> 31) + (p & kM);
  return x > kM ? x - kM : x;
}

struct Mem {
  uint64_t remaining, n_blocks, blocks_memory, cap, rnd, entries;
  void fresh() {
    remaining = kBlock - kHead, n_blocks = 1, blocks_memory = kBlock, cap = 1, rnd = kSeed, entries = 0;
  }
  uint64_t usage() const { return blocks_memory + 8 * cap; }
  void block(uint64_t bytes) {
    blocks_memory += bytes;
    if (++n_blocks > cap) cap *= 2;
  }
  void add(uint64_t L) {
    uint64_t h = 1;
    while (h < 12 && ((rnd = next(rnd)) & 3) == 0) h++;
    const uint64_t node = 8 + 8 * h, cost = ((L + 7) & ~7ull) + node;
    entries++;
    if (cost <= remaining) {  // (remaining is a multiple of 8 between entries)
      remaining -= cost;
      return;
    }
    if (L <= remaining) remaining -= L;
    else if (L > kBlock / 4) block(L);
    else block(kBlock), remaining = kBlock - L;
    const uint64_t slop = remaining & 7;
    if (node + slop <= remaining) remaining -= node + slop;
    else block(kBlock), remaining = kBlock - node;
  }
};

}  // namespace

extern "C" int memcut_host(const uint32_t* ikl, const uint32_t* vl, uint64_t n_entries, const uint64_t* entry_base,
                           uint64_t n_records, const uint32_t* rec_status, uint32_t mode, uint64_t write_buffer_size,
                           const uint64_t* state_in, uint64_t* usage, uint64_t* mem_first, uint64_t* mem_usage,
                           uint64_t mem_cap, uint64_t* counts, uint64_t* state_out) {
  if (write_buffer_size < kFresh || mode > MEMCUT_WRITE || entry_base[0] != 0 || entry_base[n_records] != n_entries)
    return MEMCUT_BAD_INPUT;
  for (uint64_t i = 0; i < n_records; i++)
    if (entry_base[i] > entry_base[i + 1]) return MEMCUT_BAD_INPUT;
  Mem m = {};
  bool have = false;
  if (state_in) {
    if (state_in[0] > 1 || state_in[1] > kBlock || (state_in[1] & 7) || (state_in[0] && !state_in[2]) ||
        state_in[4] == 0 || state_in[4] >= kM)
      return MEMCUT_BAD_INPUT;
    have = state_in[0] != 0;
    m.remaining = state_in[1], m.n_blocks = state_in[2], m.blocks_memory = state_in[3], m.rnd = state_in[4];
    m.entries = state_in[5];
    for (m.cap = 1; m.cap < m.n_blocks;) m.cap *= 2;
  }
  bool pending = have, listed = false;
  uint64_t last = have ? m.usage() : 0, n_mem = 0, continues = 0;
  auto end = [&]() {
    if (listed && n_mem <= mem_cap) mem_usage[n_mem - 1] = last;
    have = listed = pending = false, last = 0;
  };
  for (uint64_t i = 0; i < n_records; i++) {
    const uint32_t st = mode == MEMCUT_RECOVER && rec_status ? rec_status[i] : 0;
    if (st == 1 || st == 6 || st == 7) {
      usage[i] = last;
      continue;
    }
    if (mode == MEMCUT_WRITE && have && last > write_buffer_size) end();
    if (!have) m.fresh(), have = true, last = m.usage();
    else if (pending) continues = 1, pending = false;
    if (!listed) {
      if (n_mem < mem_cap) mem_first[n_mem] = i;
      n_mem++, listed = true;
    }
    for (uint64_t e = entry_base[i]; e < entry_base[i + 1]; e++)
      m.add(varint_length(ikl[e]) + ikl[e] + varint_length(vl[e]) + vl[e]);
    usage[i] = last = m.usage();
    if (mode == MEMCUT_RECOVER && last > write_buffer_size) end();
  }
  if (have && listed && n_mem <= mem_cap) mem_usage[n_mem - 1] = last;
  if (n_mem > mem_cap) return MEMCUT_NO_ROOM;
  mem_first[n_mem] = n_records;
  counts[0] = n_mem, counts[1] = continues;
  const uint64_t out[6] = {have, have ? m.remaining : 0, have ? m.n_blocks : 0, have ? m.blocks_memory : 0,
                           have ? m.rnd : kSeed, have ? m.entries : 0};
  for (int k = 0; k < 6; k++) state_out[k] = out[k];
  return MEMCUT_OK;
}

#ifdef MEMCUT_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

namespace {

// the brute force: every allocation made for real
class BruteArena {
 public:
  BruteArena() : ptr_(nullptr), left_(0), bytes_(0) {}
  char* Plain(size_t n) {
    if (n <= left_) return Take(n);
    return Fallback(n);
  }
  char* Aligned(size_t n) {
    const size_t mod = reinterpret_cast<uintptr_t>(ptr_) % 8, slop = mod ? 8 - mod : 0;
    if (n + slop <= left_) return Take(n + slop) + slop;
    return Fallback(n);
  }
  size_t Usage() const { return bytes_ + blocks_.capacity() * sizeof(char*); }

 private:
  char* Take(size_t n) {
    char* r = ptr_;
    ptr_ += n, left_ -= n;
    return r;
  }
  char* Block(size_t n) {
    blocks_.push_back(std::unique_ptr<char[]>(new char[n]));
    bytes_ += n;
    return blocks_.back().get();
  }
  char* Fallback(size_t n) {
    if (n > 1024) return Block(n);
    ptr_ = Block(4096), left_ = 4096;
    return Take(n);
  }
  char* ptr_;
  size_t left_, bytes_;
  std::vector<std::unique_ptr<char[]>> blocks_;
};

struct BruteMem {
  BruteArena arena;
  uint64_t rnd = kSeed;
  BruteMem() { arena.Aligned(kHead); }
  void Add(uint64_t ikl, uint64_t vl) {
    arena.Plain(varint_length(ikl) + ikl + varint_length(vl) + vl);
    int h = 1;
    while (h < 12) {
      rnd = rnd * 16807 % 2147483647;
      if (rnd % 4) break;
      h++;
    }
    arena.Aligned(8 + 8 * h);
  }
};

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

struct Result {
  std::vector<uint64_t> usage, first, ended;
};

Result brute(const std::vector<uint32_t>& ikl, const std::vector<uint32_t>& vl, const std::vector<uint64_t>& base,
             const std::vector<uint32_t>& status, uint32_t mode, uint64_t wbs) {
  Result r;
  std::unique_ptr<BruteMem> mem;
  uint64_t last = 0;
  for (size_t i = 0; i + 1 < base.size(); i++) {
    if (mode == MEMCUT_RECOVER && (status[i] == 1 || status[i] == 6 || status[i] == 7)) {
      r.usage.push_back(last);
      continue;
    }
    if (mode == MEMCUT_WRITE && mem && mem->arena.Usage() > wbs) r.ended.push_back(mem->arena.Usage()), mem.reset();
    if (!mem) mem.reset(new BruteMem), r.first.push_back(i);
    for (uint64_t e = base[i]; e < base[i + 1]; e++) mem->Add(ikl[e], vl[e]);
    last = mem->arena.Usage();
    r.usage.push_back(last);
    if (mode == MEMCUT_RECOVER && last > wbs) r.ended.push_back(last), mem.reset(), last = 0;
  }
  if (mem) r.ended.push_back(mem->arena.Usage());
  return r;
}

void fail(const char* what, uint64_t seed) {
  printf("memcut_host self-check FAILED: %s (seed %llu)\n", what, (unsigned long long)seed);
  exit(1);
}

}  // namespace

int main() {
  static const uint32_t kSizes[] = {0, 10, 100, 100, 100, 900, 1000, 1100, 3000, 5000, 17000};
  static const uint64_t kWbs[] = {4104, 8192, 65536, 65600, 65664, 4u << 20};
  uint64_t checked = 0;
  for (uint64_t seed = 1; seed <= 60; seed++) {
    uint64_t s = seed;
    const uint64_t n_records = splitmix(s) % 300;
    std::vector<uint32_t> ikl, vl, status;
    std::vector<uint64_t> base(1, 0);
    for (uint64_t i = 0; i < n_records; i++) {
      const uint64_t roll = splitmix(s) % 16;
      status.push_back(roll == 0 ? 1 : roll == 1 ? 2 : 0);
      const uint64_t n = status.back() == 1 ? 0 : splitmix(s) % (seed % 3 == 0 ? 40 : 4);
      for (uint64_t k = 0; k < n; k++) {
        ikl.push_back(8 + splitmix(s) % 41);
        vl.push_back(splitmix(s) % 8 == 0 ? 0 : kSizes[splitmix(s) % 11] + splitmix(s) % 9);
      }
      base.push_back(ikl.size());
    }
    for (uint64_t wbs : kWbs)
      for (uint32_t mode = 0; mode < 2; mode++) {
        const Result want = brute(ikl, vl, base, status, mode, wbs);
        std::vector<uint64_t> usage(n_records + 1), first(n_records + 2), ended(n_records + 1);
        uint64_t counts[2], state[6];
        if (memcut_host(ikl.data(), vl.data(), ikl.size(), base.data(), n_records, status.data(), mode, wbs, nullptr,
                        usage.data(), first.data(), ended.data(), n_records + 1, counts, state) != MEMCUT_OK)
          fail("status", seed);
        usage.resize(n_records), first.resize(counts[0]), ended.resize(counts[0]);
        if (usage != want.usage || first != want.first || ended != want.ended || counts[1] != 0)
          fail("one call differs from the brute force", seed);
        // the same in two calls through the state, at a seeded split
        const uint64_t at = n_records ? splitmix(s) % (n_records + 1) : 0;
        std::vector<uint64_t> b1(base.begin(), base.begin() + at + 1), b2;
        for (uint64_t i = at; i <= n_records; i++) b2.push_back(base[i] - base[at]);
        std::vector<uint64_t> u(n_records + 2), f1(n_records + 2), e1(n_records + 2), f2(n_records + 2),
            e2(n_records + 2);
        uint64_t c1[2], c2[2], s1[6], s2[6];
        if (memcut_host(ikl.data(), vl.data(), base[at], b1.data(), at, status.data(), mode, wbs, nullptr, u.data(),
                        f1.data(), e1.data(), n_records + 1, c1, s1) != MEMCUT_OK ||
            memcut_host(ikl.data() + base[at], vl.data() + base[at], ikl.size() - base[at], b2.data(), n_records - at,
                        status.data() + at, mode, wbs, s1, u.data() + at, f2.data(), e2.data(), n_records + 1, c2,
                        s2) != MEMCUT_OK)
          fail("status of a split call", seed);
        u.resize(n_records);
        std::vector<uint64_t> f(f1.begin(), f1.begin() + c1[0]), e(e1.begin(), e1.begin() + c1[0]);
        for (uint64_t k = 0; k < c2[0]; k++) {
          if (k == 0 && c2[1]) e.back() = e2[0];
          else f.push_back(f2[k] + at), e.push_back(e2[k]);
        }
        if (u != want.usage || f != want.first || e != want.ended) fail("two calls differ from one", seed);
        for (int k = 0; k < 6; k++)
          if (s2[k] != state[k]) fail("the state after two calls differs", seed);
        checked++;
      }
  }
  printf("memcut_host self-check ok: %llu runs equal the brute force, in one call and in two\n",
         (unsigned long long)checked);
  return 0;
}
#endif
