// memtable_host.cc -- host baselines for tools/bench_memtable.py (DESIGN.md
// section 16).  Our own code in the reference's shape:
//
//   memtable_host_insert  WriteBatch::Iterate over every record and, per entry,
//                         MemTable::Add: the entry encoded into an arena
//                         (varint32 internal-key length, user key, fixed64 tag,
//                         varint32 value length, value) and inserted into a
//                         skiplist (max height 12, branching 4) under the
//                         internal-key comparator; then one walk of level 0.
//                         One thread, as the reference runs it.
//   memtable_host_sort    std::sort of the decoded entries' indices under the
//                         same order, in `threads` chunks that are then merged
//                         pairwise (std::inplace_merge), the pairs in parallel.
//
// Build: g++ -O2 -std=c++17 -fPIC -shared -pthread -o libmemtablehost.so memtable_host.cc
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

namespace {

const uint8_t* get_varint32(const uint8_t* p, uint32_t* v) {
  uint32_t result = 0;
  for (uint32_t shift = 0; shift <= 28; shift += 7) {
    const uint32_t byte = *p++;
    if (byte & 128) {
      result |= (byte & 127) << shift;
    } else {
      *v = result | (byte << shift);
      return p;
    }
  }
  return nullptr;
}

uint8_t* put_varint32(uint8_t* p, uint32_t v) {
  while (v >= 128) {
    *p++ = (uint8_t)(v | 128);
    v >>= 7;
  }
  *p++ = (uint8_t)v;
  return p;
}

// InternalKeyComparator over two internal keys
inline int compare_internal(const uint8_t* a, size_t alen, const uint8_t* b, size_t blen) {
  const size_t ua = alen - 8, ub = blen - 8, m = ua < ub ? ua : ub;
  int r = memcmp(a, b, m);
  if (r == 0) r = ua < ub ? -1 : (ua > ub ? 1 : 0);
  if (r == 0) {
    uint64_t ta, tb;
    memcpy(&ta, a + ua, 8);
    memcpy(&tb, b + ub, 8);
    r = ta > tb ? -1 : (ta < tb ? 1 : 0);
  }
  return r;
}

struct Arena {
  std::vector<uint8_t*> blocks;
  uint8_t* at = nullptr;
  size_t left = 0;
  uint8_t* allocate(size_t n) {
    n = (n + 7) & ~(size_t)7;
    if (n > left) {
      const size_t size = n > (4u << 20) ? n : (4u << 20);
      blocks.push_back(new uint8_t[size]);
      at = blocks.back();
      left = size;
    }
    uint8_t* p = at;
    at += n;
    left -= n;
    return p;
  }
  ~Arena() {
    for (uint8_t* b : blocks) delete[] b;
  }
};

constexpr int kMaxHeight = 12;

struct Node {
  const uint8_t* entry;  // varint32 internal-key length, the key, ...
  uint64_t arrival;
  Node* next[1];
};

struct SkipList {
  Arena* arena;
  Node* head;
  int height = 1;
  uint32_t seed = 0xdeadbeef & 0x7fffffffu;
  explicit SkipList(Arena* a) : arena(a) {
    head = new_node(nullptr, 0, kMaxHeight);
    for (int i = 0; i < kMaxHeight; i++) head->next[i] = nullptr;
  }
  Node* new_node(const uint8_t* entry, uint64_t arrival, int h) {
    Node* n = reinterpret_cast<Node*>(arena->allocate(sizeof(Node) + sizeof(Node*) * (h - 1)));
    n->entry = entry;
    n->arrival = arrival;
    return n;
  }
  uint32_t next_random() {  // util/random.h's generator
    const uint32_t M = 2147483647u;
    const uint64_t product = (uint64_t)seed * 16807u;
    seed = (uint32_t)((product >> 31) + (product & M));
    if (seed > M) seed -= M;
    return seed;
  }
  int random_height() {
    int h = 1;
    while (h < kMaxHeight && (next_random() % 4) == 0) h++;
    return h;
  }
  static int compare(const uint8_t* a, const uint8_t* b) {
    uint32_t alen = 0, blen = 0;
    const uint8_t* ka = get_varint32(a, &alen);
    const uint8_t* kb = get_varint32(b, &blen);
    return compare_internal(ka, alen, kb, blen);
  }
  void insert(const uint8_t* entry, uint64_t arrival) {
    Node* prev[kMaxHeight];
    Node* x = head;
    int level = height - 1;
    while (true) {  // FindGreaterOrEqual
      Node* next = x->next[level];
      if (next != nullptr && compare(next->entry, entry) < 0) {
        x = next;
      } else {
        prev[level] = x;
        if (level == 0) break;
        level--;
      }
    }
    const int h = random_height();
    if (h > height) {
      for (int i = height; i < h; i++) prev[i] = head;
      height = h;
    }
    Node* n = new_node(entry, arrival, h);
    for (int i = 0; i < h; i++) {
      n->next[i] = prev[i]->next[i];
      prev[i]->next[i] = n;
    }
  }
};

struct Less {
  const uint8_t* keys;
  const uint64_t* koff;
  bool operator()(uint32_t a, uint32_t b) const {
    const int r = compare_internal(keys + koff[a], koff[a + 1] - koff[a], keys + koff[b], koff[b + 1] - koff[b]);
    return r ? r < 0 : a > b;
  }
};

}  // namespace

extern "C" {

// Returns the number of entries inserted, or -1 for a malformed record;
// out_order[j] = arrival index of the entry at iteration position j.
long long memtable_host_insert(const uint8_t* image, const uint64_t* records, uint64_t n_records, uint64_t* out_order,
                               uint64_t order_cap) {
  Arena arena;
  SkipList list(&arena);
  uint64_t arrival = 0;
  for (uint64_t r = 0; r < n_records; r++) {
    const uint8_t* p = image + records[2 * r];
    const uint8_t* end = p + records[2 * r + 1];
    if (end - p < 12) continue;
    uint64_t seq;
    memcpy(&seq, p, 8);
    p += 12;
    while (p < end) {
      const uint8_t tag = *p++;
      uint32_t klen = 0, vlen = 0;
      const uint8_t* k = get_varint32(p, &klen);
      if (tag > 1 || k == nullptr || k + klen > end) return -1;
      p = k + klen;
      const uint8_t* v = p;
      if (tag == 1) {
        v = get_varint32(p, &vlen);
        if (v == nullptr || v + vlen > end) return -1;
        p = v + vlen;
      }
      // MemTable::Add
      uint8_t* buf = arena.allocate(5 + klen + 8 + 5 + vlen);
      uint8_t* q = put_varint32(buf, klen + 8);
      memcpy(q, k, klen);
      q += klen;
      const uint64_t packed = (seq << 8) | tag;
      memcpy(q, &packed, 8);
      q = put_varint32(q + 8, vlen);
      memcpy(q, v, vlen);
      list.insert(buf, arrival++);
      seq++;
    }
  }
  uint64_t j = 0;
  for (Node* x = list.head->next[0]; x != nullptr && j < order_cap; x = x->next[0]) out_order[j++] = x->arrival;
  return (long long)arrival;
}

int memtable_host_sort(const uint8_t* keys, const uint64_t* koff, uint64_t n, uint32_t* order, int threads) {
  if (threads < 1) threads = 1;
  for (uint64_t i = 0; i < n; i++) order[i] = (uint32_t)i;
  const Less less = {keys, koff};
  std::vector<uint64_t> cut(threads + 1);
  for (int t = 0; t <= threads; t++) cut[t] = n * t / threads;
  {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
      pool.emplace_back([&, t] { std::sort(order + cut[t], order + cut[t + 1], less); });
    for (std::thread& th : pool) th.join();
  }
  for (int width = 1; width < threads; width *= 2) {
    std::vector<std::thread> pool;
    for (int t = 0; t + width < threads; t += 2 * width) {
      const int hi = t + 2 * width < threads ? t + 2 * width : threads;
      pool.emplace_back([&, t, hi, width] {
        std::inplace_merge(order + cut[t], order + cut[t + width], order + cut[hi], less);
      });
    }
    for (std::thread& th : pool) th.join();
  }
  return 0;
}

}  // extern "C"
