// The packed-buffer layout of lsbm_amd/csrc/host_staging.h (Packed, Field),
// built with -fsanitize=address,undefined: host code only, no HIP headers.
#include <stdio.h>

#include <vector>

#define LSBM_STAGING_LAYOUT_ONLY
#include "../../lsbm_amd/csrc/host_staging.h"

static int fails = 0;
#define EXPECT(c)                                          \
  do {                                                     \
    if (!(c)) {                                            \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);   \
      fails++;                                             \
    }                                                      \
  } while (0)

template <class A, class B>
constexpr bool same = false;
template <class A>
constexpr bool same<A, A> = true;

int main() {
  // widest first, back to back: u64[3] u32[2] u8[5]
  lsbm::Packed p;
  const auto a = p.add<uint64_t>(3);
  const auto b = p.add<uint32_t>(2);
  const auto c = p.add<uint8_t>(5);
  EXPECT(a.offset == 0 && a.count == 3 && a.bytes() == 24);
  EXPECT(b.offset == 24 && b.count == 2 && b.bytes() == 8);
  EXPECT(c.offset == 32 && c.count == 5 && c.bytes() == 5);
  EXPECT(p.bytes() == 37);

  // an empty field takes no room: the next one starts where it does
  lsbm::Packed q;
  const auto q0 = q.add<uint64_t>(2);
  const auto empty = q.add<uint64_t>(0);
  const auto q1 = q.add<uint32_t>(1);
  EXPECT(q0.offset == 0 && empty.offset == 16 && empty.bytes() == 0 && q1.offset == 16);
  EXPECT(q.bytes() == 20);
  EXPECT(lsbm::Packed().bytes() == 0);

  // in(base) is base + offset with the field's type, for a mutable and a const base
  std::vector<uint64_t> store(5, 0);  // (8-byte aligned, 40 bytes >= 37)
  uint8_t* base = reinterpret_cast<uint8_t*>(store.data());
  const uint8_t* cbase = base;
  static_assert(same<decltype(a.in(base)), uint64_t*> && same<decltype(a.in(cbase)), const uint64_t*>, "u64");
  static_assert(same<decltype(b.in(base)), uint32_t*> && same<decltype(b.in(cbase)), const uint32_t*>, "u32");
  static_assert(same<decltype(c.in(base)), uint8_t*> && same<decltype(c.in(cbase)), const uint8_t*>, "u8");
  EXPECT(reinterpret_cast<uint8_t*>(a.in(base)) == base);
  EXPECT(reinterpret_cast<uint8_t*>(b.in(base)) == base + 24);
  EXPECT(c.in(base) == base + 32 && c.in(cbase) == cbase + 32);
  EXPECT(reinterpret_cast<const uint8_t*>(b.in(cbase)) == cbase + 24);
  EXPECT(b.in(static_cast<void*>(nullptr)) == nullptr);  // a failed scratch request stays null

  // what is written through one side's pointers is read through the other's
  for (size_t i = 0; i < a.count; i++) a.in(base)[i] = 0x0101010101010101ull * (i + 1);
  for (size_t i = 0; i < b.count; i++) b.in(base)[i] = 0xb0b0b0b0u + (uint32_t)i;
  for (size_t i = 0; i < c.count; i++) c.in(base)[i] = (uint8_t)(0xc0 + i);
  EXPECT(a.in(cbase)[2] == 0x0303030303030303ull && b.in(cbase)[1] == 0xb0b0b0b1u && c.in(cbase)[4] == 0xc4);
  EXPECT(cbase[23] == 0x03 && cbase[24] == 0xb0 && cbase[32] == 0xc0 && cbase[36] == 0xc4);

  if (fails) {
    printf("FAILED %d\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
