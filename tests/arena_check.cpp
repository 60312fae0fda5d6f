// Stand-alone check of csrc/wh_arena.h (tests/test_arena_host.py builds and runs it, under the host sanitizers where
// they link): wh::Carve lays regions out exactly as the hand-written `off += (bytes + 255) & ~255` columns it replaced.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "wh_arena.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

struct Rec64 {  // (a 64-byte record, like the pulse records of the time base)
  alignas(64) char b[64];
};
struct Rec24 {  // (a record whose size is no power of two, like the contour's sections)
  int32_t a[6];
};

struct Item {
  int elem;  // element size: 1, 4, 8, 16, 24 or 64
  int64_t count;
};
struct Taken {
  size_t off, count, bytes;
};

static Taken take(wh::Carve& c, const Item& it) {
  switch (it.elem) {
    case 1: { auto r = c.take<uint8_t>(it.count); return {r.off, r.count, r.bytes()}; }
    case 4: { auto r = c.take<int32_t>(it.count); return {r.off, r.count, r.bytes()}; }
    case 8: { auto r = c.take<double>(it.count); return {r.off, r.count, r.bytes()}; }
    case 16: { auto r = c.take<long double>(it.count); return {r.off, r.count, r.bytes()}; }
    case 24: { auto r = c.take<Rec24>(it.count); return {r.off, r.count, r.bytes()}; }
    default: { auto r = c.take<Rec64>(it.count); return {r.off, r.count, r.bytes()}; }
  }
}

// every offset and the end against the old formula, from `start`; regions ascending and disjoint
static void check_list(const std::vector<Item>& items, size_t start) {
  wh::Carve c(start);
  size_t off = start, prev_end = start;
  for (const Item& it : items) {
    const Taken t = take(c, it);
    const size_t bytes = (size_t)it.elem * (size_t)it.count;
    CHECK(t.off == off);
    CHECK(t.count == (size_t)it.count && t.bytes == bytes);
    CHECK(t.off % wh::kWsAlign == start % wh::kWsAlign);
    CHECK(t.off >= prev_end);
    prev_end = t.off + t.bytes;
    off += (bytes + 255) & ~(size_t)255;  // the formula every call site used to spell out
    CHECK(c.end() == off);
    CHECK(prev_end <= c.end());
  }
  CHECK(c.ok());
}

int main() {
  static_assert(sizeof(long double) == 16 && sizeof(Rec24) == 24 && sizeof(Rec64) == 64, "the element sizes of the lists");
  const std::vector<std::vector<Item>> lists = {
      {{8, 1}, {1, 1}, {4, 1}, {64, 1}},
      {{8, 0}, {8, 32}, {8, 33}, {1, 255}, {1, 256}, {1, 257}, {4, 0}, {4, 63}, {4, 64}, {4, 65}},
      {{8, 160001}, {1, 160001}, {8, 20000}, {8, 20000}, {8, 20000}, {8, 20000}, {4, 3}, {1, 3 * 157 * 256}, {4, 3 * 157},
       {8, 4}, {64, 60000}},                                                  // a time base's shape
      {{8, 4807}, {4, 2 * 411}, {24, 411}, {4, 24}, {8, 32 * 801 + 1024}},     // a contour share's shape
      {{16, 2049 * 7}, {16, 0}, {8, 2049 * 7}, {24, 0}, {64, 0}, {1, 0}, {4, 1}},
  };
  for (const auto& l : lists) {
    check_list(l, 0);
    check_list(l, 256);
    check_list(l, 7 * 256 + 4096);
  }

  {  // take_if(false, n) takes nothing and returns the current offset; take_if(true, n) is take(n)
    wh::Carve c;
    c.take<double>(5);
    const size_t at = c.end();
    const auto none = c.take_if<double>(false, 1000);
    CHECK(none.off == at && none.count == 0 && none.bytes() == 0 && c.end() == at && c.ok());
    const auto some = c.take_if<int32_t>(true, 1000);
    CHECK(some.off == at && some.count == 1000 && c.end() == at + 4096 && c.ok());
  }
  {  // a negative count
    wh::Carve c;
    c.take<double>(3);
    const auto r = c.take<int32_t>(-1);
    CHECK(!c.ok() && r.count == 0 && c.end() == 256);
    c.take<double>(1);
    CHECK(!c.ok());  // (it stays failed)
  }
  {  // a size beyond size_t
    wh::Carve c;
    const auto r = c.take<double>((int64_t)(SIZE_MAX / 4));
    CHECK(!c.ok() && r.count == 0 && c.end() == 0);
    wh::Carve c2(SIZE_MAX - 1023);  // (the rounding itself must not wrap either)
    c2.take<uint8_t>(1000);
    CHECK(!c2.ok());
  }

  // a real arena: the first and the last element of every region, written through at()
  for (const auto& l : lists) {
    wh::Carve c;
    std::vector<wh::Region<uint8_t>> bytes_of;  // every region again, as the bytes it spans
    std::vector<wh::Region<double>> doubles;
    std::vector<wh::Region<Rec64>> recs;
    for (const Item& it : l) {
      if (it.elem == 8) {
        doubles.push_back(c.take<double>(it.count));
        bytes_of.push_back({doubles.back().off, doubles.back().bytes()});
      } else if (it.elem == 64) {
        recs.push_back(c.take<Rec64>(it.count));
        bytes_of.push_back({recs.back().off, recs.back().bytes()});
      } else {
        const Taken t = take(c, it);
        bytes_of.push_back({t.off, t.bytes});
      }
    }
    CHECK(c.ok());
    void* base = nullptr;
    if (posix_memalign(&base, wh::kWsAlign, c.end() ? c.end() : wh::kWsAlign) != 0) return 2;  // (aligned like a device allocation)
    for (const auto& r : bytes_of) {
      if (!r.count) continue;
      r.at(base)[0] = 0x11;
      r.at(base)[r.count - 1] = 0x22;
    }
    for (const auto& r : doubles) {
      if (!r.count) continue;
      r.at(base)[0] = 1.5;
      r.at(base)[r.count - 1] = 2.5;
      CHECK(r.at((const void*)base)[r.count - 1] == 2.5);
    }
    for (const auto& r : recs) {
      if (!r.count) continue;
      memset(&r.at(base)[0], 1, sizeof(Rec64));
      memset(&r.at(base)[r.count - 1], 2, sizeof(Rec64));
    }
    free(base);
  }

  if (g_failed) {
    printf("%d checks failed\n", g_failed);
    return 1;
  }
  printf("arena_check: ok\n");
  return 0;
}
