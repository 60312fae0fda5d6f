// THE way to lay out device scratch: a region is declared once, with its element type and count, and the pointer, the
// offset and the size all come from that one declaration.  Host only, no HIP include (tests/arena_check.cpp builds it
// with the plain host compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace wh {
constexpr size_t kWsAlign = 256;

// `count` elements of T at byte `off` of some base (the context's workspace, a persistent slot, another context's arena).
template <class T>
struct Region {
  size_t off = 0, count = 0;
  T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
  const T* at(const void* base) const { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }
  size_t bytes() const { return count * sizeof(T); }  // unrounded
};

// Hands out consecutive regions: every start is kWsAlign-aligned (given an aligned start), every region advances the
// offset by its size rounded up to kWsAlign.  A negative count or a size beyond size_t makes the carve !ok() (and takes
// nothing); wh::ws_reserve(ctx, carve) refuses such a layout.
class Carve {
 public:
  explicit Carve(size_t start = 0) : off_(start) {}
  template <class T>
  Region<T> take(int64_t count) {
    Region<T> r;
    r.off = off_;
    if (count < 0 || (uint64_t)count > (SIZE_MAX - (kWsAlign - 1) - off_) / sizeof(T)) {
      ok_ = false;
      return r;
    }
    r.count = (size_t)count;
    off_ += (r.bytes() + (kWsAlign - 1)) & ~(kWsAlign - 1);
    return r;
  }
  // not wanted: a zero-length region at the current offset (a valid pointer that nothing dereferences)
  template <class T>
  Region<T> take_if(bool wanted, int64_t count) {
    return take<T>(wanted ? count : 0);
  }
  size_t end() const { return off_; }
  bool ok() const { return ok_; }

 private:
  size_t off_;
  bool ok_ = true;
};
}  // namespace wh
