// How a backward entry point divides its one opaque workspace.  A layout function (lin_bwd_layout in linear.h, conv_bwd_layout in
// conv.h, mlp_bwd_layout in mlp_mfma.hip, wattn_bwd_layout in wattn.h) walks a WsCarver over the base pointer and returns a struct
// of regions plus the total; the size query calls it with a null base and returns the total, the launcher calls it with the
// caller's pointer, so size, carve and grid cap cannot disagree.  Plain host C++: nothing from HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Bump carver.  No alignment padding of its own: a region starts where the one before it ends.
struct WsCarver {
  char* base;   // null: measuring only
  size_t off = 0;
  explicit WsCarver(void* b) : base(static_cast<char*>(b)) {}
  template <typename T>
  T* take(size_t count) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return r;
  }
  size_t bytes() const { return off; }
};

// A region of per-workgroup slab rows: `rows` rows of `stride` floats.  A kernel never gets more than `rows` workgroups, and
// one whose rows are wider than the region's own stride gets as many as the same floats hold.
struct WsSlab {
  float* p = nullptr;
  int64_t rows = 0, stride = 0;
  int64_t rows_at(int64_t s) const { return s <= stride ? rows : s > 0 ? rows * stride / s : 0; }
  int64_t cap(int64_t want, int64_t s) const { return want < rows_at(s) ? want : rows_at(s); }   // a launcher's grid cap
  bool fits(int64_t grid, int64_t s) const { return grid >= 0 && grid <= rows_at(s); }            // may `grid` workgroups of stride s write here
  // the i-th of n equal column parts of every row: the same rows, stride / n wide, one part behind the other
  WsSlab part(int i, int n) const { return WsSlab{p ? p + i * rows * (stride / n) : nullptr, rows, stride / n}; }
};
static inline WsSlab ws_take_slab(WsCarver& c, int64_t rows, int64_t stride) {
  return WsSlab{c.take<float>((size_t)rows * (size_t)stride), rows, stride};
}
