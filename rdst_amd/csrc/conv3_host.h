// Host pieces that the register-stationary 3x3 files share (conv3_kernel.h, conv3_wgrad.hip, conv3x_wgrad.hip): the strip plan, the
// backward shape table and the guards around it.
#pragma once
#include "conv.h"

// A workgroup owns vertical strips, 32 pixels wide and SH rows high.  SH starts at 16 and halves, down to sh_floor, while the image
// batch gives fewer than `want` strips; `npg` workgroups (<= want) walk the `nstrips` strips.  false: 2^31 strips or more.
struct Conv3Strips { int SH, nys, nstrips, npg; };
inline bool conv3_strip_plan(int B, int H, int W, int sh_floor, int want, Conv3Strips& sp) {
  auto count = [&](int sh) { return (int64_t)B * ((H + sh - 1) / sh) * (W / 32); };
  int SH = 16;
  while (count(SH) < want && SH > sh_floor) SH /= 2;
  const int64_t ns = count(SH);
  if (ns >= (1ll << 31)) return false;
  sp.SH = SH;
  sp.nys = (H + SH - 1) / SH;
  sp.nstrips = (int)ns;
  sp.npg = ns < want ? (int)ns : want;
  return true;
}

// dgrad / wgrad: 1 = 150 -> 60, 2 = 60 -> 60, 3 = 60 -> 240 + PixelShuffle(2), 0 = not covered
inline int conv3_bwd_shape(int Cin, int Cout, int r) {
  if (Cin == 150 && Cout == 60 && r == 1) return 1;
  if (Cin == 60 && Cout == 60 && r == 1) return 2;
  if (Cin == 60 && Cout == 240 && r == 2) return 3;
  return 0;
}
// ... on a geometry the kernels take at all, with 16-byte aligned scratch (the packed weights / the wgrad slab)
inline bool conv3_bwd_geom_ok(const ConvGeom& g, int in_act, const void* scratch) {
  return scratch && g.ks == 3 && g.pad == 1 && !in_act && g.W % 32 == 0 && ((uintptr_t)scratch & 15) == 0;
}

// rows the kernels read and write as 4-byte words: bf16 rows hold channel pairs
inline bool conv3_rows_ok(const bf16* ptr, int64_t ld) { return ((uintptr_t)ptr & 3) == 0 && (ld & 1) == 0; }
inline bool conv3_rows_ok(const float* ptr, int64_t) { return ((uintptr_t)ptr & 3) == 0; }
