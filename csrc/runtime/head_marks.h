// Detect-head cell marks: which tiles of a level's first head conv anything reads.  Plain C++ (no HIP), shared by
// the kernels (as __host__ __device__ code), the executor, the bindings and the tests.
//
// The gated box conv of a level (head_gate.h) continues on a tile only when one of the tile's class logits reaches
// gate_min, and it reads its input, the box half of the level's first head conv F, on that tile grown by its 3x3
// halo.  The box half of F is therefore read only around the tiles that continue.  The executor runs F as two
// channel windows: the class window everywhere, before the class conv; the box window after it, on the tiles that
// some continuing box tile reads.
//
// A mark is one int per kMarkCell x kMarkCell-pixel cell and image ([image][cell row][cell column], the cell grid
// being ceil(H / 8) x ceil(W / 8)): 1 iff one of the class logits of an in-map pixel of the cell is >= gate_min
// (NaN compares false: the predicate of ConvParams.gate).  head_mark.hip writes them, head_marks_needed() is the one
// definition of what they imply; conv_x3hp_kernel evaluates the same function.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define ARENA_MARKS_HD __host__ __device__
#else
#define ARENA_MARKS_HD
#endif

namespace arena {

constexpr int kMarkCell = 8;
constexpr int kMarkMaxLevels = 3;

ARENA_MARKS_HD inline int head_mark_cells(int extent) { return (extent + kMarkCell - 1) / kMarkCell; }

// Consumer tile (uy, ux) of uh x uw pixels on an H x W map continues iff a cell that intersects it inside the map is
// marked.  m: the image's marks.
ARENA_MARKS_HD inline bool head_marks_continues(const int* m, int H, int W, int uy, int ux, int uh, int uw) {
  const int y0 = uy * uh, x0 = ux * uw;
  const int y1 = (y0 + uh < H ? y0 + uh : H) - 1, x1 = (x0 + uw < W ? x0 + uw : W) - 1;  // last in-map pixel
  const int ncx = head_mark_cells(W);
  for (int cy = y0 / kMarkCell; cy <= y1 / kMarkCell; ++cy)
    for (int cx = x0 / kMarkCell; cx <= x1 / kMarkCell; ++cx)
      if (m[cy * ncx + cx] != 0) return true;
  return false;
}

// Producer tile (ty, tx) of th x tw pixels is needed iff some continuing consumer tile, grown by `halo` pixels and
// clipped to the map, intersects it.  Consumer tile u covers [u * uh, (u + 1) * uh) clipped to the map; grown, it
// meets the producer rows [t0, t1) iff (u + 1) * uh + halo > t0 and u * uh - halo < t1.  All sizes > 0, halo >= 0,
// the tile inside the map (ty * th < H, tx * tw < W).
ARENA_MARKS_HD inline bool head_marks_needed(const int* m, int H, int W, int ty, int tx, int th, int tw, int uh,
                                             int uw, int halo) {
  const int ty0 = ty * th, tx0 = tx * tw;
  const int ty1 = ty0 + th < H ? ty0 + th : H, tx1 = tx0 + tw < W ? tx0 + tw : W;
  const int nuy = (H + uh - 1) / uh, nux = (W + uw - 1) / uw;
  const int uy_lo = ty0 > halo ? (ty0 - halo) / uh : 0, ux_lo = tx0 > halo ? (tx0 - halo) / uw : 0;
  int uy_hi = (ty1 + halo - 1) / uh, ux_hi = (tx1 + halo - 1) / uw;
  if (uy_hi > nuy - 1) uy_hi = nuy - 1;
  if (ux_hi > nux - 1) ux_hi = nux - 1;
  for (int uy = uy_lo; uy <= uy_hi; ++uy)
    for (int ux = ux_lo; ux <= ux_hi; ++ux)
      if (head_marks_continues(m, H, W, uy, ux, uh, uw)) return true;
  return false;
}

}  // namespace arena
