// Pieces shared by the temporal-grid kernels (tgrid.hip: per-sample and run-length kernels; tgrid_tiles.hip: the tiled, owner-computes backward):
// the closed form of the temporal channel table, the per-level geometry of NS/field_components/cuda/csrc/temporal_gridencoder.cu:146-176, the
// sample position of snerf_coords and the cell it falls into.  Every kernel of both files goes through these, so they land in the same cell for the same
// sample by construction.  Everything here -- and, from this include on, in the including file -- is evaluated exactly as written (no contraction).
#pragma once
#include "table_level.hpp"

#pragma clang fp contract(off)

namespace snerf {

// (column, weight) of slot (ch, ab) at a time row; closed form of the reference's sampling_index table + get_temporal_index
__device__ __forceinline__ void tg_slot_from_time(float t, int C, int n_rows, int ch, int ab, int& col, float& w) {
  const float v = t * (float)(n_rows - 1);
  int r = (int)v;  // floor for t >= 0
  if (t == 1.f) r = n_rows - 1;
  auto occ = [&](int q) { return r > q ? C + q + C * ((r - 1 - q) / C) : q; };
  const int p = r % C;
  if (ch == p) {
    if (ab == 0) { col = occ(p); w = (float)(r + 1) - v; }
    else { col = C + r; w = v - (float)r; }
  } else {
    col = occ(ch);
    w = ab == 0 ? 1.f : 0.f;
  }
}

using TgLevel = TableLevel;  // table_level.hpp: shared with the static hash grid

// Level `level` of a table indexed along D <= 3 axes (the tiled backward and the run-length walk: always 3).  The only place that derives a temporal-grid
// level's rows, scale, dense-or-hashed decision and multipliers.
__device__ __forceinline__ TgLevel tg_level(const snerf_tgrid_desc& d, int level, int D) {
  TgLevel lv;
  lv.off0 = (uint32_t)d.offsets[level];
  lv.rows = (uint32_t)(d.offsets[level + 1] - d.offsets[level]);
  lv.scale = exp2f((float)level * d.S) * (float)d.H - 1.0f;  // .cu:146-148
  const uint32_t resolution = (uint32_t)ceilf(lv.scale) + 1;
  const uint32_t primes[3] = {1u, 2654435761u, 805459861u};
  uint32_t stride = 1;
  for (int k = 0; k < D && stride <= lv.rows; ++k) stride *= d.align_corners ? resolution : (resolution + 1);
  lv.hashed = d.gridtype == 0 && stride > lv.rows;
  uint32_t st = 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // constant subscripts (D may be a run-time value): the level stays in registers
    lv.mult[k] = 0u;
    if (k >= D) continue;
    lv.mult[k] = lv.hashed ? primes[k] : (st <= lv.rows ? st : 0u);  // dense: axes beyond the overflowing stride do not contribute (.cu:70-74)
    if (st <= lv.rows) st *= d.align_corners ? resolution : (resolution + 1);
  }
  lv.pow2 = (lv.rows & (lv.rows - 1u)) == 0u;
  return lv;
}

// One axis of the midpoint of the ray bin whose two edges sum to `edge_sum`, as a fraction of the box [lo, lo + extent] (snerf_coords mode 1).  The one
// ray-midpoint expression of the table encoders: the run-length walk calls it with the ray in registers, everything else through tg_ray_sample_x.
__device__ __forceinline__ float tg_ray_x(float origin, float dir, float edge_sum, float lo, float extent) {
  const float pos = origin + (dir * edge_sum) / 2.f;
  return (pos - lo) / extent;
}
// sample s of ray r
__device__ __forceinline__ void tg_ray_sample_x(const snerf_coords& c, int64_t r, int s, float x[3]) {
  const float* eb = c.ebins + r * (c.S + 1) + s;
  const float mid = eb[0] + eb[1];
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = tg_ray_x(c.origins[r * 3 + k], c.dirs[r * 3 + k], mid, c.aabb_min[k], c.aabb_max[k] - c.aabb_min[k]);
}

// .cu:119-124: a sample outside [0,1]^D reads nothing and receives no gradient
__device__ __forceinline__ bool tg_out_of_range(const float x[3], int D) {
  bool oob = false;
  for (int k = 0; k < D; ++k) oob |= (x[k] < 0.f) || (x[k] > 1.f);
  return oob;
}

// Sample b of a D = 3 batch in [0,1]^3 (snerf_coords mode 0: explicit points [B,3]; mode 1: the midpoint of bin b % S of ray b / S); returns "out of range".
// For B < 2^31: a 32-bit division (the 64-bit one is a ~100-instruction routine); tgrid_kernel, whose B is not bounded, divides in 64 bits itself.
__device__ __forceinline__ bool tg_sample_x(const snerf_coords& c, int64_t b, float x[3]) {
  if (c.mode == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = c.pts[b * 3 + k];
  } else {
    const uint32_t r = (uint32_t)b / (uint32_t)c.S;
    tg_ray_sample_x(c, (int64_t)r, (int)((uint32_t)b - r * (uint32_t)c.S), x);
  }
  return tg_out_of_range(x, 3);
}

// cell and in-cell position of x at a level, along D axes
__device__ __forceinline__ void tg_cell(const TgLevel& lv, bool align_corners, const float x[3], int D, uint32_t pg[3], float frac[3]) {
  for (int k = 0; k < D; ++k) {
    const float pos = x[k] * lv.scale + (align_corners ? 0.0f : 0.5f);
    const float f = floorf(pos);
    pg[k] = (uint32_t)f;
    frac[k] = pos - f;
  }
}

// ---- one sample's forward at one level, for the kernels that keep a cell's eight corner values in registers (D = 3: tgrid.hip's run-length
// forward, tgrid_density.hip) ----
// table element of corner idx (bit d: the far side of axis d) of `cell`, at `column` of its row
__device__ __forceinline__ size_t tg_corner_entry(const TgLevel& lv, int grid_C, const uint32_t cell[3], int idx, int column) {
  const uint32_t row = lv.row_of(cell[0] + (uint32_t)(idx & 1), cell[1] + (uint32_t)((idx >> 1) & 1), cell[2] + (uint32_t)(idx >> 2));
  return ((size_t)lv.off0 + row) * (size_t)grid_C + (size_t)column;
}
// One (channel, column) slot's share of a sample's feature: the eight corner values times the slot's temporal weight, interpolated at in-cell position
// fr -- tgrid_kernel<false>'s products and its order of the eight additions.  The feature is this plus the same of the channel's other column.
__device__ __forceinline__ float tg_cell_interp(const float val[8], const float fr[3], float wt) {
  float acc = 0.f;
#pragma unroll
  for (int idx = 0; idx < 8; ++idx) {
    const float v = val[idx] * wt;  // the temporal weight is applied per sample (explicit points: every sample has its own time), as tgrid_kernel does
    acc += table_corner_weight(fr, 3, idx) * v;
  }
  return acc;
}

}  // namespace snerf
