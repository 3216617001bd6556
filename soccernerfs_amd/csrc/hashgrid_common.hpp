// Pieces shared by the static hash grid's kernels (hashgrid.hip: gather and atomic scatter; hashgrid_tiles.hip: the tiled, owner-computes backward): the
// level geometry of tcnn's grid_index and the cell of pos_fract (Mueller et al. 2022, grid.h), so that both files land in the same cell and row for the
// same point by construction.  No file-scope contraction setting: hashgrid.hip lets its interpolation sums contract, hashgrid_tiles.hip does not; the cell
// below has one explicit fmaf and nothing else that could fuse.
#pragma once
#include "table_level.hpp"

namespace snerf {

// Level `level` of a table indexed along D <= 3 axes (the tiled backward: always 3).  Scale, resolution and rows come from the descriptor
// (snerf_hashgrid_layout computed them once on the host); the only place that derives the dense-or-hashed decision and the multipliers from them.
__device__ __forceinline__ TableLevel ht_level(const snerf_hashgrid_desc& d, int level, int D) {
  TableLevel lv;
  lv.off0 = (uint32_t)d.offsets[level];
  lv.rows = (uint32_t)(d.offsets[level + 1] - d.offsets[level]);
  lv.scale = d.scale[level];
  const uint32_t resolution = (uint32_t)d.resolution[level];
  const uint32_t primes[3] = {1u, 2654435761u, 805459861u};
  uint64_t stride = 1;
  for (int k = 0; k < D && stride <= lv.rows; ++k) stride *= resolution;
  lv.hashed = lv.rows < stride;
  // dense stride of axis k: the product of the resolutions before it while that product is <= rows (64-bit in grid.h; kept here as a 32-bit value and
  // a flag, which is the same thing: a product that fits is < 2^32, and one that does not is never multiplied or used again)
  uint32_t st = 1;
  bool fits = 1u <= lv.rows;
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // constant subscripts (D may be a run-time value): the level stays in registers
    lv.mult[k] = 0u;
    if (k >= D) continue;
    lv.mult[k] = lv.hashed ? primes[k] : (fits ? st : 0u);
    if (fits) {
      const uint64_t next = (uint64_t)st * resolution;
      st = (uint32_t)next;
      fits = (next >> 32) == 0 && st <= lv.rows;
    }
  }
  lv.pow2 = (lv.rows & (lv.rows - 1u)) == 0u;
  return lv;
}

// cell and in-cell position of x at a level, along D axes (no bounds check on coordinates, as tcnn)
__device__ __forceinline__ void ht_cell(const TableLevel& lv, const float* x, int D, uint32_t pg[3], float fr[3]) {
#pragma clang fp contract(off)
  for (int k = 0; k < D; ++k) {
    const float p = fmaf(lv.scale, x[k], 0.5f);  // pos_fract
    const float f = floorf(p);
    pg[k] = (uint32_t)(int)f;
    fr[k] = p - f;
  }
}

}  // namespace snerf
