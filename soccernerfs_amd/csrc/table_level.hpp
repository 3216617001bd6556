// One level of a multi-level table (temporal hash grid: tgrid_common.hpp fills it; static hash grid: hashgrid_common.hpp): the one definition of "which
// table row does this corner live in" and of a corner's interpolation weight that every table kernel shares -- per-sample gather / scatter, run-length walk
// and tiled backward alike.  No file-scope contraction setting here (hashgrid.hip contracts, the temporal grid's files do not): the functions with
// floating-point arithmetic carry their own.
#pragma once
#include "common.hpp"

namespace snerf {

// Table rows [off0, off0 + rows), position scale, and the per-axis multipliers whose XOR (hashed level) or sum (dense level) over the corner's integer
// coordinates, reduced modulo `rows`, is get_grid_index (temporal_gridencoder.cu:62-88; tcnn's grid_index is the same construction).  Filled by tg_level /
// ht_level for D <= 3 axes; mult[] of the axes beyond D is 0.
struct TableLevel {
  uint32_t off0, rows, mult[3];
  float scale;
  bool hashed, pow2;
  // one reduction modulo the table size -- a mask when the size is a power of two (every hashed level: 2^log2_hashmap_size)
  __device__ __forceinline__ uint32_t reduce(uint32_t index) const { return pow2 ? (index & (rows - 1u)) : (index % rows); }
  __device__ __forceinline__ uint32_t row_of(uint32_t cx, uint32_t cy, uint32_t cz) const {
    const uint32_t a = cx * mult[0], b = cy * mult[1], c = cz * mult[2];
    return reduce(hashed ? (a ^ b ^ c) : (a + b + c));
  }
  // The same row for the 2^D corners of ONE cell with the per-axis products shared between them (a third of the integer work; the per-sample kernels
  // visit all corners of a cell in one lane): term[d][bit] = (pg[d] + bit) * mult[d], and corner idx takes bit d of idx on axis d.
  __device__ __forceinline__ void corner_terms(const uint32_t pg[3], int D, uint32_t term[3][2]) const {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d >= D) continue;
      term[d][0] = pg[d] * mult[d];
      term[d][1] = (pg[d] + 1u) * mult[d];
    }
  }
  __device__ __forceinline__ uint32_t row_of_corner(const uint32_t term[3][2], int D, int idx) const {
    uint32_t index = 0;
    for (int d = 0; d < D; ++d) index = hashed ? (index ^ term[d][(idx >> d) & 1]) : (index + term[d][(idx >> d) & 1]);
    return reduce(index);
  }
};

// D-linear interpolation weight of corner idx (bit d of idx: the far side of axis d) at in-cell position fr; factors multiplied in axis order
__device__ __forceinline__ float table_corner_weight(const float fr[3], int D, int idx) {
#pragma clang fp contract(off)
  float w = 1.f;
  for (int d = 0; d < D; ++d) w *= ((idx >> d) & 1) ? fr[d] : 1.f - fr[d];
  return w;
}

}  // namespace snerf
