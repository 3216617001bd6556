// One level of a D = 3 multi-level table (temporal hash grid: tgrid_common.hpp fills it; static hash grid: hashgrid_tiles.hip): the one definition of
// "which table row does this corner live in" that the scatter kernels and the tiled backwards share.
#pragma once
#include "common.hpp"

namespace snerf {

// Table rows [off0, off0 + rows), position scale, and the per-axis multipliers whose XOR (hashed level) or sum (dense level) over the corner's integer
// coordinates, reduced modulo `rows`, is get_grid_index (temporal_gridencoder.cu:62-88; tcnn's grid_index is the same construction).
struct TableLevel {
  uint32_t off0, rows, mult[3];
  float scale;
  bool hashed, pow2;
  __device__ __forceinline__ uint32_t row_of(uint32_t cx, uint32_t cy, uint32_t cz) const {
    const uint32_t a = cx * mult[0], b = cy * mult[1], c = cz * mult[2];
    const uint32_t index = hashed ? (a ^ b ^ c) : (a + b + c);
    return pow2 ? (index & (rows - 1u)) : (index % rows);
  }
};

}  // namespace snerf
