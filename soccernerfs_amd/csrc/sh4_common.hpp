// Real spherical harmonics of degree 4 (16 values): soccernerfs_amd/sh.py's expressions in its order, with contraction off, so a coefficient is
// the bit pattern the torch expression gives.  Shared by the NeRFPlayer head input (nerfplayer.hip) and the view-dependent K-Planes colour input
// (color_vd.hip, field_fused.hip, mlp_rows.hip).
#pragma once

namespace snerf {

__device__ __forceinline__ float sh4_coeff(int k, float x, float y, float z) {
#pragma clang fp contract(off)
  const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
  switch (k) {
    case 0: return 0.28209479177387814f;
    case 1: return -0.48860251190291987f * y;
    case 2: return 0.48860251190291987f * z;
    case 3: return -0.48860251190291987f * x;
    case 4: return 1.0925484305920792f * xy;
    case 5: return -1.0925484305920792f * yz;
    case 6: return 0.94617469575755997f * z2 - 0.31539156525251999f;
    case 7: return -1.0925484305920792f * xz;
    case 8: return 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    case 9: return (0.59004358992664352f * y) * (-3.0f * x2 + y2);
    case 10: return (2.8906114426405538f * xy) * z;
    case 11: return (0.45704579946446572f * y) * (1.0f - 5.0f * z2);
    case 12: return (0.3731763325901154f * z) * (5.0f * z2 - 3.0f);
    case 13: return (0.45704579946446572f * x) * (1.0f - 5.0f * z2);
    case 14: return (1.4453057213202769f * z) * (x2 - y2);
    default: return (0.59004358992664352f * x) * (-x2 + 3.0f * y2);
  }
}

// K-Planes' direction input of the SH encoder: get_normalized_directions = (d + 1) / 2 (NS/fields/base_field.py:131-137), which tcnn maps
// back with 2x - 1 (soccernerfs_amd/tcnn_compat.py Encoding): two roundings, evaluated as the torch expressions are
__device__ __forceinline__ float sh4_kplanes_input(float d) {
#pragma clang fp contract(off)
  const float u = (d + 1.0f) / 2.0f;
  return u * 2.0f - 1.0f;
}

}  // namespace snerf
