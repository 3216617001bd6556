// The fused K-Planes field forward (field_fused.hip) on CONTRACTED coordinates: snerf_coords.contract = 1, the L-inf scene contraction of an
// unbounded scene evaluated where the tile derives a sample's coordinate from its ray (kplanes_common.hpp: load_coords_ray).
// The kernels are field_fused_common.hpp's with CT = 1, six planes per scale here (the unordered walk and the walk in frame-time order); the
// three-plane form is field_fused_contract_static.hip.  Translation units of their own: with the switch as a run-time branch several bounded
// instantiations, which sit at the 128-VGPR limit, gained spilled registers, so the bounded kernels are compiled from the text they were.
#include "field_fused_common.hpp"

namespace snerf {

template <typename T, int NS, int KEEP, bool VD>
static int launch_contract_k(const FieldArgs& a, const int32_t* ray_order, hipStream_t st) {
  const int64_t n_tiles = (a.N + FF_TS - 1) / FF_TS;
  int64_t grid = field_fwd_grid<NS>(n_tiles);
  if (ray_order) {
    auto k = field_fwd_ordered_kernel<T, NS, KEEP, VD, 1>;
    SNERF_ALLOW_LDS(k, LDS_LIMIT);
    if (grid >= 8) grid &= ~(int64_t)7;  // whole eights, as field_fused.hip
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FF_NW * 64), PlanFF<NS>::BYTES, st, a, (uint32_t)n_tiles, ray_order, (uint32_t)(a.c.S / FF_TS));
  } else {
    auto k = field_fwd_kernel<T, NS, KEEP, VD, 6, 1>;
    SNERF_ALLOW_LDS(k, LDS_LIMIT);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FF_NW * 64), PlanFF<NS>::BYTES, st, a, n_tiles);
  }
  SNERF_LAUNCH_CHECK("kplanes_field_fwd");
  return 0;
}
template <typename T, int NS, bool VD>
static int launch_contract_vd(const FieldArgs& a, const int32_t* ray_order, hipStream_t st) {
  if (a.feat16 && a.feat32) return launch_contract_k<T, NS, 2, VD>(a, ray_order, st);
  if (a.feat16) return launch_contract_k<T, NS, 1, VD>(a, ray_order, st);
  return launch_contract_k<T, NS, 0, VD>(a, ray_order, st);
}
template <typename T, int NS>
static int launch_contract(const FieldArgs& a, const int32_t* ray_order, hipStream_t st, bool vd) {
  return vd ? launch_contract_vd<T, NS, true>(a, ray_order, st) : launch_contract_vd<T, NS, false>(a, ray_order, st);
}

int launch_field_fwd_contract_static(const FieldArgs& a, int operands, hipStream_t st, bool vd);

int launch_field_fwd_contract(const FieldArgs& a, int operands, const int32_t* ray_order, hipStream_t st, bool vd) {
  if (a.d.n_coords == 3) return launch_field_fwd_contract_static(a, operands, st, vd);  // a ray order was refused for it by the caller
  FF_DISPATCH_FWD(launch_contract, operands, a.d.n_scales, a, ray_order, st, vd);
}

}  // namespace snerf
