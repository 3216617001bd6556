// The fused K-Planes field forward on contracted coordinates (field_fused_contract.hip) for THREE planes per scale: field_fwd_kernel with
// NP = 3 and CT = 1.  A translation unit of its own for build time.
#include "field_fused_common.hpp"

namespace snerf {

template <typename T, int NS, int KEEP, bool VD>
static int launch_contract_static_k(const FieldArgs& a, hipStream_t st) {
  const int64_t n_tiles = (a.N + FF_TS - 1) / FF_TS;
  auto k = field_fwd_kernel<T, NS, KEEP, VD, 3, 1>;
  SNERF_ALLOW_LDS(k, LDS_LIMIT);
  hipLaunchKernelGGL(k, dim3((unsigned)field_fwd_grid<NS>(n_tiles)), dim3(FF_NW * 64), PlanFF<NS>::BYTES, st, a, n_tiles);
  SNERF_LAUNCH_CHECK("kplanes_field_fwd");
  return 0;
}
template <typename T, int NS, bool VD>
static int launch_contract_static_vd(const FieldArgs& a, hipStream_t st) {
  if (a.feat16 && a.feat32) return launch_contract_static_k<T, NS, 2, VD>(a, st);
  if (a.feat16) return launch_contract_static_k<T, NS, 1, VD>(a, st);
  return launch_contract_static_k<T, NS, 0, VD>(a, st);
}
template <typename T, int NS>
static int launch_contract_static(const FieldArgs& a, hipStream_t st, bool vd) {
  return vd ? launch_contract_static_vd<T, NS, true>(a, st) : launch_contract_static_vd<T, NS, false>(a, st);
}

int launch_field_fwd_contract_static(const FieldArgs& a, int operands, hipStream_t st, bool vd) {
  FF_DISPATCH_FWD(launch_contract_static, operands, a.d.n_scales, a, st, vd);
}

}  // namespace snerf
