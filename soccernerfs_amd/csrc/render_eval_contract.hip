// The render tail of render_eval.hip on contracted coordinates (snerf_coords.contract = 1; an unbounded scene): field_render_kernel with
// CT = 1, six or three planes per scale.  A translation unit of its own, so that the bounded instantiations of render_eval.hip and
// render_eval_static.hip are compiled from the text they were (field_fused_contract.hip says why).
#include "render_eval_common.hpp"

namespace snerf {

template <typename T, int NS, bool VD, int NP>
static int launch_render_contract_k(const FieldArgs& a, int R, const RayOut& o, hipStream_t st) {
  auto k = field_render_kernel<T, NS, VD, NP, 1>;
  SNERF_ALLOW_LDS(k, LDS_LIMIT);
  hipLaunchKernelGGL(k, dim3((unsigned)field_render_grid<NS>(R)), dim3(FF_NW * 64), PlanFF<NS>::BYTES + RAY_LDS_B, st, a, R, o);
  SNERF_LAUNCH_CHECK("kplanes_field_render");
  return 0;
}
template <typename T, int NS>
static int launch_render_contract(const FieldArgs& a, int R, const RayOut& o, hipStream_t st, bool vd) {
  if (a.d.n_coords == 3)
    return vd ? launch_render_contract_k<T, NS, true, 3>(a, R, o, st) : launch_render_contract_k<T, NS, false, 3>(a, R, o, st);
  return vd ? launch_render_contract_k<T, NS, true, 6>(a, R, o, st) : launch_render_contract_k<T, NS, false, 6>(a, R, o, st);
}

int launch_field_render_contract(const FieldArgs& a, int R, const RayOut& o, int operands, hipStream_t st, bool vd) {
  FF_DISPATCH_FWD(launch_render_contract, operands, a.d.n_scales, a, R, o, st, vd);
}

}  // namespace snerf
