// The render tail of render_eval.hip for THREE planes per scale (a static scene, or PlaneSet.space_desc() of frozen time planes): the same walk
// over a ray's tiles and the same per-ray compositing (render_eval_common.hpp) with the tile gathered from XY, XZ, YZ alone; coords.times is
// never read.  A translation unit of its own, so that the six-plane instantiations of render_eval.hip are compiled from the text they were.
#include "render_eval_common.hpp"

namespace snerf {

template <typename T, int NS, bool VD>
static int launch_render_static_vd(const FieldArgs& a, int R, const RayOut& o, hipStream_t st) {
  auto k = field_render_kernel<T, NS, VD, 3>;
  SNERF_ALLOW_LDS(k, LDS_LIMIT);
  hipLaunchKernelGGL(k, dim3((unsigned)field_render_grid<NS>(R)), dim3(FF_NW * 64), PlanFF<NS>::BYTES + RAY_LDS_B, st, a, R, o);
  SNERF_LAUNCH_CHECK("kplanes_field_render");
  return 0;
}
template <typename T, int NS>
static int launch_render_static(const FieldArgs& a, int R, const RayOut& o, hipStream_t st, bool vd) {
  return vd ? launch_render_static_vd<T, NS, true>(a, R, o, st) : launch_render_static_vd<T, NS, false>(a, R, o, st);
}

int launch_field_render_static(const FieldArgs& a, int R, const RayOut& o, int operands, hipStream_t st, bool vd) {
  FF_DISPATCH_FWD(launch_render_static, operands, a.d.n_scales, a, R, o, st, vd);
}

}  // namespace snerf
