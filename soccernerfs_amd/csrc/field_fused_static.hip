// The fused K-Planes field forward (field_fused.hip) for THREE planes per scale: a static scene (len(spacetime_resolution) == 3,
// NS/fields/kplanes_field.py:59-61) or the space planes of a 4-coordinate set whose time planes are frozen (:95-99; PlaneSet.space_desc()).
// The kernel and its tile are field_fused_common.hpp's with NP = 3: XY, XZ, YZ gathered and multiplied in that order, no time tap, coords.times never read --
// bit-identical to snerf_kplanes_gather_fwd on the same descriptor + the two snerf_mlp_fwd (tests/test_gpu_static_planes.py).  A translation
// unit of its own, so that the six-plane instantiations of field_fused.hip are compiled from the text they were.  The walk in frame-time
// order (field_fwd_ordered_kernel) is not built here: it exists for the time planes' rows.
#include "field_fused_common.hpp"

namespace snerf {

template <typename T, int NS, int KEEP, bool VD>
static int launch_static_k(const FieldArgs& a, hipStream_t st) {
  const int64_t n_tiles = (a.N + FF_TS - 1) / FF_TS;
  auto k = field_fwd_kernel<T, NS, KEEP, VD, 3>;
  SNERF_ALLOW_LDS(k, LDS_LIMIT);
  hipLaunchKernelGGL(k, dim3((unsigned)field_fwd_grid<NS>(n_tiles)), dim3(FF_NW * 64), PlanFF<NS>::BYTES, st, a, n_tiles);
  SNERF_LAUNCH_CHECK("kplanes_field_fwd");
  return 0;
}
template <typename T, int NS, bool VD>
static int launch_static_vd(const FieldArgs& a, hipStream_t st) {
  if (a.feat16 && a.feat32) return launch_static_k<T, NS, 2, VD>(a, st);
  if (a.feat16) return launch_static_k<T, NS, 1, VD>(a, st);
  return launch_static_k<T, NS, 0, VD>(a, st);
}
template <typename T, int NS>
static int launch_static(const FieldArgs& a, hipStream_t st, bool vd) {
  return vd ? launch_static_vd<T, NS, true>(a, st) : launch_static_vd<T, NS, false>(a, st);
}

int launch_field_fwd_static(const FieldArgs& a, int operands, hipStream_t st, bool vd) { FF_DISPATCH_FWD(launch_static, operands, a.d.n_scales, a, st, vd); }

}  // namespace snerf
