// Rendering whole frames (eval / camera paths): ray generation for a pixel range of ONE camera without an index table, and the render tail
// of the K-Planes model -- plane gather -> sigma_net -> colour net -> get_weights -> RGB / accumulation / depth per ray -- as ONE kernel.
//
// Reference: what `ns-render` runs per chunk of --eval-num-rays-per-chunk rays (scripts/render.py:60-131 -> Model.get_outputs_for_camera_ray_bundle,
// NS/models/base_model.py:159-186): Cameras.generate_rays(camera_indices=k) (NS/cameras/cameras.py:300-418: a meshgrid of image coordinates, then
// _generate_rays_from_coords :505-741), the AABB collider, and for the nerf level KPlanesField.forward (NS/fields/kplanes_field.py:275-358),
// RaySamples.get_weights (NS/cameras/rays.py:127-149), RGBRenderer / AccumulationRenderer / DepthRenderer in eval mode
// (NS/model_components/renderers.py:58-140, :197-223, :226-287; background "last_sample", nan_to_num, clamp).
//
// field_render_kernel: the tile of field_fused_common.hpp (the same code field_fwd_kernel runs, so the same density / colour bits) with another
// work decomposition above it: a workgroup owns a WHOLE RAY and walks its 32-sample tiles front to back.  The ray's density [S], colour [S,3] and
// bin edges [S+1] stay in LDS (7.7 KB at the limit S = 320, beside the ~43 KB of the tile: two workgroups per CU as before); per-sample density
// and colour never reach HBM.  After the last tile wave 0 runs the per-ray phases of resample_kernel stage 1 (snerf_weights_fwd) and
// render_fwd_kernel (training = 0, bg_mode = 1) on the LDS-resident values -- the same functions of per_ray_common.hpp -- so the outputs equal
// the three-kernel chain bit for bit, as ray_train_kernel's equal the training step's five.  The kernel is defined in render_eval_common.hpp,
// a template over the plane count: render_eval_static.hip builds the three-plane form.
//
// Early ray termination (transmittance_cutoff > 0): after a tile every wave forms the ray's remaining transmittance T = exp(-sum sigma delta) over
// the samples evaluated so far (the same LDS values, the same arithmetic: the decision is workgroup-uniform without a broadcast).  If T < cutoff
// the ray's remaining tiles are not gathered or decoded; their samples count as zero density, and the background is the last evaluated sample's
// colour.  The weights that are dropped sum to less than T: |rgb error| <= cutoff per channel.  cutoff = 0 never terminates: the exact path.
#include "render_eval_common.hpp"
#include "raygen_common.hpp"

namespace snerf {

struct FrameRaygenArgs {
  float fx, fy, cx, cy, c2w[12], time;
  int W, H;
  int64_t p0, p1;
  float near_plane, aabb_min[3], aabb_max[3];
  float* origins; float* dirs; float* pixel_area; float* dir_norm; float* times; float* nears; float* fars;
};

// pixel p0 + r of the frame in row-major order -> ray r: the (row, col) the meshgrid index table would hold, then raygen_kernel's arithmetic
__global__ void raygen_frame_kernel(FrameRaygenArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.p1 - a.p0) return;
  const uint32_t pix = (uint32_t)(a.p0 + r);  // W * H < 2^31 (checked by the entry point)
  const uint32_t yi = pix / (uint32_t)a.W, xi = pix - yi * (uint32_t)a.W;
  const PixelRay p = pixel_ray((int64_t)yi, (int64_t)xi, a.fx, a.fy, a.cx, a.cy, a.c2w);
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.origins[r * 3 + k] = p.o[k]; a.dirs[r * 3 + k] = p.d[k]; }
  a.pixel_area[r] = p.pixel_area;
  a.dir_norm[r] = p.dir_norm;
  if (a.times) a.times[r] = a.time;
  aabb_interval(p.o, p.d, a.aabb_min, a.aabb_max, a.near_plane, 0, a.nears[r], a.fars[r]);
}

// raygen_frame_kernel through a lens: the same pixel walk, pixel_ray_lens for pixel_ray (a sibling: the pinhole kernel above stays as it was)
struct FrameRaygenLensArgs {
  FrameRaygenArgs base;
  float distortion[6];
};

__global__ void raygen_frame_lens_kernel(FrameRaygenLensArgs l) {
  const FrameRaygenArgs& a = l.base;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.p1 - a.p0) return;
  const uint32_t pix = (uint32_t)(a.p0 + r);  // W * H < 2^31 (checked by the entry point)
  const uint32_t yi = pix / (uint32_t)a.W, xi = pix - yi * (uint32_t)a.W;
  const PixelRay p = pixel_ray_lens((int64_t)yi, (int64_t)xi, a.fx, a.fy, a.cx, a.cy, a.c2w, l.distortion);
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.origins[r * 3 + k] = p.o[k]; a.dirs[r * 3 + k] = p.d[k]; }
  a.pixel_area[r] = p.pixel_area;
  a.dir_norm[r] = p.dir_norm;
  if (a.times) a.times[r] = a.time;
  aabb_interval(p.o, p.d, a.aabb_min, a.aabb_max, a.near_plane, 0, a.nears[r], a.fars[r]);
}

// raygen_frame_lens_kernel for a camera of any CameraType (cameras.py:645-700): the single type goes by value, so the branch is uniform
struct FrameRaygenCamArgs {
  FrameRaygenLensArgs lens;
  int camera_type, has_distortion;
};

__global__ void raygen_frame_cam_kernel(FrameRaygenCamArgs q) {
  const FrameRaygenArgs& a = q.lens.base;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.p1 - a.p0) return;
  const uint32_t pix = (uint32_t)(a.p0 + r);  // W * H < 2^31 (checked by the entry point)
  const uint32_t yi = pix / (uint32_t)a.W, xi = pix - yi * (uint32_t)a.W;
  const PixelRay p = pixel_ray_cam((int64_t)yi, (int64_t)xi, a.fx, a.fy, a.cx, a.cy, a.c2w, q.camera_type, q.has_distortion != 0, q.lens.distortion);
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.origins[r * 3 + k] = p.o[k]; a.dirs[r * 3 + k] = p.d[k]; }
  a.pixel_area[r] = p.pixel_area;
  a.dir_norm[r] = p.dir_norm;
  if (a.times) a.times[r] = a.time;
  aabb_interval(p.o, p.d, a.aabb_min, a.aabb_max, a.near_plane, 0, a.nears[r], a.fars[r]);
}

template <typename T, int NS>
static int launch_field_render(const FieldArgs& a, int R, const RayOut& o, hipStream_t st, bool vd) {
  using P = PlanFF<NS>;
  constexpr size_t BYTES = P::BYTES + RAY_LDS_B;
  const int grid = field_render_grid<NS>(R);
  if (vd) {
    auto k = field_render_kernel<T, NS, true, 6>;
    SNERF_ALLOW_LDS(k, LDS_LIMIT);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FF_NW * 64), BYTES, st, a, R, o);
  } else {
    auto k = field_render_kernel<T, NS, false, 6>;
    SNERF_ALLOW_LDS(k, LDS_LIMIT);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FF_NW * 64), BYTES, st, a, R, o);
  }
  SNERF_LAUNCH_CHECK("kplanes_field_render");
  return 0;
}

static bool render_shape_ok(int S) { return S >= FF_TS && S % FF_TS == 0 && S <= MAX_S; }

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_raygen_frame(const snerf_raygen_frame_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "raygen_frame: null args");
  SNERF_REQUIRE(p->W >= 1 && p->H >= 1 && (int64_t)p->W * p->H < (1LL << 31), "raygen_frame: W=%d H=%d", p->W, p->H);
  SNERF_REQUIRE(p->p0 >= 0 && p->p0 <= p->p1 && p->p1 <= (int64_t)p->W * p->H, "raygen_frame: pixel range [%lld, %lld) outside the %d x %d frame",
                (long long)p->p0, (long long)p->p1, p->W, p->H);
  if (p->p0 == p->p1) return 0;
  SNERF_REQUIRE(p->origins && p->dirs && p->pixel_area && p->dir_norm && p->nears && p->fars, "raygen_frame: null output buffer");
  FrameRaygenArgs a;
  a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy; a.time = p->time; a.W = p->W; a.H = p->H; a.p0 = p->p0; a.p1 = p->p1;
  for (int k = 0; k < 12; ++k) a.c2w[k] = p->c2w[k];
  a.near_plane = p->near_plane;
  for (int k = 0; k < 3; ++k) { a.aabb_min[k] = p->aabb_min[k]; a.aabb_max[k] = p->aabb_max[k]; }
  a.origins = p->origins; a.dirs = p->dirs; a.pixel_area = p->pixel_area; a.dir_norm = p->dir_norm; a.times = p->times; a.nears = p->nears; a.fars = p->fars;
  hipLaunchKernelGGL(raygen_frame_kernel, dim3(ceil_div(p->p1 - p->p0, 256)), dim3(256), 0, (hipStream_t)stream, a);
  SNERF_LAUNCH_CHECK("raygen_frame");
  return 0;
}

extern "C" int snerf_raygen_frame_lens(const snerf_raygen_frame_lens_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "raygen_frame_lens: null args");
  SNERF_REQUIRE(p->W >= 1 && p->H >= 1 && (int64_t)p->W * p->H < (1LL << 31), "raygen_frame_lens: W=%d H=%d", p->W, p->H);
  SNERF_REQUIRE(p->p0 >= 0 && p->p0 <= p->p1 && p->p1 <= (int64_t)p->W * p->H, "raygen_frame_lens: pixel range [%lld, %lld) outside the %d x %d frame",
                (long long)p->p0, (long long)p->p1, p->W, p->H);
  if (p->p0 == p->p1) return 0;
  SNERF_REQUIRE(p->origins && p->dirs && p->pixel_area && p->dir_norm && p->nears && p->fars, "raygen_frame_lens: null output buffer");
  FrameRaygenLensArgs l;
  FrameRaygenArgs& a = l.base;
  a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy; a.time = p->time; a.W = p->W; a.H = p->H; a.p0 = p->p0; a.p1 = p->p1;
  for (int k = 0; k < 12; ++k) a.c2w[k] = p->c2w[k];
  a.near_plane = p->near_plane;
  for (int k = 0; k < 3; ++k) { a.aabb_min[k] = p->aabb_min[k]; a.aabb_max[k] = p->aabb_max[k]; }
  a.origins = p->origins; a.dirs = p->dirs; a.pixel_area = p->pixel_area; a.dir_norm = p->dir_norm; a.times = p->times; a.nears = p->nears; a.fars = p->fars;
  for (int k = 0; k < 6; ++k) l.distortion[k] = p->distortion[k];
  hipLaunchKernelGGL(raygen_frame_lens_kernel, dim3(ceil_div(p->p1 - p->p0, 256)), dim3(256), 0, (hipStream_t)stream, l);
  SNERF_LAUNCH_CHECK("raygen_frame_lens");
  return 0;
}

extern "C" int snerf_raygen_frame_cam(const snerf_raygen_frame_cam_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "raygen_frame_cam: null args");
  SNERF_REQUIRE(p->camera_type >= CAMERA_PERSPECTIVE && p->camera_type <= CAMERA_EQUIRECTANGULAR,
                "raygen_frame_cam: camera_type=%d not supported (1: perspective, 2: fisheye, 3: equirectangular)", p->camera_type);
  SNERF_REQUIRE(p->W >= 1 && p->H >= 1 && (int64_t)p->W * p->H < (1LL << 31), "raygen_frame_cam: W=%d H=%d", p->W, p->H);
  SNERF_REQUIRE(p->p0 >= 0 && p->p0 <= p->p1 && p->p1 <= (int64_t)p->W * p->H, "raygen_frame_cam: pixel range [%lld, %lld) outside the %d x %d frame",
                (long long)p->p0, (long long)p->p1, p->W, p->H);
  if (p->p0 == p->p1) return 0;
  SNERF_REQUIRE(p->origins && p->dirs && p->pixel_area && p->dir_norm && p->nears && p->fars, "raygen_frame_cam: null output buffer");
  FrameRaygenCamArgs q;
  FrameRaygenArgs& a = q.lens.base;
  a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy; a.time = p->time; a.W = p->W; a.H = p->H; a.p0 = p->p0; a.p1 = p->p1;
  for (int k = 0; k < 12; ++k) a.c2w[k] = p->c2w[k];
  a.near_plane = p->near_plane;
  for (int k = 0; k < 3; ++k) { a.aabb_min[k] = p->aabb_min[k]; a.aabb_max[k] = p->aabb_max[k]; }
  a.origins = p->origins; a.dirs = p->dirs; a.pixel_area = p->pixel_area; a.dir_norm = p->dir_norm; a.times = p->times; a.nears = p->nears; a.fars = p->fars;
  for (int k = 0; k < 6; ++k) q.lens.distortion[k] = p->distortion[k];
  q.camera_type = p->camera_type; q.has_distortion = p->has_distortion != 0;
  hipLaunchKernelGGL(raygen_frame_cam_kernel, dim3(ceil_div(p->p1 - p->p0, 256)), dim3(256), 0, (hipStream_t)stream, q);
  SNERF_LAUNCH_CHECK("raygen_frame_cam");
  return 0;
}

extern "C" int snerf_kplanes_field_render_supported(const snerf_kplanes_desc* desc, const snerf_mlp_desc* sigma, const snerf_mlp_desc* color, int32_t S) {
  snerf_coords c = {};
  c.mode = 1;
  c.S = S >= 1 ? S : 1;
  return desc && sigma && color && render_shape_ok(S) && validate_field(desc, &c, 0, sigma, color, 6) == 0 ? 1 : 0;
}

extern "C" int snerf_kplanes_field_render(const snerf_kplanes_desc* desc, const float* planes, const snerf_coords* coords, int32_t R,
                                          const snerf_mlp_desc* sigma, const float* W_sigma, const snerf_mlp_desc* color, const float* W_color,
                                          float transmittance_cutoff, float* rgb_out, float* acc_out, float* depth_median, float* depth_expected,
                                          int64_t* median_index, int32_t* samples_done, snerf_stream_t stream) {
  SNERF_REQUIRE(coords && R >= 0, "kplanes_field_render: null coords or R=%d", R);
  SNERF_REQUIRE(coords->mode == 1 && render_shape_ok(coords->S),
                "kplanes_field_render: needs per-ray coordinates (coords.mode = 1) and S a multiple of %d, <= %d; got mode=%d S=%d", FF_TS, MAX_S,
                coords->mode, coords->S);
  int rc = validate_field(desc, coords, (int64_t)R * coords->S, sigma, color, 6);
  if (rc) return rc;
  SNERF_REQUIRE(transmittance_cutoff >= 0.f && transmittance_cutoff < 1.f, "kplanes_field_render: transmittance_cutoff=%g (0 <= cutoff < 1)",
                (double)transmittance_cutoff);
  if (R == 0) return 0;
  SNERF_REQUIRE(planes && W_sigma && W_color && rgb_out && acc_out, "kplanes_field_render: null buffer");
  FieldArgs a = {};
  a.d = *desc; a.planes = planes; a.c = *coords; a.N = (int64_t)R * coords->S; a.Wsig = W_sigma; a.Wcol = W_color;
  RayOut o = {transmittance_cutoff, rgb_out, acc_out, depth_median, depth_expected, median_index, samples_done};
  if (coords->contract) return launch_field_render_contract(a, R, o, sigma->operands, (hipStream_t)stream, color->d_in != FF_GEO);
  if (desc->n_coords == 3) return launch_field_render_static(a, R, o, sigma->operands, (hipStream_t)stream, color->d_in != FF_GEO);
  FF_DISPATCH_FWD(launch_field_render, sigma->operands, desc->n_scales, a, R, o, (hipStream_t)stream, color->d_in != FF_GEO);
}
