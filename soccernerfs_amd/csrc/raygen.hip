// Ray generation (pinhole, through the OpenCV lens distortion, or by camera type: perspective / fisheye / equirectangular) fused with the AABB
// collider, and the camera optimiser's two kernels around it: the pose rows composed into the camera table before the rays are formed, and the
// ray gradients taken back to the pose rows.
//
// Reference: RayGenerator.forward (NS/model_components/ray_generators.py:41-59) ->
// Cameras._generate_rays_from_coords (NS/cameras/cameras.py:505-741; the perspective slice :596-633,:663-670,
// :704-741 -- ~40 small ATen kernels incl. boolean-mask scatters) and AABBBoxCollider._intersect_with_aabb
// (NS/model_components/scene_colliders.py:59-95).  One lane per ray; the per-camera table (fx,fy,cx,cy,c2w,time)
// is a few KB and stays in L1/L2.  The raygen kernels themselves know nothing of the camera optimiser: snerf_pose_apply
// (CameraOptimizer.forward + cameras.py:707-708, NS/cameras/lie_groups.py:23-58; one lane per camera) writes the adjusted table they read,
// and snerf_raygen_pose_bwd (what autograd does from the rays back to pose_adjustment; one lane per ray, fixed-point cells) is their backward
// with respect to the pose rows.
#include "raygen_common.hpp"

#pragma clang fp contract(off)

namespace snerf {

struct RaygenArgs {
  const int64_t* indices;  // [R,3] (camera, row, col)
  const float* fx; const float* fy; const float* cx; const float* cy;  // [M]
  const float* c2w;        // [M,3,4]
  const float* cam_times;  // [M] or null
  int R;
  float* origins; float* dirs; float* pixel_area; float* dir_norm; float* times;  // [R,3],[R,3],[R],[R],[R]
  // collider
  int collide; int training; float near_plane;
  float aabb_min[3], aabb_max[3];
  float* nears; float* fars;  // [R]
};

__global__ void raygen_kernel(RaygenArgs a) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.R) return;
  const int64_t c = a.indices[(int64_t)r * 3], yi = a.indices[(int64_t)r * 3 + 1], xi = a.indices[(int64_t)r * 3 + 2];
  const PixelRay p = pixel_ray(yi, xi, a.fx[c], a.fy[c], a.cx[c], a.cy[c], a.c2w + c * 12);
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.origins[(int64_t)r * 3 + k] = p.o[k]; a.dirs[(int64_t)r * 3 + k] = p.d[k]; }
  a.pixel_area[r] = p.pixel_area;
  a.dir_norm[r] = p.dir_norm;
  if (a.times) a.times[r] = a.cam_times ? a.cam_times[c] : 0.f;
  if (a.collide) aabb_interval(p.o, p.d, a.aabb_min, a.aabb_max, a.near_plane, a.training, a.nears[r], a.fars[r]);
}

// raygen_kernel through the cameras' lens distortion (Cameras._generate_rays_from_coords with distortion_params, cameras.py:635-653): a sibling
// kernel, so that the pinhole kernel above is the code it always was.  distortion: [M,6] rows (stride 6) or one row for all cameras (stride 0).
struct RaygenLensArgs {
  RaygenArgs base;
  const float* distortion;
  int distortion_stride;
};

__global__ void raygen_lens_kernel(RaygenLensArgs l) {
  const RaygenArgs& a = l.base;
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.R) return;
  const int64_t c = a.indices[(int64_t)r * 3], yi = a.indices[(int64_t)r * 3 + 1], xi = a.indices[(int64_t)r * 3 + 2];
  float k[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) k[i] = l.distortion[c * l.distortion_stride + i];
  const PixelRay p = pixel_ray_lens(yi, xi, a.fx[c], a.fy[c], a.cx[c], a.cy[c], a.c2w + c * 12, k);
#pragma unroll
  for (int k3 = 0; k3 < 3; ++k3) { a.origins[(int64_t)r * 3 + k3] = p.o[k3]; a.dirs[(int64_t)r * 3 + k3] = p.d[k3]; }
  a.pixel_area[r] = p.pixel_area;
  a.dir_norm[r] = p.dir_norm;
  if (a.times) a.times[r] = a.cam_times ? a.cam_times[c] : 0.f;
  if (a.collide) aabb_interval(p.o, p.d, a.aabb_min, a.aabb_max, a.near_plane, a.training, a.nears[r], a.fars[r]);
}

// raygen_lens_kernel for a table of any camera types (Cameras._generate_rays_from_coords, cameras.py:645-700): each ray branches on ITS camera's
// type -- a mixed table is legal in the reference, and the lanes of a wavefront may diverge here.  Another sibling: the two kernels above stay
// the code they were.  camera_type: int32 [M] (stride 1), one shared value (stride 0) or null (all perspective); distortion may be null (no lens).
struct RaygenCamArgs {
  RaygenLensArgs lens;
  const int32_t* camera_type;
  int camera_type_stride;
};

__global__ void raygen_cam_kernel(RaygenCamArgs q) {
  const RaygenArgs& a = q.lens.base;
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.R) return;
  const int64_t c = a.indices[(int64_t)r * 3], yi = a.indices[(int64_t)r * 3 + 1], xi = a.indices[(int64_t)r * 3 + 2];
  const int type = q.camera_type ? q.camera_type[c * q.camera_type_stride] : CAMERA_PERSPECTIVE;
  const bool lens = q.lens.distortion != nullptr;
  float k[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) k[i] = lens ? q.lens.distortion[c * q.lens.distortion_stride + i] : 0.f;
  const PixelRay p = pixel_ray_cam(yi, xi, a.fx[c], a.fy[c], a.cx[c], a.cy[c], a.c2w + c * 12, type, lens, k);
#pragma unroll
  for (int k3 = 0; k3 < 3; ++k3) { a.origins[(int64_t)r * 3 + k3] = p.o[k3]; a.dirs[(int64_t)r * 3 + k3] = p.d[k3]; }
  a.pixel_area[r] = p.pixel_area;
  a.dir_norm[r] = p.dir_norm;
  if (a.times) a.times[r] = a.cam_times ? a.cam_times[c] : 0.f;
  if (a.collide) aabb_interval(p.o, p.d, a.aabb_min, a.aabb_max, a.near_plane, a.training, a.nears[r], a.fars[r]);
}

// PixelSampler.sample_method (NS/data/pixel_samplers.py:74-77: floor(rand(R,3) * [M,H,W]).long()) fused with the image gather of
// collate_image_dataset_batch (:111-123): one lane per ray instead of seven elementwise / index launches
__global__ void sample_pixels_kernel(const float* __restrict__ u, int R, int M, int H, int W, const uint8_t* __restrict__ images,
                                     int64_t* __restrict__ indices, float* __restrict__ target) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  // rand < 1 so the products stay below M, H, W except for the fp32 rounding of u * n at u -> 1: clamp like an index would fault otherwise
  int64_t c = (int64_t)floorf(u[(int64_t)r * 3] * (float)M), y = (int64_t)floorf(u[(int64_t)r * 3 + 1] * (float)H),
          x = (int64_t)floorf(u[(int64_t)r * 3 + 2] * (float)W);
  c = c < M ? c : M - 1; y = y < H ? y : H - 1; x = x < W ? x : W - 1;
  indices[(int64_t)r * 3] = c; indices[(int64_t)r * 3 + 1] = y; indices[(int64_t)r * 3 + 2] = x;
  if (images) {
    const uint8_t* px = images + (((int64_t)c * H + y) * W + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) target[(int64_t)r * 3 + k] = (float)px[k] / 255.0f;  // uint8 -> float32 / 255 (NS/data/datasets/base_dataset.py:82)
  }
}

// EquirectangularPixelSampler.sample_method (pixel_samplers.py:255-265): the draw that is uniform on the sphere of an equirectangular image --
// image and column as above, the row by inverse-transform sampling of f(phi) = sin(phi) / 2: floor((acos(1 - 2 u1) / pi) * H), in float32 with
// every operation rounded as torch rounds it -- with sample_pixels_kernel's gather.  u1 < 1 keeps acos below pi; the clamp is the same guard.
__global__ void sample_pixels_sphere_kernel(const float* __restrict__ u, int R, int M, int H, int W, const uint8_t* __restrict__ images,
                                            int64_t* __restrict__ indices, float* __restrict__ target) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float phi = acosf(1.0f - 2.0f * u[(int64_t)r * 3 + 1]) / PI_F32;
  int64_t c = (int64_t)floorf(u[(int64_t)r * 3] * (float)M), y = (int64_t)floorf(phi * (float)H), x = (int64_t)floorf(u[(int64_t)r * 3 + 2] * (float)W);
  c = c < M ? c : M - 1; y = y < H ? y : H - 1; x = x < W ? x : W - 1;
  y = y < 0 ? 0 : y;  // u1 outside [0, 1] (not a rand() value) makes acos NaN: keep the gather inside the image
  indices[(int64_t)r * 3] = c; indices[(int64_t)r * 3 + 1] = y; indices[(int64_t)r * 3 + 2] = x;
  if (images) {
    const uint8_t* px = images + (((int64_t)c * H + y) * W + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) target[(int64_t)r * 3 + k] = (float)px[k] / 255.0f;
  }
}

// The ray batch in order of a per-image key (the frame time): a batch is a set -- losses are means over it, the per-ray draws are i.i.d. -- so
// its order is free, and with equal-time rays next to each other every gather of a time plane (3 of the 6 planes of each scale; the
// temporal hash grid's rows likewise) finds the same two texel rows of its plane for the whole group instead of rows all over the plane:
// fused field forward 0.378 -> 0.309 ms at the k-planes preset (profiles/r03_kernels.md section 11).  One workgroup, bitonic sort in LDS of
// the words key << 14 | ray: unique words, so the order is a pure function of the batch (stable for equal keys).  256 threads on purpose: the
// kernel starts while the previous step's optimiser sweep fills the GPU, and a 1024-thread workgroup waited for sixteen free wave slots on one CU
// until the sweep had drained -- the whole head of the step behind it (measured: +0.1 ms per step).
__global__ __launch_bounds__(256) void sort_rays_kernel(const int64_t* __restrict__ idx_in, const int32_t* __restrict__ image_key, int R, int n_pow2,
                                                        const float* __restrict__ aux_in, int aux_cols, int64_t* __restrict__ idx_out,
                                                        float* __restrict__ aux_out) {
  extern __shared__ uint32_t s_w[];
  for (int i = threadIdx.x; i < n_pow2; i += blockDim.x)
    s_w[i] = i < R ? (((uint32_t)image_key[idx_in[(int64_t)i * 3]] << 14) | (uint32_t)i) : 0xffffffffu;
  __syncthreads();
  for (int k = 2; k <= n_pow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n_pow2 / 2; t += blockDim.x) {
        const int i = ((t / j) * 2 * j) + (t % j), l = i + j;  // j is a power of two: shifts and masks
        const bool up = (i & k) == 0;
        const uint32_t a = s_w[i], b = s_w[l];
        if ((a > b) == up) { s_w[i] = b; s_w[l] = a; }
      }
      __syncthreads();
    }
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const int64_t src = s_w[r] & 0x3fffu;
#pragma unroll
    for (int c = 0; c < 3; ++c) idx_out[(int64_t)r * 3 + c] = idx_in[src * 3 + c];
    for (int c = 0; c < aux_cols; ++c) aux_out[(int64_t)r * aux_cols + c] = aux_in[src * aux_cols + c];
  }
}

// The permutation that sorts the rays' times ascending, ties by ray index: the same one-workgroup bitonic sort, on 64-bit words (time bits << 32 | ray).
// Times are non-negative, so their bit patterns order as unsigned integers; whatever the bits are, the low words are the distinct ray indices and the
// padding word is above every key, so the output is always a permutation of 0..R-1.
__global__ __launch_bounds__(256) void ray_time_order_kernel(const float* __restrict__ times, int R, int n_pow2, int32_t* __restrict__ order_out) {
  extern __shared__ uint64_t s_tk[];
  for (int i = threadIdx.x; i < n_pow2; i += blockDim.x)
    s_tk[i] = i < R ? (((uint64_t)__float_as_uint(times[i]) << 32) | (uint32_t)i) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= n_pow2; k <<= 1)
    for (int lj = 31 - __clz(k >> 1); lj >= 0; --lj) {  // partner distance j = 2^lj
      const int j = 1 << lj;
      for (int t = threadIdx.x; t < n_pow2 / 2; t += blockDim.x) {
        const int i = ((t >> lj) << (lj + 1)) | (t & (j - 1)), l = i + j;
        const bool up = (i & k) == 0;
        const uint64_t a = s_tk[i], b = s_tk[l];
        if ((a > b) == up) { s_tk[i] = b; s_tk[l] = a; }
      }
      __syncthreads();
    }
  for (int r = threadIdx.x; r < R; r += blockDim.x) order_out[r] = (int32_t)(uint32_t)s_tk[r];
}

__global__ void aabb_kernel(const float* __restrict__ o, const float* __restrict__ d, int R, float near_plane, int training, const float* amin3,
                            float* __restrict__ nears, float* __restrict__ fars, float a0, float a1, float a2, float b0, float b1, float b2) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float mn[3] = {a0, a1, a2}, mx[3] = {b0, b1, b2};
  float tn = -INFINITY, tf = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float inv = 1.f / (d[(int64_t)r * 3 + k] + 1e-6f);
    float t1 = (mn[k] - o[(int64_t)r * 3 + k]) * inv, t2 = (mx[k] - o[(int64_t)r * 3 + k]) * inv;
    tn = fmaxf(tn, fminf(t1, t2));
    tf = fminf(tf, fmaxf(t1, t2));
  }
  tn = fmaxf(tn, training ? near_plane : 0.f);
  tf = fmaxf(tf, tn + 1e-6f);
  nears[r] = tn; fars[r] = tf;
}

// CameraOptimizer.forward + the composition of cameras.py:707-708 for the whole table: one lane per camera.  group: int32 [M] (the row of
// pose_adjustment each camera reads) or null (row m).  An all-zero row copies the camera through: the composition would give the same values
// (E is the identity exactly) but turn a -0.0 of the table into +0.0, and a zero-initialised optimiser must leave the rays bit-identical.
__global__ void pose_apply_kernel(const float* __restrict__ c2w, const float* __restrict__ adj, const int32_t* __restrict__ group, int M, int G,
                                  float* __restrict__ out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int g = group ? group[m] : m;
  float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool zero = true;
  if (g >= 0 && g < G) {  // a row outside the table is the identity (the binding refuses such a table)
#pragma unroll
    for (int i = 0; i < 6; ++i) { a[i] = adj[(int64_t)g * 6 + i]; zero = zero && a[i] == 0.f; }
  }
  float mm[12], o[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) mm[i] = c2w[(int64_t)m * 12 + i];
  if (zero) {
#pragma unroll
    for (int i = 0; i < 12; ++i) o[i] = mm[i];
  } else {
    const PoseExp e = pose_exp_map(a);
    pose_compose(mm, e.E, a, o);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) out[(int64_t)m * 12 + i] = o[i];
}

// d(sum g_o . o + g_d . d) / d pose_adjustment, one lane per ray: the camera-space direction v is recomputed (a constant of the pose), then
//   d = w / |w|, w = R E v        ->  g_w = (g_d - d (d . g_d)) / |w|,  g_E = (R^T g_w) v^T
//   o = t + R tau                 ->  g_tau = R^T g_o
//   E = I + fac1 K + fac2 K^2     ->  g_K = fac1 g_E + fac2 (g_E K^T + K^T g_E),  g_fac1 = <g_E, K>,  g_fac2 = <g_E, K^2>
// fac1 and fac2 are constants while |w|^2 < 1e-4 (torch.clamp passes no gradient below its bound), as autograd sees them; from the bound on they
// carry gradient through theta.  Rows are accumulated in 2^50-scaled 64-bit cells: any arrival order gives the same bits.
struct PoseBwdArgs {
  const int64_t* indices;
  const float* fx; const float* fy; const float* cx; const float* cy;
  const float* c2w;
  const float* distortion; int distortion_stride;
  const int32_t* camera_type; int camera_type_stride;
  const float* adj; const int32_t* group;
  int M, G, R;
  const float* g_origins; const float* g_dirs;
  long long* grad_pose_fx;
  int32_t* nonfinite_flag;
};

__global__ void raygen_pose_bwd_kernel(PoseBwdArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.R) return;
  const int64_t c = a.indices[(int64_t)r * 3], yi = a.indices[(int64_t)r * 3 + 1], xi = a.indices[(int64_t)r * 3 + 2];
  if (c < 0 || c >= a.M) return;
  const int g = a.group ? a.group[c] : (int)c;
  if (g < 0 || g >= a.G) return;
  const int type = a.camera_type ? a.camera_type[c * a.camera_type_stride] : CAMERA_PERSPECTIVE;
  const bool lens = a.distortion != nullptr;
  float k[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) k[i] = lens ? a.distortion[c * a.distortion_stride + i] : 0.f;
  float v[3];
  pixel_camera_direction(yi, xi, a.fx[c], a.fy[c], a.cx[c], a.cy[c], type, lens, k, v);
  float adj[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) adj[i] = a.adj[(int64_t)g * 6 + i];
  const PoseExp e = pose_exp_map(adj);
  const float* m = a.c2w + c * 12;
  float Rm[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rm[i * 3 + j] = m[i * 4 + j];
  // forward: w = R (E v), d = w / max(|w|, 4 eps)
  float ev[3], w[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ev[i] = e.E[i * 3] * v[0] + e.E[i * 3 + 1] * v[1] + e.E[i * 3 + 2] * v[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = Rm[i * 3] * ev[0] + Rm[i * 3 + 1] * ev[1] + Rm[i * 3 + 2] * ev[2];
  const float nraw = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const float n = fmaxf(nraw, 8.8817841970012523e-16f);
  const float d[3] = {w[0] / n, w[1] / n, w[2] / n};
  float go[3], gd[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { go[i] = a.g_origins[(int64_t)r * 3 + i]; gd[i] = a.g_dirs[(int64_t)r * 3 + i]; }
  const float dg = d[0] * gd[0] + d[1] * gd[1] + d[2] * gd[2];
  float gw[3], u[3], gtau[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) gw[i] = (gd[i] - (nraw > 8.8817841970012523e-16f ? d[i] * dg : 0.f)) / n;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    u[j] = Rm[j] * gw[0] + Rm[3 + j] * gw[1] + Rm[6 + j] * gw[2];     // R^T g_w
    gtau[j] = Rm[j] * go[0] + Rm[3 + j] * go[1] + Rm[6 + j] * go[2];  // R^T g_o
  }
  float gE[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) gE[i * 3 + j] = u[i] * v[j];
  float gK[9];
  float gf1 = 0.f, gf2 = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float t = 0.f;  // (g_E K^T + K^T g_E)[i][j]
#pragma unroll
      for (int l = 0; l < 3; ++l) t += gE[i * 3 + l] * e.K[j * 3 + l] + e.K[l * 3 + i] * gE[l * 3 + j];
      gK[i * 3 + j] = e.fac1 * gE[i * 3 + j] + e.fac2 * t;
      gf1 += gE[i * 3 + j] * e.K[i * 3 + j];
      gf2 += gE[i * 3 + j] * e.K2[i * 3 + j];
    }
  float gwv[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
  if (e.nrms >= 1e-4f) {  // above the clamp: fac1 = sin(th) / th, fac2 = (1 - cos(th)) / th^2, th = |w|
    const float th = sqrtf(e.nrms), sn = sinf(th), cs = cosf(th);
    const float df1 = (th * cs - sn) / (th * th);
    const float df2 = (th * sn - 2.f * (1.f - cs)) / (th * th * th);
    const float gth = (gf1 * df1 + gf2 * df2) / th;
#pragma unroll
    for (int i = 0; i < 3; ++i) gwv[i] += gth * adj[3 + i];
  }
  if (a.nonfinite_flag) {
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) finite = finite && fabsf(gtau[i]) <= 3.402823466e+38f && fabsf(gwv[i]) <= 3.402823466e+38f;
    if (!finite) *a.nonfinite_flag = 1;
  }
  long long* row = a.grad_pose_fx + (int64_t)g * 6;
#pragma unroll
  for (int i = 0; i < 3; ++i) { fx_atomic_add(row + i, gtau[i]); fx_atomic_add(row + 3 + i, gwv[i]); }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_raygen(const snerf_raygen_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "raygen: null args");
  SNERF_REQUIRE(p->R >= 0, "raygen: R=%d", p->R);
  if (p->R == 0) return 0;
  SNERF_REQUIRE(p->indices && p->fx && p->fy && p->cx && p->cy && p->c2w, "raygen: null camera/index buffer");
  SNERF_REQUIRE(p->origins && p->dirs && p->pixel_area && p->dir_norm, "raygen: null output buffer");
  SNERF_REQUIRE(!p->collide || (p->nears && p->fars), "raygen: collide set but nears/fars null");
  RaygenArgs a;
  a.indices = p->indices; a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy; a.c2w = p->c2w; a.cam_times = p->cam_times; a.R = p->R;
  a.origins = p->origins; a.dirs = p->dirs; a.pixel_area = p->pixel_area; a.dir_norm = p->dir_norm; a.times = p->times;
  a.collide = p->collide; a.training = p->training; a.near_plane = p->near_plane;
  for (int k = 0; k < 3; ++k) { a.aabb_min[k] = p->aabb_min[k]; a.aabb_max[k] = p->aabb_max[k]; }
  a.nears = p->nears; a.fars = p->fars;
  hipLaunchKernelGGL(raygen_kernel, dim3(ceil_div(p->R, 256)), dim3(256), 0, (hipStream_t)stream, a);
  SNERF_LAUNCH_CHECK("raygen");
  return 0;
}

extern "C" int snerf_raygen_lens(const snerf_raygen_lens_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "raygen_lens: null args");
  SNERF_REQUIRE(p->R >= 0, "raygen_lens: R=%d", p->R);
  SNERF_REQUIRE(p->distortion_stride == 0 || p->distortion_stride == 6, "raygen_lens: distortion_stride=%d (0: one shared row, 6: a [M,6] table)",
                p->distortion_stride);
  if (p->R == 0) return 0;
  SNERF_REQUIRE(p->indices && p->fx && p->fy && p->cx && p->cy && p->c2w && p->distortion, "raygen_lens: null camera/index/distortion buffer");
  SNERF_REQUIRE(p->origins && p->dirs && p->pixel_area && p->dir_norm, "raygen_lens: null output buffer");
  SNERF_REQUIRE(!p->collide || (p->nears && p->fars), "raygen_lens: collide set but nears/fars null");
  RaygenLensArgs l;
  RaygenArgs& a = l.base;
  a.indices = p->indices; a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy; a.c2w = p->c2w; a.cam_times = p->cam_times; a.R = p->R;
  a.origins = p->origins; a.dirs = p->dirs; a.pixel_area = p->pixel_area; a.dir_norm = p->dir_norm; a.times = p->times;
  a.collide = p->collide; a.training = p->training; a.near_plane = p->near_plane;
  for (int k = 0; k < 3; ++k) { a.aabb_min[k] = p->aabb_min[k]; a.aabb_max[k] = p->aabb_max[k]; }
  a.nears = p->nears; a.fars = p->fars;
  l.distortion = p->distortion; l.distortion_stride = p->distortion_stride;
  hipLaunchKernelGGL(raygen_lens_kernel, dim3(ceil_div(p->R, 256)), dim3(256), 0, (hipStream_t)stream, l);
  SNERF_LAUNCH_CHECK("raygen_lens");
  return 0;
}

extern "C" int snerf_raygen_cam(const snerf_raygen_cam_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "raygen_cam: null args");
  SNERF_REQUIRE(p->R >= 0, "raygen_cam: R=%d", p->R);
  SNERF_REQUIRE(p->distortion_stride == 0 || p->distortion_stride == 6, "raygen_cam: distortion_stride=%d (0: one shared row, 6: a [M,6] table)",
                p->distortion_stride);
  SNERF_REQUIRE(p->camera_type_stride == 0 || p->camera_type_stride == 1, "raygen_cam: camera_type_stride=%d (0: one shared value, 1: an [M] table)",
                p->camera_type_stride);
  if (p->R == 0) return 0;
  SNERF_REQUIRE(p->indices && p->fx && p->fy && p->cx && p->cy && p->c2w, "raygen_cam: null camera/index buffer");
  SNERF_REQUIRE(p->origins && p->dirs && p->pixel_area && p->dir_norm, "raygen_cam: null output buffer");
  SNERF_REQUIRE(!p->collide || (p->nears && p->fars), "raygen_cam: collide set but nears/fars null");
  RaygenCamArgs q;
  RaygenArgs& a = q.lens.base;
  a.indices = p->indices; a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy; a.c2w = p->c2w; a.cam_times = p->cam_times; a.R = p->R;
  a.origins = p->origins; a.dirs = p->dirs; a.pixel_area = p->pixel_area; a.dir_norm = p->dir_norm; a.times = p->times;
  a.collide = p->collide; a.training = p->training; a.near_plane = p->near_plane;
  for (int k = 0; k < 3; ++k) { a.aabb_min[k] = p->aabb_min[k]; a.aabb_max[k] = p->aabb_max[k]; }
  a.nears = p->nears; a.fars = p->fars;
  q.lens.distortion = p->distortion; q.lens.distortion_stride = p->distortion_stride;
  q.camera_type = p->camera_type; q.camera_type_stride = p->camera_type_stride;
  hipLaunchKernelGGL(raygen_cam_kernel, dim3(ceil_div(p->R, 256)), dim3(256), 0, (hipStream_t)stream, q);
  SNERF_LAUNCH_CHECK("raygen_cam");
  return 0;
}

extern "C" int snerf_sample_pixels_sphere(const float* u, int32_t R, int32_t M, int32_t H, int32_t W, const uint8_t* images, int64_t* indices,
                                          float* target, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && M >= 1 && H >= 1 && W >= 1, "sample_pixels_sphere: R=%d M=%d H=%d W=%d", R, M, H, W);
  if (R == 0) return 0;
  SNERF_REQUIRE(u && indices && (!images || target), "sample_pixels_sphere: null buffer");
  hipLaunchKernelGGL(sample_pixels_sphere_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, (hipStream_t)stream, u, R, M, H, W, images, indices, target);
  SNERF_LAUNCH_CHECK("sample_pixels_sphere");
  return 0;
}

extern "C" int snerf_sample_pixels_uniform(const float* u, int32_t R, int32_t M, int32_t H, int32_t W, const uint8_t* images, int64_t* indices,
                                           float* target, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && M >= 1 && H >= 1 && W >= 1, "sample_pixels_uniform: R=%d M=%d H=%d W=%d", R, M, H, W);
  if (R == 0) return 0;
  SNERF_REQUIRE(u && indices && (!images || target), "sample_pixels_uniform: null buffer");
  hipLaunchKernelGGL(sample_pixels_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, (hipStream_t)stream, u, R, M, H, W, images, indices, target);
  SNERF_LAUNCH_CHECK("sample_pixels_uniform");
  return 0;
}

extern "C" int snerf_sort_rays_by_key(const int64_t* indices_in, const int32_t* image_key, int32_t n_keys, int32_t R, const float* aux_in,
                                      int32_t aux_cols, int64_t* indices_out, float* aux_out, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && R <= 16384 && n_keys >= 1 && n_keys <= (1 << 18) && aux_cols >= 0,
                "sort_rays_by_key: R=%d (<= 16384) n_keys=%d (<= 262144) aux_cols=%d", R, n_keys, aux_cols);
  if (R == 0) return 0;
  SNERF_REQUIRE(indices_in && image_key && indices_out && indices_in != indices_out && (aux_cols == 0 || (aux_in && aux_out && aux_in != aux_out)),
                "sort_rays_by_key: null or aliased buffer (the sort is out of place)");
  int n = 2;
  while (n < R) n <<= 1;
  hipLaunchKernelGGL(sort_rays_kernel, dim3(1), dim3(256), (size_t)n * sizeof(uint32_t), (hipStream_t)stream, indices_in, image_key, R, n, aux_in, aux_cols,
                     indices_out, aux_out);
  SNERF_LAUNCH_CHECK("sort_rays_by_key");
  return 0;
}

extern "C" int snerf_ray_time_order(const float* times, int32_t R, int32_t* order_out, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && R <= 16384, "ray_time_order: R=%d (<= 16384: one workgroup sorts in LDS)", R);
  if (R == 0) return 0;
  SNERF_REQUIRE(times && order_out, "ray_time_order: null buffer");
  int n = 2;
  while (n < R) n <<= 1;
  SNERF_ALLOW_LDS(ray_time_order_kernel, 16384 * (int)sizeof(uint64_t));  // 128 KB at the largest R
  hipLaunchKernelGGL(ray_time_order_kernel, dim3(1), dim3(256), (size_t)n * sizeof(uint64_t), (hipStream_t)stream, times, R, n, order_out);
  SNERF_LAUNCH_CHECK("ray_time_order");
  return 0;
}

extern "C" int snerf_aabb_collide(const float* origins, const float* dirs, int32_t R, const float* aabb6, float near_plane, int32_t training,
                                  float* nears, float* fars, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && aabb6, "aabb_collide: bad arguments");
  if (R == 0) return 0;
  SNERF_REQUIRE(origins && dirs && nears && fars, "aabb_collide: null buffer");
  hipLaunchKernelGGL(aabb_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, (hipStream_t)stream, origins, dirs, R, near_plane, training, nullptr, nears,
                     fars, aabb6[0], aabb6[1], aabb6[2], aabb6[3], aabb6[4], aabb6[5]);
  SNERF_LAUNCH_CHECK("aabb_collide");
  return 0;
}

extern "C" int snerf_pose_apply(const float* c2w, const float* pose_adjustment, const int32_t* group, int32_t M, int32_t G, float* c2w_adj,
                                snerf_stream_t stream) {
  SNERF_REQUIRE(M >= 0 && G >= 0, "pose_apply: M=%d G=%d", M, G);
  SNERF_REQUIRE(group || G == M, "pose_apply: no group table, so G=%d must equal M=%d", G, M);
  if (M == 0) return 0;
  SNERF_REQUIRE(c2w && pose_adjustment && c2w_adj, "pose_apply: null buffer");
  hipLaunchKernelGGL(pose_apply_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, (hipStream_t)stream, c2w, pose_adjustment, group, M, G, c2w_adj);
  SNERF_LAUNCH_CHECK("pose_apply");
  return 0;
}

extern "C" int snerf_raygen_pose_bwd(const snerf_raygen_pose_bwd_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "raygen_pose_bwd: null args");
  SNERF_REQUIRE(p->R >= 0 && p->M >= 1 && p->G >= 1, "raygen_pose_bwd: R=%d M=%d G=%d", p->R, p->M, p->G);
  SNERF_REQUIRE(p->group || p->G == p->M, "raygen_pose_bwd: no group table, so G=%d must equal M=%d", p->G, p->M);
  SNERF_REQUIRE(p->distortion_stride == 0 || p->distortion_stride == 6, "raygen_pose_bwd: distortion_stride=%d (0: one shared row, 6: a [M,6] table)",
                p->distortion_stride);
  SNERF_REQUIRE(p->camera_type_stride == 0 || p->camera_type_stride == 1, "raygen_pose_bwd: camera_type_stride=%d (0: one shared value, 1: an [M] table)",
                p->camera_type_stride);
  if (p->R == 0) return 0;
  SNERF_REQUIRE(p->indices && p->fx && p->fy && p->cx && p->cy && p->c2w && p->pose_adjustment, "raygen_pose_bwd: null camera/index/pose buffer");
  SNERF_REQUIRE(p->g_origins && p->g_dirs && p->grad_pose_fx, "raygen_pose_bwd: null gradient buffer");
  PoseBwdArgs a;
  a.indices = p->indices; a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy; a.c2w = p->c2w;
  a.distortion = p->distortion; a.distortion_stride = p->distortion_stride;
  a.camera_type = p->camera_type; a.camera_type_stride = p->camera_type_stride;
  a.adj = p->pose_adjustment; a.group = p->group; a.M = p->M; a.G = p->G; a.R = p->R;
  a.g_origins = p->g_origins; a.g_dirs = p->g_dirs; a.grad_pose_fx = reinterpret_cast<long long*>(p->grad_pose_fx);
  a.nonfinite_flag = p->nonfinite_flag;
  hipLaunchKernelGGL(raygen_pose_bwd_kernel, dim3(ceil_div(p->R, 256)), dim3(256), 0, (hipStream_t)stream, a);
  SNERF_LAUNCH_CHECK("raygen_pose_bwd");
  return 0;
}
