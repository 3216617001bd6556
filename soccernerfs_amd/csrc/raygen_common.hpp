// One pixel's ray (pinhole, through an OpenCV lens, or of a fisheye / equirectangular camera) and its AABB interval: the arithmetic of
// Cameras._generate_rays_from_coords (NS/cameras/cameras.py:596-741) and AABBBoxCollider._intersect_with_aabb (NS/model_components/scene_colliders.py:59-95), shared by the kernel that reads
// (camera, row, col) from an index table (raygen.hip) and the one that walks a frame's pixels in order (render_eval.hip): one copy, same bits.
// Contraction is off inside these functions whatever the including file sets: the reference rounds every product.
#pragma once
#include "common.hpp"

namespace snerf {

__device__ __forceinline__ void cam_to_world(const float* rot /*3x4 row-major*/, float x, float y, float z, float out[3], float& norm) {
#pragma clang fp contract(off)
  float v[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] = (x * rot[i * 4 + 0] + y * rot[i * 4 + 1]) + z * rot[i * 4 + 2];  // sum over the last axis (cameras.py:712-714)
  norm = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  // normalize_with_norm (NS/cameras/camera_utils.py:240-252): norm = max(|v|, 4*eps_f64); returns x / norm and norm
  norm = fmaxf(norm, 8.8817841970012523e-16f);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = v[i] / norm;
}

struct PixelRay {
  float o[3], d[3], pixel_area, dir_norm;
};

// pixel (row yi, column xi) of a camera with intrinsics fx, fy, cx, cy and camera-to-world m [3,4]
__device__ __forceinline__ PixelRay pixel_ray(int64_t yi, int64_t xi, float fx, float fy, float cx, float cy, const float* m) {
#pragma clang fp contract(off)
  const float y = (float)yi + 0.5f, x = (float)xi + 0.5f;  // image_coords = pixel index + 0.5 (cameras.py:318-319)
  float dx[3], dy[3], nx, ny;
  PixelRay p;
  cam_to_world(m, (x - cx) / fx, -(y - cy) / fy, -1.f, p.d, p.dir_norm);
  cam_to_world(m, ((x + 1.f) - cx) / fx, -(y - cy) / fy, -1.f, dx, nx);
  cam_to_world(m, (x - cx) / fx, -((y + 1.f) - cy) / fy, -1.f, dy, ny);
  const float* d0 = p.d;
  float ax = sqrtf(((d0[0] - dx[0]) * (d0[0] - dx[0]) + (d0[1] - dx[1]) * (d0[1] - dx[1])) + (d0[2] - dx[2]) * (d0[2] - dx[2]));
  float ay = sqrtf(((d0[0] - dy[0]) * (d0[0] - dy[0]) + (d0[1] - dy[1]) * (d0[1] - dy[1])) + (d0[2] - dy[2]) * (d0[2] - dy[2]));
  p.o[0] = m[3]; p.o[1] = m[7]; p.o[2] = m[11];
  p.pixel_area = ax * ay;
  return p;
}

// radial_and_tangential_undistort (NS/cameras/camera_utils.py:363-401) of ONE normalised coordinate pair for the OpenCV coefficients
// k = (k1, k2, k3, k4, p1, p2): Newton on the forward model from the distorted point, ten iterations, no early exit -- the reference runs all
// ten on every point.  Residual and Jacobian are _compute_residual_and_jacobian's (:298-360) statement by statement, every product rounded
// (Python's left-to-right association written out).  Both step components are zero when |denominator| <= eps = 1e-3 (torch.where, :395-396).
// With an all-zero k the residual is exactly zero (d = 1, x * 1 - x), so each step is 0 / -1 and (x, y) come back as they went in.
__device__ __forceinline__ void undistort_pair(float xd, float yd, const float k[6], float& x_out, float& y_out) {
#pragma clang fp contract(off)
  const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3], p1 = k[4], p2 = k[5];
  float x = xd, y = yd;
#pragma unroll 1
  for (int it = 0; it < 10; ++it) {
    const float r = x * x + y * y;
    const float d = 1.0f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
    const float fx = ((d * x + ((2.f * p1) * x) * y) + p2 * (r + (2.f * x) * x)) - xd;
    const float fy = ((d * y + ((2.f * p2) * x) * y) + p1 * (r + (2.f * y) * y)) - yd;
    const float d_r = k1 + r * (2.0f * k2 + r * (3.0f * k3 + (r * 4.0f) * k4));
    const float d_x = (2.0f * x) * d_r;
    const float d_y = (2.0f * y) * d_r;
    const float fx_x = ((d + d_x * x) + (2.0f * p1) * y) + (6.0f * p2) * x;
    const float fx_y = (d_y * x + (2.0f * p1) * x) + (2.0f * p2) * y;
    const float fy_x = (d_x * y + (2.0f * p2) * y) + (2.0f * p1) * x;
    const float fy_y = ((d + d_y * y) + (2.0f * p2) * x) + (6.0f * p1) * y;
    const float den = fy_x * fx_y - fx_x * fy_y;
    const float xn = fx * fy_y - fy * fx_y;
    const float yn = fy * fx_x - fx * fy_x;
    const bool ok = fabsf(den) > 1e-3f;
    x = x + (ok ? xn / den : 0.f);
    y = y + (ok ? yn / den : 0.f);
  }
  x_out = x; y_out = y;
}

// pixel_ray through a lens (cameras.py:620-653): the three coordinate pairs -- the pixel, x + 1, y + 1 -- are formed first, and EACH is
// undistorted on its own, so that the pixel area carries the lens's local Jacobian; from there on it is pixel_ray's code.
// One deliberate difference in rounding order from the reference: the offsets are formed as pixel_ray forms them, ((x + 1) - cx) / fx and
// -((y + 1) - cy) / fy, where cameras.py:623-624 writes (x - cx + 1) / fx and -(y - cy + 1) / fy.  For a non-integer cx the two can differ by one
// float32 ulp of the coordinate.  pixel_ray's form is what makes a zero row equal the pinhole kernel bit for bit; it touches the pixel area only.
__device__ __forceinline__ PixelRay pixel_ray_lens(int64_t yi, int64_t xi, float fx, float fy, float cx, float cy, const float* m, const float k[6]) {
#pragma clang fp contract(off)
  const float y = (float)yi + 0.5f, x = (float)xi + 0.5f;
  float c[3][2] = {{(x - cx) / fx, -(y - cy) / fy}, {((x + 1.f) - cx) / fx, -(y - cy) / fy}, {(x - cx) / fx, -((y + 1.f) - cy) / fy}};
#pragma unroll
  for (int i = 0; i < 3; ++i) undistort_pair(c[i][0], c[i][1], k, c[i][0], c[i][1]);
  float dx[3], dy[3], nx, ny;
  PixelRay p;
  cam_to_world(m, c[0][0], c[0][1], -1.f, p.d, p.dir_norm);
  cam_to_world(m, c[1][0], c[1][1], -1.f, dx, nx);
  cam_to_world(m, c[2][0], c[2][1], -1.f, dy, ny);
  const float* d0 = p.d;
  float ax = sqrtf(((d0[0] - dx[0]) * (d0[0] - dx[0]) + (d0[1] - dx[1]) * (d0[1] - dx[1])) + (d0[2] - dx[2]) * (d0[2] - dx[2]));
  float ay = sqrtf(((d0[0] - dy[0]) * (d0[0] - dy[0]) + (d0[1] - dy[1]) * (d0[1] - dy[1])) + (d0[2] - dy[2]) * (d0[2] - dy[2]));
  p.o[0] = m[3]; p.o[1] = m[7]; p.o[2] = m[11];
  p.pixel_area = ax * ay;
  return p;
}

// CameraType of NS/cameras/cameras.py:42-47 (the values of the reference's enum)
constexpr int CAMERA_PERSPECTIVE = 1, CAMERA_FISHEYE = 2, CAMERA_EQUIRECTANGULAR = 3;
constexpr float PI_F32 = 3.14159265358979323846f;  // math.pi / torch.pi as a float32 tensor operand holds it

// One (undistorted) coordinate pair -> the ray's direction in camera coordinates, by camera type (cameras.py:663-696); every product rounded,
// Python's left-to-right association written out.  An unknown type is treated as perspective: the callers refuse it before the launch.
__device__ __forceinline__ void camera_direction(int type, float cx, float cy, float d[3]) {
#pragma clang fp contract(off)
  if (type == CAMERA_FISHEYE) {  // :672-683
    float theta = sqrtf(cx * cx + cy * cy);
    theta = fminf(fmaxf(theta, 0.0f), PI_F32);  // torch.clip(theta, 0.0, math.pi)
    const float s = sinf(theta);
    // ONE deliberate deviation: at theta == 0 (a pixel centre exactly on the principal point) the reference's x * sin(theta) / theta is
    // 0 * 0 / 0 = NaN; here sin(theta) / theta := 1, its limit, so the ray is (0, 0, -1).  Every other input, theta clipped at pi included,
    // is the reference's expression (x * sin(theta)) / theta.
    d[0] = theta == 0.0f ? cx : (cx * s) / theta;
    d[1] = theta == 0.0f ? cy : (cy * s) / theta;
    d[2] = -cosf(theta);
  } else if (type == CAMERA_EQUIRECTANGULAR) {  // :685-696
    const float theta = -PI_F32 * cx;  // minus sign for right-handed
    const float phi = PI_F32 * (0.5f - cy);
    const float sp = sinf(phi);
    d[0] = -sinf(theta) * sp;
    d[1] = cosf(phi);
    d[2] = -cosf(theta) * sp;
  } else {  // :665-670
    d[0] = cx; d[1] = cy; d[2] = -1.f;
  }
}

// pixel_ray / pixel_ray_lens for a camera of any CameraType (cameras.py:620-741): the three coordinate pairs are formed as pixel_ray_lens forms
// them; each is undistorted unless there is no lens row (lens == false: k is not read) or the camera is equirectangular ("Do not apply
// distortion for equirectangular images", :645-647); each is mapped to its camera-space direction by type; the rest is pixel_ray's code.  For a
// perspective camera the statements are pixel_ray's (no lens) or pixel_ray_lens's, so the outputs are the same bits.  The row comes as a flag
// and an array, not as a nullable pointer: a pointer that may be null would put the array into scratch memory.
__device__ __forceinline__ PixelRay pixel_ray_cam(int64_t yi, int64_t xi, float fx, float fy, float cx, float cy, const float* m, int type, bool lens,
                                                  const float k[6]) {
#pragma clang fp contract(off)
  const float y = (float)yi + 0.5f, x = (float)xi + 0.5f;
  float c[3][2] = {{(x - cx) / fx, -(y - cy) / fy}, {((x + 1.f) - cx) / fx, -(y - cy) / fy}, {(x - cx) / fx, -((y + 1.f) - cy) / fy}};
  if (lens && type != CAMERA_EQUIRECTANGULAR) {
#pragma unroll
    for (int i = 0; i < 3; ++i) undistort_pair(c[i][0], c[i][1], k, c[i][0], c[i][1]);
  }
  float v[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) camera_direction(type, c[i][0], c[i][1], v[i]);
  float dx[3], dy[3], nx, ny;
  PixelRay p;
  cam_to_world(m, v[0][0], v[0][1], v[0][2], p.d, p.dir_norm);
  cam_to_world(m, v[1][0], v[1][1], v[1][2], dx, nx);
  cam_to_world(m, v[2][0], v[2][1], v[2][2], dy, ny);
  const float* d0 = p.d;
  float ax = sqrtf(((d0[0] - dx[0]) * (d0[0] - dx[0]) + (d0[1] - dx[1]) * (d0[1] - dx[1])) + (d0[2] - dx[2]) * (d0[2] - dx[2]));
  float ay = sqrtf(((d0[0] - dy[0]) * (d0[0] - dy[0]) + (d0[1] - dy[1]) * (d0[1] - dy[1])) + (d0[2] - dy[2]) * (d0[2] - dy[2]));
  p.o[0] = m[3]; p.o[1] = m[7]; p.o[2] = m[11];
  p.pixel_area = ax * ay;
  return p;
}

// The camera-space direction of a pixel's CENTRE: the first of pixel_ray_cam's three coordinate pairs, through the same statements (the
// pair, undistort_pair, camera_direction).  It does not depend on the camera-to-world matrix: the pose backward recomputes it as a constant.
__device__ __forceinline__ void pixel_camera_direction(int64_t yi, int64_t xi, float fx, float fy, float cx, float cy, int type, bool lens,
                                                       const float k[6], float v[3]) {
#pragma clang fp contract(off)
  const float y = (float)yi + 0.5f, x = (float)xi + 0.5f;
  float c0 = (x - cx) / fx, c1 = -(y - cy) / fy;
  if (lens && type != CAMERA_EQUIRECTANGULAR) undistort_pair(c0, c1, k, c0, c1);
  camera_direction(type, c0, c1, v);
}

// exp_map_SO3xR3 (NS/cameras/lie_groups.py:23-58) of one tangent vector a = (translation, so(3) vector): E = I + fac1 K + fac2 K^2 with
// K = skew(w), theta = sqrt(clamp(|w|^2, 1e-4)), fac1 = (1 / theta) sin(theta), fac2 = (1 / theta)(1 / theta)(1 - cos(theta)); the
// translation is a[0..3) as it stands.  K2 = K K is returned for the backward.  Every product rounded, in the reference's order.
struct PoseExp {
  float E[9], K[9], K2[9], fac1, fac2, nrms;
};
__device__ __forceinline__ PoseExp pose_exp_map(const float a[6]) {
#pragma clang fp contract(off)
  PoseExp e;
  const float wx = a[3], wy = a[4], wz = a[5];
  e.nrms = (wx * wx + wy * wy) + wz * wz;
  const float ang = sqrtf(fmaxf(e.nrms, 1e-4f));
  const float inv = 1.0f / ang;
  e.fac1 = inv * sinf(ang);
  e.fac2 = (inv * inv) * (1.0f - cosf(ang));
  const float K[9] = {0.f, -wz, wy, wz, 0.f, -wx, -wy, wx, 0.f};
#pragma unroll
  for (int i = 0; i < 9; ++i) e.K[i] = K[i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) e.K2[i * 3 + j] = (K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j]) + K[i * 3 + 2] * K[6 + j];
#pragma unroll
  for (int i = 0; i < 9; ++i) e.E[i] = (e.fac1 * e.K[i] + e.fac2 * e.K2[i]) + ((i % 4 == 0) ? 1.f : 0.f);
  return e;
}

// pose_utils.multiply(c2w, [E | tau]) (NS/utils/poses.py:53-67, as NS/cameras/cameras.py:707-708 composes it): R' = R E, t' = t + R tau
__device__ __forceinline__ void pose_compose(const float* m /*3x4*/, const float E[9], const float tau[3], float out[12]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out[i * 4 + j] = (m[i * 4] * E[j] + m[i * 4 + 1] * E[3 + j]) + m[i * 4 + 2] * E[6 + j];
    out[i * 4 + 3] = m[i * 4 + 3] + ((m[i * 4] * tau[0] + m[i * 4 + 1] * tau[1]) + m[i * 4 + 2] * tau[2]);
  }
}

// AABBBoxCollider: near_plane applies in training only
__device__ __forceinline__ void aabb_interval(const float o[3], const float d[3], const float mn[3], const float mx[3], float near_plane, int training,
                                              float& tn_out, float& tf_out) {
#pragma clang fp contract(off)
  float tn = -INFINITY, tf = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float inv = 1.f / (d[k] + 1e-6f);  // scene_colliders.py:71
    float t1 = (mn[k] - o[k]) * inv, t2 = (mx[k] - o[k]) * inv;
    tn = fmaxf(tn, fminf(t1, t2));
    tf = fminf(tf, fmaxf(t1, t2));
  }
  tn = fmaxf(tn, training ? near_plane : 0.f);
  tf = fmaxf(tf, tn + 1e-6f);
  tn_out = tn; tf_out = tf;
}

}  // namespace snerf
