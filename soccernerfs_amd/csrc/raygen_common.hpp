// One pixel's ray (pinhole, no distortion) and its AABB interval: the arithmetic of Cameras._generate_rays_from_coords (NS/cameras/cameras.py:596-633,
// :663-670, :704-741) and AABBBoxCollider._intersect_with_aabb (NS/model_components/scene_colliders.py:59-95), shared by the kernel that reads
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
