// What the render-tail kernels share (render_eval.hip: six planes per scale; render_eval_static.hip: three): the ray's LDS behind the tile's
// plan, the per-ray compositing by one wavefront, and the kernel that walks a workgroup over its rays.
#pragma once
#include "field_fused_common.hpp"
#include "per_ray_common.hpp"

namespace snerf {

constexpr size_t RAY_LDS_B = sizeof(float) * (MAX_S * 6 + 4);  // a ray's density / prefix sums / colour / bin edges behind the tile's LDS plan

struct RayOut {
  float cutoff;
  float* rgb_out; float* acc_out; float* depth_median; float* depth_expected;
  int64_t* median_index; int32_t* samples_done;
};

// One ray by ONE wavefront from LDS: dd holds the densities of the first `done` samples on entry (the rest count as zero), col the colours,
// eb the S + 1 euclidean bin edges.  The phases of snerf_weights_fwd and of render_fwd_kernel in eval mode (per_ray_common.hpp), with the
// wave's own barrier between them.
__device__ __forceinline__ void composite_ray(float* dd, float* aux, const float* col, const float* eb, int S, int done, int64_t r, const RayOut& o,
                                              int lane) {
#pragma clang fp contract(off)
  ray_weights<WaveSync>(eb, dd, done, dd, aux, dd, nullptr, false, S, lane);  // from here on dd holds the weights
  wave_lds_publish();
  const RaySums s = ray_weighted_sums<true>(dd, nullptr, col, done, true, eb, S, lane);
  const int idx = ray_median_index<WaveSync>(dd, aux, S, lane);
  if (lane == 0) {
    float b[3], out[3];
    ray_background(1, nullptr, r, col + (done - 1) * 3, true, b);  // "last_sample" background: the last EVALUATED sample
    ray_blend(s, b, true, out);
    o.rgb_out[r * 3] = out[0]; o.rgb_out[r * 3 + 1] = out[1]; o.rgb_out[r * 3 + 2] = out[2];
    o.acc_out[r] = s.acc;
    if (o.median_index) o.median_index[r] = idx;
    if (o.depth_median) o.depth_median[r] = bin_midpoint(eb, idx);
    if (o.depth_expected) o.depth_expected[r] = s.dsum / (s.acc + 1e-10f);
    if (o.samples_done) o.samples_done[r] = done;
  }
}

// sum of delta * sigma over the tile's 32 samples, the same value in every lane of every wave
__device__ __forceinline__ float tile_optical_depth(const float* dens, const float* eb, int lane) {
#pragma clang fp contract(off)
  float v = 0.f;
  if (lane < FF_TS) v = (eb[lane + 1] - eb[lane]) * dens[lane];
  return wave_sum(v);
}

// The render kernel (render_eval.hip describes it).  NP: planes per scale -- 6 is instantiated by render_eval.hip, 3 (a 3-coordinate descriptor) by
// render_eval_static.hip.
template <typename T, int NS, bool VD, int NP = 6, int CT = 0>
__global__ __launch_bounds__(FF_NW * 64, 4) void field_render_kernel(FieldArgs a, int R, RayOut o) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  float* s_dd = reinterpret_cast<float*>(smem_raw + PlanFF<NS>::BYTES);  // [MAX_S] density, then delta * sigma, then the weights
  float* s_aux = s_dd + MAX_S;                                           // [MAX_S] the two prefix sums
  float* s_col = s_aux + MAX_S;                                          // [MAX_S, 3]
  float* s_eb = s_col + MAX_S * 3;                                       // [MAX_S + 1]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int S = a.c.S, n_tiles = S / FF_TS;
  typename Ops<T>::v8 breg[NS];
  field_stage_weights<T, NS, VD>(a, smem, breg);
  for (int ray = blockIdx.x; ray < R; ray += gridDim.x) {
    // the previous ray's compositing (wave 0) read s_eb: the barrier below is behind it for every wave
    __syncthreads();
    for (int i = threadIdx.x; i <= S; i += FF_NW * 64) s_eb[i] = a.c.ebins[(int64_t)ray * (S + 1) + i];
    float tau = 0.f;
    int done = S;
    for (int t = 0; t < n_tiles; ++t) {
      field_tile<T, NS, 0, VD, NP, CT>(
          a, (int64_t)ray * S + t * FF_TS, smem, breg, [&](int row, int64_t, float v) { s_dd[t * FF_TS + row] = v; },
          [&](int row, int64_t, int c, float v) { s_col[(t * FF_TS + row) * 3 + c] = v; });
      if (o.cutoff > 0.f && t + 1 < n_tiles) {
        // the tile's densities were published by the barrier behind the sigma_net output layer; s_eb by the tile's first barrier
        tau += tile_optical_depth(s_dd + t * FF_TS, s_eb + t * FF_TS, lane);
        if (expf(-tau) < o.cutoff) { done = (t + 1) * FF_TS; break; }  // workgroup-uniform: every wave formed the same tau
      }
    }
    __syncthreads();  // the last tile's colours (waves 0-1) are in LDS
    if (wave == 0) composite_ray(s_dd, s_aux, s_col, s_eb, S, done, ray, o, lane);
  }
}

// grid and dynamic LDS of the render kernels: two 8-wave workgroups per CU, as field_fwd_kernel
template <int NS>
inline int field_render_grid(int R) {
  int per_cu = (int)(LDS_LIMIT / (PlanFF<NS>::BYTES + RAY_LDS_B));
  per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
  const int grid = 256 * per_cu;
  return grid > R ? R : grid;
}

// the render tail for a 3-coordinate descriptor (render_eval_static.hip)
int launch_field_render_static(const FieldArgs& a, int R, const RayOut& o, int operands, hipStream_t st, bool vd);
// the render tail with contracted coordinates (a.c.contract = 1), six or three planes (render_eval_contract.hip)
int launch_field_render_contract(const FieldArgs& a, int R, const RayOut& o, int operands, hipStream_t st, bool vd);

}  // namespace snerf
