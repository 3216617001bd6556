// K-Planes plane gather: the gradient with respect to the sample COORDINATES, reduced to the ray.
//
// Replaces what autograd does in the reference when the camera optimiser is on: F.grid_sample differentiated with respect to its grid
// (ATen grid_sampler_2d_backward, bilinear, align_corners=True, border padding) x 6 planes per scale, the product rule of
// interpolate_kplanes (NS/fields/kplanes_field.py:77-126), then the chain through SceneBox.get_normalized_positions
// (NS/data/scene_box.py:55-65) and Frustums.get_positions (NS/cameras/rays.py:54) down to the ray's origin and direction.
//
// Shape: the forward gather's.  C/4 lanes own a sample and move float4s; both slopes of a plane come from the four texels the forward
// fetches, so the traffic is one forward gather plus the upstream gradient.  One WAVEFRONT owns a ray (mode 1) or a fixed block of samples
// (mode 0): the 64 / (C/4) lane groups walk the ray's samples in steps, the C/4 lanes of a group are summed with DPP / swizzle moves, and the
// per-ray sums go through a fixed butterfly -- no atomics, the same bits on every run.
//
// Bin edges are constants here (include/snerf.h): the gradient is that of moving the samples rigidly with the ray.
#include "kplanes_common.hpp"

namespace snerf {

// sum over the LPS = C/4 adjacent lanes that own one sample; every lane of the group ends with the total.  xor 1 and xor 2 are DPP quad
// permutations, xor 4 is ds_swizzle in bit mode (no memory access, no per-lane address) -- as xor_lanes in kplanes.hip
template <int LPS>
__device__ __forceinline__ float group_sum(float x) {
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
  if (LPS >= 4) x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
  if (LPS >= 8) x += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x101f));  // xor mask 4
  return x;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

// d(unnormalised, clipped coordinate) / d(coordinate): grid_sampler_compute_source_index_set_grad for align_corners=True + border padding --
// (size - 1) / 2, and zero where the unnormalised coordinate is clipped (<= 0 or >= size - 1), hence also for an axis of resolution 1
__device__ __forceinline__ float axis_slope(float x, int size) {
  const float fx = ((x + 1.f) / 2.f) * (float)(size - 1);
  return (fx <= 0.f || fx >= (float)(size - 1)) ? 0.f : (float)(size - 1) / 2.f;
}

// value of plane p for this lane's 4 channels and its slopes along the plane's two axes, per texel: from the forward's four texels
template <int C>
__device__ __forceinline__ void plane_sample_slopes(const float* __restrict__ base, int W, const AxisTap& tx, const AxisTap& ty, int cg, float4& v,
                                                    float4& da, float4& db) {
  const float* r0 = base + ((int64_t)ty.i0 * W) * C + cg * 4;
  const float* r1 = base + ((int64_t)ty.i1 * W) * C + cg * 4;
  const float4 nw = *reinterpret_cast<const float4*>(r0 + (int64_t)tx.i0 * C);
  const float4 ne = *reinterpret_cast<const float4*>(r0 + (int64_t)tx.i1 * C);
  const float4 sw = *reinterpret_cast<const float4*>(r1 + (int64_t)tx.i0 * C);
  const float4 se = *reinterpret_cast<const float4*>(r1 + (int64_t)tx.i1 * C);
  const float4 w = tap_weights(tx, ty);
  v = make_float4(bilerp4(nw.x, ne.x, sw.x, se.x, w.x, w.y, w.z, w.w), bilerp4(nw.y, ne.y, sw.y, se.y, w.x, w.y, w.z, w.w),
                  bilerp4(nw.z, ne.z, sw.z, se.z, w.x, w.y, w.z, w.w), bilerp4(nw.w, ne.w, sw.w, se.w, w.x, w.y, w.z, w.w));
  // an out-of-range corner (i1 clamped onto i0) makes its difference zero; it occurs only where the axis is clipped and the slope is dropped
  da = make_float4((ne.x - nw.x) * ty.w0 + (se.x - sw.x) * ty.w1, (ne.y - nw.y) * ty.w0 + (se.y - sw.y) * ty.w1,
                   (ne.z - nw.z) * ty.w0 + (se.z - sw.z) * ty.w1, (ne.w - nw.w) * ty.w0 + (se.w - sw.w) * ty.w1);
  db = make_float4((sw.x - nw.x) * tx.w0 + (se.x - ne.x) * tx.w1, (sw.y - nw.y) * tx.w0 + (se.y - ne.y) * tx.w1,
                   (sw.z - nw.z) * tx.w0 + (se.z - ne.z) * tx.w1, (sw.w - nw.w) * tx.w0 + (se.w - ne.w) * tx.w1);
}

// g (the gradient w.r.t. p = contract_inf_half(pos), first three components) -> the gradient w.r.t. pos: the contraction's Jacobian
// transposed.  Inside (m < 1) p = pos / 2.  Outside p_k = f(m) pos_k / 2 with f = 2/m - 1/m^2 and m = |pos_j|:
//   h_k = (f g_k + [k == j] f'(m) sign(pos_j) sum_i pos_i g_i) / 2,   f' = -2/m^2 + 2/m^3.
// j is the FIRST axis that attains the maximum (autograd splits a tie evenly; ties have measure zero).  m == 1 goes outside, as in the forward.
__device__ __forceinline__ void contract_inf_half_vjp(const float pos[3], float g[4]) {
  const float a0 = fabsf(pos[0]), a1 = fabsf(pos[1]), a2 = fabsf(pos[2]);
  const float m = fmaxf(fmaxf(a0, a1), a2);
  if (m < 1.f) {
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = g[k] / 2.f;
    return;
  }
  const int j = a0 == m ? 0 : (a1 == m ? 1 : 2);
  const float pj = j == 0 ? pos[0] : (j == 1 ? pos[1] : pos[2]);
  const float a = 2.f / m - 1.f / (m * m);
  const float b = (-2.f / (m * m) + 2.f / (m * m * m)) * (pj < 0.f ? -1.f : 1.f);
  const float dot = (pos[0] * g[0] + pos[1] * g[1]) + pos[2] * g[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = (a * g[k] + (k == j ? b * dot : 0.f)) / 2.f;
}

constexpr int COORDS_BLOCK_STEPS = 4;  // mode 0: a wavefront takes 4 steps of its 64 / LPS lane groups

// CT: 1 = contracted coordinates (snerf_coords.contract).  Compile time: as a run-time branch it cost the six-plane kernel an occupancy step.
template <int C, int NP, int CT = 0>
__global__ __launch_bounds__(256) void kplanes_gather_bwd_coords_kernel(snerf_kplanes_desc d, const float* __restrict__ planes, snerf_coords c,
                                                                       int64_t N, const float* __restrict__ gout, float* __restrict__ gpts,
                                                                       float* __restrict__ g_origins, float* __restrict__ g_dirs) {
  constexpr int LPS = C / 4;      // lanes per sample
  constexpr int GROUPS = 64 / LPS;  // samples per wavefront step
  const int lane = threadIdx.x & 63;
  const int grp = lane / LPS, cg = lane % LPS;
  const int per = c.mode == 1 ? c.S : GROUPS * COORDS_BLOCK_STEPS;  // samples owned by one wavefront
  const int64_t owner = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;  // the ray (mode 1) or sample block (mode 0)
  const int64_t n0 = owner * per;
  if (n0 >= N) return;  // uniform over the wavefront
  const int out_w = d.concat ? C * d.n_scales : C;
  constexpr int NC = NP == 6 ? 4 : 3;

  float ro[3] = {0.f, 0.f, 0.f}, rd[3] = {0.f, 0.f, 0.f};  // this lane group's share of the ray's sums
  for (int i0 = 0; i0 < per; i0 += GROUPS) {
    const int i = i0 + grp;
    const int64_t n = n0 + i;
    const bool active = i < per && n < N;
    float gp[4] = {0.f, 0.f, 0.f, 0.f};
    float tmid = 0.f;
    float pos[3] = {0.f, 0.f, 0.f};  // contract = 1: the sample's Euclidean position, for the contraction's Jacobian
    if (active) {
      float p[4];
      if (c.mode == 1) {
        load_coords_ray<NP, CT>(c, owner, i, p);
        if constexpr (CT == 1) ray_position(c, owner, i, pos);
        const float* eb = c.ebins + owner * (c.S + 1) + i;
        tmid = (eb[0] + eb[1]) / 2.f;
      } else {
        load_coords<NP>(c, n, p);
      }
      const float* grow = gout + n * out_w + cg * 4;
      for (int s = 0; s < d.n_scales; ++s) {
        AxisTap tap[4];
        float slope[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int res = d.res[s][k] > 0 ? d.res[s][k] : 1;
          tap[k] = axis_tap(p[k], res);
          slope[k] = axis_slope(p[k], res);
        }
        float4 v[NP], da[NP], db[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q)
          plane_sample_slopes<C>(planes + d.off[s][q], d.res[s][pair_a<NP>(q)], tap[pair_a<NP>(q)], tap[pair_b<NP>(q)], cg, v[q], da[q], db[q]);
        float4 others[NP];  // upstream gradient times every plane but q
        leave_one_out<NP>(*reinterpret_cast<const float4*>(grow + (d.concat ? s * C : 0)), v, others);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};  // in texels
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          acc[pair_a<NP>(q)] += dot4(others[q], da[q]);
          acc[pair_b<NP>(q)] += dot4(others[q], db[q]);
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) gp[k] += acc[k] * slope[k];
      }
    }
    // all 64 lanes take part in the lane moves, active or not (an idle group adds zeros)
#pragma unroll
    for (int k = 0; k < NC; ++k) gp[k] = group_sum<LPS>(gp[k]);
    if (active) {
      if (gpts && cg == 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) gpts[n * NC + k] = gp[k];
      }
      if constexpr (CT == 1) contract_inf_half_vjp(pos, gp);  // gp[0..2] become d / d(pos), written to grad_pts above as d / d(p)
#pragma unroll
      for (int k = 0; k < 3; ++k) { ro[k] += gp[k]; rd[k] += tmid * gp[k]; }
    }
  }
  if (c.mode != 1 || (!g_origins && !g_dirs)) return;
  // the lane groups' shares -> the ray: a butterfly over the group index (every lane of a group holds the same share); once per ray
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = LPS; off < 64; off <<= 1) {
      ro[k] += __shfl_xor(ro[k], off, 64);
      rd[k] += __shfl_xor(rd[k], off, 64);
    }
  }
  if (lane < 3) {  // selects, not a lane-indexed read of the argument block (that would copy it to scratch)
    const float ext = lane == 0 ? c.aabb_max[0] - c.aabb_min[0] : lane == 1 ? c.aabb_max[1] - c.aabb_min[1] : c.aabb_max[2] - c.aabb_min[2];
    const float scale = CT == 1 ? 1.f : (c.rescale ? 2.f : 1.f) / ext;  // contracted: the Jacobian went in per sample, the box is not read
    const float so = lane == 0 ? ro[0] : lane == 1 ? ro[1] : ro[2];
    const float sd = lane == 0 ? rd[0] : lane == 1 ? rd[1] : rd[2];
    if (g_origins) g_origins[owner * 3 + lane] += scale * so;
    if (g_dirs) g_dirs[owner * 3 + lane] += scale * sd;
  }
}

template <int C, int NP>
static int launch_bwd_coords(const snerf_kplanes_desc* d, const float* planes, const snerf_coords* c, int64_t N, const float* gout, float* gpts,
                             float* go, float* gd, hipStream_t st) {
  const int64_t per = c->mode == 1 ? c->S : (64 / (C / 4)) * COORDS_BLOCK_STEPS;
  const int64_t owners = (N + per - 1) / per;
  if (c->contract)
    hipLaunchKernelGGL((kplanes_gather_bwd_coords_kernel<C, NP, 1>), dim3(ceil_div(owners, 4)), dim3(256), 0, st, *d, planes, *c, N, gout, gpts, go, gd);
  else
    hipLaunchKernelGGL((kplanes_gather_bwd_coords_kernel<C, NP, 0>), dim3(ceil_div(owners, 4)), dim3(256), 0, st, *d, planes, *c, N, gout, gpts, go, gd);
  SNERF_LAUNCH_CHECK("kplanes_gather_bwd_coords");
  return 0;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_kplanes_gather_bwd_coords(const snerf_kplanes_desc* desc, const float* planes, const snerf_coords* coords, int64_t N,
                                               const float* grad_out, float* grad_pts, float* grad_origins, float* grad_dirs,
                                               snerf_stream_t stream) {
  // the shapes kplanes.hip's validate() admits
  SNERF_REQUIRE(desc && coords, "kplanes_gather_bwd_coords: null descriptor");
  SNERF_REQUIRE(desc->n_scales >= 1 && desc->n_scales <= SNERF_MAX_SCALES, "kplanes_gather_bwd_coords: n_scales=%d out of range", desc->n_scales);
  SNERF_REQUIRE(desc->C == 8 || desc->C == 16 || desc->C == 32, "kplanes_gather_bwd_coords: C=%d unsupported (8, 16, 32)", desc->C);
  SNERF_REQUIRE(desc->n_coords == 3 || desc->n_coords == 4, "kplanes_gather_bwd_coords: n_coords=%d unsupported", desc->n_coords);
  SNERF_REQUIRE(N >= 0, "kplanes_gather_bwd_coords: negative N");
  SNERF_REQUIRE_CONTRACT(coords, "kplanes_gather_bwd_coords");
  for (int s = 0; s < desc->n_scales; ++s)
    for (int k = 0; k < desc->n_coords; ++k) SNERF_REQUIRE(desc->res[s][k] >= 1, "kplanes_gather_bwd_coords: res[%d][%d]=%d", s, k, desc->res[s][k]);
  if (coords->mode == 0) {
    SNERF_REQUIRE(coords->pts || N == 0, "kplanes_gather_bwd_coords: pts is null");
    SNERF_REQUIRE(!grad_origins && !grad_dirs, "kplanes_gather_bwd_coords: grad_origins / grad_dirs need coords.mode 1 (rays)");
  } else if (coords->mode == 1) {
    SNERF_REQUIRE(coords->S >= 1 && N % coords->S == 0, "kplanes_gather_bwd_coords: N=%lld not a multiple of S=%d",
                  (long long)N, coords->S);
    SNERF_REQUIRE(ray_coords_complete(coords, desc->n_coords) || N == 0,
                  "kplanes_gather_bwd_coords: null ray buffers (times may be null only with three coordinates)");
  } else {
    SNERF_REQUIRE(false, "kplanes_gather_bwd_coords: coords.mode=%d unsupported", coords->mode);
  }
  SNERF_REQUIRE(grad_pts || grad_origins || grad_dirs, "kplanes_gather_bwd_coords: no output requested");
  if (N == 0) return 0;
  SNERF_REQUIRE(planes && grad_out, "kplanes_gather_bwd_coords: null buffer");
  DISPATCH_C_NP(launch_bwd_coords, desc, planes, coords, N, grad_out, grad_pts, grad_origins, grad_dirs, (hipStream_t)stream);
}
