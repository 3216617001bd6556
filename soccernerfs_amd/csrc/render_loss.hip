// Per-ray compositing (renderers) and the ray-level losses (distortion, interlevel), forward + backward.
//
// One wavefront per ray, 4 rays per workgroup, per-ray scratch in LDS.
// Reference: NS/model_components/renderers.py (RGBRenderer :58-140, AccumulationRenderer :197-223, DepthRenderer
// :226-287, MedianRGBRenderer :290-362) and NS/model_components/losses.py (outer :46-75, lossfun_outer :78-95,
// interlevel_loss :106-121, lossfun_distortion :125-136).  The reference's distortion loss materialises an
// [R,S,S] tensor (67 MB at the preset); here the S x S interaction stays in LDS/registers.
#include "per_ray_common.hpp"

#pragma clang fp contract(off)

namespace snerf {

// ------------------------------------------------------------------------------------------------
// render forward
// ------------------------------------------------------------------------------------------------
struct RenderArgs {
  const float* weights;  // [R,S]
  const float* rgb;      // [R,S,3]
  const float* ebins;    // [R,S+1]
  const float* bg;       // bg_mode 0: [R,3]; 2: [3]; 1 (last_sample): unused
  int R, S, bg_mode, training;
  float* rgb_out;        // [R,3]
  float* acc_out;        // [R]
  float* depth_median;   // [R] or null
  float* depth_expected; // [R] or null (unclipped: sum(w*steps)/(sum(w)+1e-10))
  float* median_rgb;     // [R,3] or null
  int64_t* median_index; // [R] or null
};

__global__ __launch_bounds__(256) void render_fwd_kernel(RenderArgs a) {
  __shared__ float s_w[RAYS_PER_BLOCK][MAX_S];
  __shared__ float s_cum[RAYS_PER_BLOCK][MAX_S];
  __shared__ int s_med[RAYS_PER_BLOCK];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RAYS_PER_BLOCK + wv;
  const bool live = ray < a.R;
  const int r = live ? ray : a.R - 1;
  const int S = a.S;
  const float* eb = a.ebins + (int64_t)r * (S + 1);
  const float* rgb = a.rgb + (int64_t)r * S * 3;
  const bool eval = !a.training;
  const RaySums s = ray_weighted_sums<true>(a.weights + (int64_t)r * S, s_w[wv], rgb, S, eval, eb, S, lane);
  __syncthreads();
  const int idx = ray_median_index<BlockSync>(s_w[wv], s_cum[wv], S, lane);
  if (lane == 0) s_med[wv] = idx;
  __syncthreads();
  if (lane == 0 && live) {
    float b[3], o[3];
    ray_background(a.bg_mode, a.bg, r, rgb + (S - 1) * 3, eval, b);
    ray_blend(s, b, eval, o);
    a.rgb_out[(int64_t)r * 3] = o[0]; a.rgb_out[(int64_t)r * 3 + 1] = o[1]; a.rgb_out[(int64_t)r * 3 + 2] = o[2];
    a.acc_out[r] = s.acc;
    const int m = s_med[wv];
    if (a.median_index) a.median_index[r] = m;
    if (a.depth_median) a.depth_median[r] = bin_midpoint(eb, m);
    if (a.depth_expected) a.depth_expected[r] = s.dsum / (s.acc + 1e-10f);
    if (a.median_rgb) {
      const float* c = rgb + m * 3;
      float x = c[0], y = c[1], z = c[2];
      if (eval) { x = clamp01(nan_to_num(x)); y = clamp01(nan_to_num(y)); z = clamp01(nan_to_num(z)); }
      a.median_rgb[(int64_t)r * 3] = x; a.median_rgb[(int64_t)r * 3 + 1] = y; a.median_rgb[(int64_t)r * 3 + 2] = z;
    }
  }
}

// render backward (training): rgb_out = sum_s w_s rgb_s + bg (1 - sum_s w_s); acc = sum_s w_s
__global__ void render_bwd_kernel(const float* __restrict__ weights, const float* __restrict__ rgb, const float* __restrict__ bg, int bg_mode,
                                  const float* __restrict__ g_rgb_out, const float* __restrict__ g_acc, int R, int S,
                                  float* __restrict__ g_weights, float* __restrict__ g_rgb, int accumulate_w) {
  int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)R * S) return;
  int r = (int)(gid / S);
  const float go[3] = {g_rgb_out[(int64_t)r * 3], g_rgb_out[(int64_t)r * 3 + 1], g_rgb_out[(int64_t)r * 3 + 2]};
  float b[3];
  ray_background(bg_mode, bg, r, nullptr, false, b);
  float gw = render_bwd_gw(go, rgb + gid * 3, b);
  if (g_acc) gw += g_acc[r];
  if (accumulate_w) g_weights[gid] += gw; else g_weights[gid] = gw;
  if (g_rgb) render_bwd_grgb(go, weights[gid], g_rgb + gid * 3);
}

// render backward with the MSE image loss folded in: g_rgb_out = go_scale * (rgb_out - target) is formed per lane instead of by four
// elementwise launches (sub, square-mean, scale); sqerr_rays[r] = sum_c (rgb_out - target)^2 for the (lazy) loss value
__global__ void render_mse_bwd_kernel(const float* __restrict__ weights, const float* __restrict__ rgb, const float* __restrict__ bg, int bg_mode,
                                      const float* __restrict__ rgb_out, const float* __restrict__ target, float go_scale, int R, int S,
                                      float* __restrict__ g_weights, float* __restrict__ g_rgb, float* __restrict__ sqerr_rays) {
  int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)R * S) return;
  int r = (int)(gid / S);
  float go[3], b[3];
  const float sqerr = mse_upstream(rgb_out + (int64_t)r * 3, target + (int64_t)r * 3, go_scale, go);
  if (sqerr_rays && gid == (int64_t)r * S) sqerr_rays[r] = sqerr;
  ray_background(bg_mode, bg, r, nullptr, false, b);
  g_weights[gid] = render_bwd_gw(go, rgb + gid * 3, b);
  if (g_rgb) render_bwd_grgb(go, weights[gid], g_rgb + gid * 3);
}

// ------------------------------------------------------------------------------------------------
// distortion loss (per-ray value + gradient w.r.t. weights)
//   L_r = sum_i w_i sum_j w_j |m_i - m_j| + (1/3) sum_i w_i^2 (t_{i+1} - t_i),  m = bin midpoints
//   dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i (t_{i+1} - t_i)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void distortion_kernel(const float* __restrict__ weights, const float* __restrict__ sbins, int R, int S,
                                                        float grad_scale, float* __restrict__ loss_rays, float* __restrict__ g_weights,
                                                        int accumulate) {
  __shared__ float s_w[RAYS_PER_BLOCK][MAX_S];
  __shared__ float s_m[RAYS_PER_BLOCK][MAX_S];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RAYS_PER_BLOCK + wv;
  const bool live = ray < R;
  const int r = live ? ray : R - 1;
  for (int i = lane; i < S; i += 64) s_w[wv][i] = weights[(int64_t)r * S + i];
  const float total = ray_distortion<BlockSync>(s_w[wv], s_m[wv], sbins + (int64_t)r * (S + 1), grad_scale,
                                                g_weights && live ? g_weights + (int64_t)r * S : nullptr, accumulate != 0, S, lane);
  if (lane == 0 && live && loss_rays) loss_rays[r] = total;
}

// ------------------------------------------------------------------------------------------------
// interlevel (proposal) loss for ONE proposal level against the (detached) nerf level:
//   w_outer_i = cy[hi_i + 1] - cy[lo_i],  cy = [0, cumsum(wp)]
//   lo_i = clamp(searchsorted(tp[:-1], c_i, right) - 1, 0, Sp-1),  hi_i = clamp(searchsorted(tp[1:], c_{i+1}, right), 0, Sp-1)
//   loss_i = max(w_i - w_outer_i, 0)^2 / (w_i + 1e-7)
// outputs per-ray sum of loss_i and d(sum)/d wp (scaled by grad_scale)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void interlevel_kernel(const float* __restrict__ c_bins, const float* __restrict__ w_nerf, int S,
                                                        const float* __restrict__ p_bins, const float* __restrict__ w_prop, int Sp, int R,
                                                        float grad_scale, float* __restrict__ loss_rays, float* __restrict__ g_wprop) {
  __shared__ float s_tp[RAYS_PER_BLOCK][MAX_S + 1];
  __shared__ float s_cy[RAYS_PER_BLOCK][MAX_S + 1];
  __shared__ float s_g[RAYS_PER_BLOCK][MAX_S];
  __shared__ int s_lo[RAYS_PER_BLOCK][MAX_S];
  __shared__ int s_hi[RAYS_PER_BLOCK][MAX_S];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RAYS_PER_BLOCK + wv;
  const bool live = ray < R;
  const int r = live ? ray : R - 1;
  float* tp = s_tp[wv];
  float* cy = s_cy[wv];
  for (int i = lane; i <= Sp; i += 64) tp[i] = p_bins[(int64_t)r * (Sp + 1) + i];
  for (int i = lane; i < Sp; i += 64) cy[i + 1] = w_prop[(int64_t)r * Sp + i];
  __syncthreads();
  wave_scan_f64<false, false>(cy + 1, cy + 1, Sp, lane);  // cy = [0, cumsum(wp)], double accumulator
  if (lane == 0) cy[0] = 0.f;
  __syncthreads();
  float total = 0.f;
  for (int i = lane; i < S; i += 64) {
    const float c0 = c_bins[(int64_t)r * (S + 1) + i], c1 = c_bins[(int64_t)r * (S + 1) + i + 1];
    // searchsorted(tp[0..Sp-1], c0, right)
    int lo = 0, hi = Sp;
    while (lo < hi) { int mid = (lo + hi) >> 1; if (tp[mid] <= c0) lo = mid + 1; else hi = mid; }
    int ilo = lo - 1; ilo = ilo < 0 ? 0 : (ilo > Sp - 1 ? Sp - 1 : ilo);
    // searchsorted(tp[1..Sp], c1, right)
    lo = 0; hi = Sp;
    while (lo < hi) { int mid = (lo + hi) >> 1; if (tp[mid + 1] <= c1) lo = mid + 1; else hi = mid; }
    int ihi = lo; ihi = ihi < 0 ? 0 : (ihi > Sp - 1 ? Sp - 1 : ihi);
    const float wo = cy[ihi + 1] - cy[ilo];
    const float w = w_nerf[(int64_t)r * S + i];
    const float d = fmaxf(w - wo, 0.f);
    total += d * d / (w + 1.0e-7f);
    s_lo[wv][i] = ilo; s_hi[wv][i] = ihi;
    s_g[wv][i] = -2.f * d / (w + 1.0e-7f);  // d loss_i / d w_outer_i (0 when clipped)
  }
  total = wave_sum(total);
  if (lane == 0 && live && loss_rays) loss_rays[r] = total;
  __syncthreads();
  if (g_wprop) {
    // d loss / d w_prop[j] = sum of g_i over the nerf intervals whose envelope [lo_i, hi_i] holds j.  Both bounds are searchsorted results of
    // ascending queries, i.e. non-decreasing in i, so those intervals are ONE contiguous range [a_j, b_j]: a_j = first i with hi_i >= j,
    // b_j = last i with lo_i <= j (two binary searches), summed in ascending i -- the order (and therefore the bits) of the dense
    // "for every i: if (lo_i <= j <= hi_i)" loop this replaces, in O(S + Sp) instead of O(S Sp) LDS reads per ray.
    const int* slo = s_lo[wv];
    const int* shi = s_hi[wv];
    for (int j = lane; j < Sp; j += 64) {
      int a = 0, e = S;
      while (a < e) { const int mid = (a + e) >> 1; if (shi[mid] < j) a = mid + 1; else e = mid; }   // a = first i with hi_i >= j
      int b = 0;
      e = S;
      while (b < e) { const int mid = (b + e) >> 1; if (slo[mid] <= j) b = mid + 1; else e = mid; }  // b = first i with lo_i > j
      float acc = 0.f;
      for (int i = a; i < b; ++i) acc += s_g[wv][i];
      if (live) g_wprop[(int64_t)r * Sp + j] = acc * grad_scale;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// ds_nerf_depth_loss (losses.py:213-235) behind depth_loss (:261-311, DS_NERF branch) for one sampling level:
//   loss_r = [D_r > 0] * sum_s -log(w_s + 1e-7) * exp(-(t_s - D_r)^2 / (2 sigma)) * (e_{s+1} - e_s),  t_s = (e_s + e_{s+1}) / 2,
//   D_r = termination depth (x directions_norm when the depth maps hold z-distances), mean over rays by the caller's grad_scale.
// One wavefront per ray; g_weights (+)= grad_scale * d loss_r / d w.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_loss_kernel(const float* __restrict__ weights, const float* __restrict__ ebins, const float* __restrict__ term,
                                                        const float* __restrict__ dir_norm, float sigma, int R, int S, float grad_scale,
                                                        float* __restrict__ loss_rays, float* __restrict__ g_weights, int accumulate) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RAYS_PER_BLOCK + wv;
  if (ray >= R) return;
  float D = term[ray];
  if (dir_norm) D = D * dir_norm[ray];
  const bool on = D > 0.f;
  float total = 0.f;
  for (int i = lane; i < S; i += 64) {
    const float e0 = ebins[(int64_t)ray * (S + 1) + i], e1 = ebins[(int64_t)ray * (S + 1) + i + 1];
    const float w = weights[(int64_t)ray * S + i];
    const float t = (e0 + e1) / 2.f;
    const float k = expf(-((t - D) * (t - D)) / (2.f * sigma)) * (e1 - e0);
    total += -logf(w + 1.0e-7f) * k;
    if (g_weights) {
      const float g = on ? grad_scale * (-k / (w + 1.0e-7f)) : 0.f;
      if (accumulate) g_weights[(int64_t)ray * S + i] += g; else g_weights[(int64_t)ray * S + i] = g;
    }
  }
  total = wave_sum(total);
  if (lane == 0 && loss_rays) loss_rays[ray] = on ? total : 0.f;
}

// ------------------------------------------------------------------------------------------------
// urban_radiance_field_depth_loss (losses.py:238-274) behind depth_loss (:261-311, URF branch) for one sampling level, D as above:
//   loss_r = [D_r > 0] * ( (D_r - d_r)^2                                          d_r = the level's predicted depth
//                        + sum_{|t_s - D_r| <= sigma} (w_s - N(t_s - D_r; 0, sigma / 3))^2   "line of sight", near the surface
//                        + sum_{t_s < D_r - sigma} w_s^2 )                                   ... and in front of it
// with N the normal density (torch.distributions.Normal.log_prob, exponentiated).  g_weights (+)= grad_scale * d loss_r / d w,
// g_pred (may be NULL) = grad_scale * d loss_r / d d_r.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void urf_depth_loss_kernel(const float* __restrict__ weights, const float* __restrict__ ebins, const float* __restrict__ term,
                                                            const float* __restrict__ dir_norm, const float* __restrict__ pred, float sigma, int R, int S,
                                                            float grad_scale, float* __restrict__ loss_rays, float* __restrict__ g_weights,
                                                            float* __restrict__ g_pred, int accumulate) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RAYS_PER_BLOCK + wv;
  if (ray >= R) return;
  float D = term[ray];
  if (dir_norm) D = D * dir_norm[ray];
  const bool on = D > 0.f;
  const float sd = sigma / 3.0f;  // URF_SIGMA_SCALE_FACTOR (losses.py:36)
  const float log_norm = -logf(sd) - 0.918938533204672742f;  // - log(sd) - log(sqrt(2 pi))
  float total = 0.f;
  for (int i = lane; i < S; i += 64) {
    const float e0 = ebins[(int64_t)ray * (S + 1) + i], e1 = ebins[(int64_t)ray * (S + 1) + i + 1];
    const float w = weights[(int64_t)ray * S + i];
    const float t = (e0 + e1) / 2.f;
    const float x = t - D;
    float term_i = 0.f, g = 0.f;
    if (t <= D + sigma && t >= D - sigma) {
      const float pdf = expf(-(x * x) / (2.f * sd * sd) + log_norm);
      term_i = (w - pdf) * (w - pdf);
      g = 2.f * (w - pdf);
    } else if (t < D - sigma) {
      term_i = w * w;
      g = 2.f * w;
    }
    total += term_i;
    if (g_weights) {
      const float gv = on ? grad_scale * g : 0.f;
      if (accumulate) g_weights[(int64_t)ray * S + i] += gv; else g_weights[(int64_t)ray * S + i] = gv;
    }
  }
  total = wave_sum(total);
  if (lane == 0) {
    const float d = pred[ray];
    if (loss_rays) loss_rays[ray] = on ? total + (D - d) * (D - d) : 0.f;
    if (g_pred) g_pred[ray] = on ? grad_scale * -2.f * (D - d) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// One launch for the nerf level's per-ray work of a TRAINING step: get_weights -> RGB / accumulation / median depth -> MSE backward ->
// distortion loss + gradient -> get_weights backward: the phases of per_ray_common.hpp that resample_kernel stage 1, render_fwd_kernel,
// render_mse_bwd_kernel, distortion_kernel and weights_bwd_kernel run one by one (equal bits by construction; tests/test_gpu_render_loss.py
// holds them to it).  On the step's critical path those five cost ~0.1 ms of launches and barriers for ~20 us of work.
// ------------------------------------------------------------------------------------------------
struct RayTrainArgs {
  const float* density; const float* ebins; const float* sbins; const float* rgb; const float* bg; const float* target;
  int R, S, bg_mode;
  float go_scale, dist_scale;
  float* weights; float* rgb_out; float* acc_out; float* depth_median; float* sqerr_rays; float* dist_rays;
  float* g_rgb; float* g_density; float* g_weights; int32_t* nonfinite_flag;
};

__global__ __launch_bounds__(256) void ray_train_kernel(RayTrainArgs a) {
  __shared__ float s_dd[RAYS_PER_BLOCK][MAX_S + 1];   // delta * sigma
  __shared__ float s_aux[RAYS_PER_BLOCK][MAX_S + 1];  // exclusive cumsum of it; later the suffix sums of the backward
  __shared__ float s_w[RAYS_PER_BLOCK][MAX_S + 1];    // weights
  __shared__ float s_m[RAYS_PER_BLOCK][MAX_S + 1];    // cumsum of w (median), then the s-space bin midpoints
  __shared__ float s_g[RAYS_PER_BLOCK][MAX_S + 1];    // d loss / d weights
  // the wave index as a scalar: the ray's row pointers that the phases take then live in SGPRs, not in VGPR pairs beside the 15 floats the
  // weights backward stages across its scan (80 VGPRs is the last count at which six waves per SIMD fit)
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ray = blockIdx.x * RAYS_PER_BLOCK + wv;
  const bool live = ray < a.R;
  const int r = live ? ray : a.R - 1;
  const int S = a.S;
  float *dd = s_dd[wv], *aux = s_aux[wv], *w = s_w[wv], *mm = s_m[wv], *gw = s_g[wv];
  const float* eb = a.ebins + (int64_t)r * (S + 1);

  // ---- get_weights; dd and aux stay for the backward ----
  ray_weights<BlockSync>(eb, a.density + (int64_t)r * S, S, dd, aux, w, a.weights + (int64_t)r * S, live, S, lane);
  __syncthreads();

  // ---- render forward, training mode ----
  const float* rgb = a.rgb + (int64_t)r * S * 3;
  const RaySums s = ray_weighted_sums<false>(w, nullptr, rgb, S, false, nullptr, S, lane);
  if (a.depth_median) {
    const int idx = ray_median_index<BlockSync>(w, mm, S, lane);
    if (lane == 0 && live) a.depth_median[r] = bin_midpoint(eb, idx);
    __syncthreads();
  }
  float b[3], o[3], go[3];
  ray_background(a.bg_mode, a.bg, r, nullptr, false, b);
  ray_blend(s, b, false, o);
  if (lane == 0 && live) {
    a.rgb_out[(int64_t)r * 3] = o[0]; a.rgb_out[(int64_t)r * 3 + 1] = o[1]; a.rgb_out[(int64_t)r * 3 + 2] = o[2];
    a.acc_out[r] = s.acc;
  }

  // ---- MSE folded into the render backward ----
  const float sqerr = mse_upstream(o, a.target + (int64_t)r * 3, a.go_scale, go);
  if (lane == 0 && live && a.sqerr_rays) a.sqerr_rays[r] = sqerr;
  for (int i = lane; i < S; i += 64) {
    gw[i] = render_bwd_gw(go, rgb + i * 3, b);
    if (live) render_bwd_grgb(go, w[i], a.g_rgb + ((int64_t)r * S + i) * 3);
  }

  // ---- distortion loss and its gradient, added to gw ----
  const float total = ray_distortion<BlockSync>(w, mm, a.sbins + (int64_t)r * (S + 1), a.dist_scale, gw, true, S, lane);
  if (lane == 0 && live && a.dist_rays) a.dist_rays[r] = total;
  if (a.g_weights && live)
    for (int i = lane; i < S; i += 64) a.g_weights[(int64_t)r * S + i] = gw[i];

  // ---- get_weights backward ----
  const bool bad = ray_weights_bwd<BlockSync>(dd, aux, gw, eb, a.g_density + (int64_t)r * S, false, live, S, lane);
  if (bad && a.nonfinite_flag) *a.nonfinite_flag = 1;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_depth_loss(const float* weights, const float* ebins, const float* termination_depth, const float* directions_norm, float sigma,
                                int32_t R, int32_t S, float grad_scale, float* loss_rays, float* g_weights, int32_t accumulate, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && S >= 1 && S <= MAX_S && sigma > 0.f, "depth_loss: R=%d S=%d sigma=%g", R, S, (double)sigma);
  if (R == 0) return 0;
  SNERF_REQUIRE(weights && ebins && termination_depth, "depth_loss: null buffer");
  hipLaunchKernelGGL(depth_loss_kernel, dim3(ceil_div(R, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, weights, ebins, termination_depth, directions_norm, sigma,
                     R, S, grad_scale, loss_rays, g_weights, accumulate);
  SNERF_LAUNCH_CHECK("depth_loss");
  return 0;
}

extern "C" int snerf_urf_depth_loss(const float* weights, const float* ebins, const float* termination_depth, const float* directions_norm,
                                    const float* predicted_depth, float sigma, int32_t R, int32_t S, float grad_scale, float* loss_rays, float* g_weights,
                                    float* g_predicted_depth, int32_t accumulate, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && S >= 1 && S <= MAX_S && sigma > 0.f, "urf_depth_loss: R=%d S=%d sigma=%g", R, S, (double)sigma);
  if (R == 0) return 0;
  SNERF_REQUIRE(weights && ebins && termination_depth && predicted_depth, "urf_depth_loss: null buffer");
  hipLaunchKernelGGL(urf_depth_loss_kernel, dim3(ceil_div(R, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, weights, ebins, termination_depth, directions_norm,
                     predicted_depth, sigma, R, S, grad_scale, loss_rays, g_weights, g_predicted_depth, accumulate);
  SNERF_LAUNCH_CHECK("urf_depth_loss");
  return 0;
}

extern "C" int snerf_render_fwd(const snerf_render_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "render_fwd: null args");
  SNERF_REQUIRE(p->R >= 0 && p->S >= 1 && p->S <= MAX_S, "render_fwd: R=%d S=%d (S <= %d)", p->R, p->S, MAX_S);
  SNERF_REQUIRE(p->bg_mode >= 0 && p->bg_mode <= 2, "render_fwd: bg_mode=%d", p->bg_mode);
  if (p->R == 0) return 0;
  SNERF_REQUIRE(p->weights && p->rgb && p->ebins && p->rgb_out && p->acc_out, "render_fwd: null buffer");
  SNERF_REQUIRE(p->bg_mode == 1 || p->bg, "render_fwd: background buffer is null");
  RenderArgs a;
  a.weights = p->weights; a.rgb = p->rgb; a.ebins = p->ebins; a.bg = p->bg; a.R = p->R; a.S = p->S; a.bg_mode = p->bg_mode;
  a.training = p->training; a.rgb_out = p->rgb_out; a.acc_out = p->acc_out; a.depth_median = p->depth_median;
  a.depth_expected = p->depth_expected; a.median_rgb = p->median_rgb; a.median_index = p->median_index;
  hipLaunchKernelGGL(render_fwd_kernel, dim3(ceil_div(p->R, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, a);
  SNERF_LAUNCH_CHECK("render_fwd");
  return 0;
}

extern "C" int snerf_render_bwd(const float* weights, const float* rgb, const float* bg, int32_t bg_mode, const float* g_rgb_out,
                                const float* g_acc, int32_t R, int32_t S, float* g_weights, float* g_rgb, int32_t accumulate_w,
                                snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && S >= 1, "render_bwd: R=%d S=%d", R, S);
  SNERF_REQUIRE(bg_mode == 0 || bg_mode == 2, "render_bwd: bg_mode=%d has no training backward", bg_mode);
  if (R == 0) return 0;
  SNERF_REQUIRE(weights && rgb && bg && g_rgb_out && g_weights, "render_bwd: null buffer");
  hipLaunchKernelGGL(render_bwd_kernel, dim3(ceil_div((int64_t)R * S, 256)), dim3(256), 0, (hipStream_t)stream, weights, rgb, bg, bg_mode,
                     g_rgb_out, g_acc, R, S, g_weights, g_rgb, accumulate_w);
  SNERF_LAUNCH_CHECK("render_bwd");
  return 0;
}

extern "C" int snerf_render_mse_bwd(const float* weights, const float* rgb, const float* bg, int32_t bg_mode, const float* rgb_out,
                                    const float* target, float go_scale, int32_t R, int32_t S, float* g_weights, float* g_rgb, float* sqerr_rays,
                                    snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && S >= 1, "render_mse_bwd: R=%d S=%d", R, S);
  SNERF_REQUIRE(bg_mode == 0 || bg_mode == 2, "render_mse_bwd: bg_mode %d has no training backward", bg_mode);
  if (R == 0) return 0;
  SNERF_REQUIRE(weights && rgb && bg && rgb_out && target && g_weights, "render_mse_bwd: null buffer");
  hipLaunchKernelGGL(render_mse_bwd_kernel, dim3(ceil_div((int64_t)R * S, 256)), dim3(256), 0, (hipStream_t)stream, weights, rgb, bg, bg_mode,
                     rgb_out, target, go_scale, R, S, g_weights, g_rgb, sqerr_rays);
  SNERF_LAUNCH_CHECK("render_mse_bwd");
  return 0;
}

extern "C" int snerf_distortion(const float* weights, const float* sbins, int32_t R, int32_t S, float grad_scale, float* loss_rays,
                                float* g_weights, int32_t accumulate, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && S >= 1 && S <= MAX_S, "distortion: R=%d S=%d (S <= %d)", R, S, MAX_S);
  if (R == 0) return 0;
  SNERF_REQUIRE(weights && sbins, "distortion: null buffer");
  hipLaunchKernelGGL(distortion_kernel, dim3(ceil_div(R, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, weights, sbins, R, S, grad_scale, loss_rays,
                     g_weights, accumulate);
  SNERF_LAUNCH_CHECK("distortion");
  return 0;
}

extern "C" int snerf_interlevel(const float* c_bins, const float* w_nerf, int32_t S, const float* p_bins, const float* w_prop, int32_t Sp,
                                int32_t R, float grad_scale, float* loss_rays, float* g_wprop, snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && S >= 1 && S <= MAX_S && Sp >= 1 && Sp <= MAX_S, "interlevel: R=%d S=%d Sp=%d", R, S, Sp);
  if (R == 0) return 0;
  SNERF_REQUIRE(c_bins && w_nerf && p_bins && w_prop, "interlevel: null buffer");
  hipLaunchKernelGGL(interlevel_kernel, dim3(ceil_div(R, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, c_bins, w_nerf, S, p_bins, w_prop, Sp, R,
                     grad_scale, loss_rays, g_wprop);
  SNERF_LAUNCH_CHECK("interlevel");
  return 0;
}

extern "C" int snerf_ray_train_fwd_bwd(const snerf_ray_train_args* p, snerf_stream_t stream) {
  SNERF_REQUIRE(p, "ray_train_fwd_bwd: null args");
  SNERF_REQUIRE(p->R >= 0 && p->S >= 1 && p->S <= MAX_S, "ray_train_fwd_bwd: R=%d S=%d (S <= %d)", p->R, p->S, MAX_S);
  SNERF_REQUIRE(p->bg_mode == 0 || p->bg_mode == 2, "ray_train_fwd_bwd: bg_mode %d has no training backward", p->bg_mode);
  if (p->R == 0) return 0;
  SNERF_REQUIRE(p->density && p->ebins && p->sbins && p->rgb && p->bg && p->target && p->weights && p->rgb_out && p->acc_out && p->g_rgb && p->g_density,
                "ray_train_fwd_bwd: null buffer");
  RayTrainArgs a = {};
  a.density = p->density; a.ebins = p->ebins; a.sbins = p->sbins; a.rgb = p->rgb; a.bg = p->bg; a.target = p->target;
  a.R = p->R; a.S = p->S; a.bg_mode = p->bg_mode; a.go_scale = p->go_scale; a.dist_scale = p->dist_scale;
  a.weights = p->weights; a.rgb_out = p->rgb_out; a.acc_out = p->acc_out; a.depth_median = p->depth_median; a.sqerr_rays = p->sqerr_rays;
  a.dist_rays = p->dist_rays; a.g_rgb = p->g_rgb; a.g_density = p->g_density; a.g_weights = p->g_weights; a.nonfinite_flag = p->nonfinite_flag;
  hipLaunchKernelGGL(ray_train_kernel, dim3(ceil_div(p->R, RAYS_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, a);
  SNERF_LAUNCH_CHECK("ray_train_fwd_bwd");
  return 0;
}
