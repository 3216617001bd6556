// The per-ray arithmetic of a step, each phase defined once: transmittance weights, compositing with the median depth, the MSE backward, the
// distortion loss and the weights backward.  ray_ops.hip (resample_kernel stage 1, weights_bwd_kernel), render_loss.hip (render_fwd_kernel,
// render_bwd_kernel, render_mse_bwd_kernel, distortion_kernel and the one-launch ray_train_kernel) and render_eval.hip (composite_ray) call
// these and hold no per-ray arithmetic of their own, so what they compute is equal bit for bit by construction.
//
// One 64-lane wavefront owns one ray of S <= MAX_S samples.  A phase works on LDS rows that are PRIVATE to the wave (dd, aux, w, ...), on
// `lane` and S, and where it needs them on the ray's own global rows, passed as pointers to the ray's first element.  Lanes of the wave
// exchange values through those rows; the barrier between a phase's steps is the caller's kind, passed as a tag: the four-wave kernels
// use BlockSync, the one-wave tail of the fused renderer WaveSync.  Every phase compiles with FP contraction off (the reference rounds
// every product), whatever its includer's setting.
//
// Reference: NS/cameras/rays.py:127-149 (get_weights), NS/model_components/renderers.py (RGBRenderer :58-140, AccumulationRenderer
// :197-223, DepthRenderer :226-287), NS/model_components/losses.py:125-136 (lossfun_distortion).
#pragma once
#include "common.hpp"

namespace snerf {

constexpr int RAYS_PER_BLOCK = 4;      // one wavefront per ray, 256 threads per workgroup
constexpr int MAX_S = 64 * WSCAN_PER;  // 320: samples per ray that wave_scan_f64 covers, the limit of every per-ray kernel

struct BlockSync { __device__ __forceinline__ static void sync() { __syncthreads(); } };
struct WaveSync { __device__ __forceinline__ static void sync() { wave_lds_publish(); } };

// ---- 1. optical depth and weights (rays.py:127-149) ----
// dd[i] = (eb[i + 1] - eb[i]) * sigma[i] for i < n_sigma and 0 behind it, aux = the exclusive cumsum of dd (double accumulator, as ATen's
// CPU cumsum).  sigma may be dd itself.
template <typename Sync>
__device__ __forceinline__ void ray_optical_depth(const float* eb, const float* sigma, int n_sigma, float* dd, float* aux, int S, int lane) {
#pragma clang fp contract(off)
  for (int i = lane; i < S; i += 64) {
    const float e0 = eb[i], e1 = eb[i + 1];
    dd[i] = (e1 - e0) * (i < n_sigma ? sigma[i] : 0.f);  // delta * sigma
  }
  Sync::sync();
  wave_scan_f64<true, false>(dd, aux, S, lane);
  Sync::sync();
}

// ... and w[i] = nan_to_num((1 - exp(-dd[i])) * exp(-aux[i])), also written to the global row w_out where that is not null.  w may be dd (the
// caller then has no use for dd behind this); dd and aux are left as the backward needs them otherwise.  No barrier behind the last store.
template <typename Sync>
__device__ __forceinline__ void ray_weights(const float* eb, const float* sigma, int n_sigma, float* dd, float* aux, float* w, float* w_out, bool live,
                                            int S, int lane) {
#pragma clang fp contract(off)
  ray_optical_depth<Sync>(eb, sigma, n_sigma, dd, aux, S, lane);
  for (int i = lane; i < S; i += 64) {
    const float alpha = 1.f - expf(-dd[i]);
    const float T = expf(-aux[i]);
    const float wt = nan_to_num(alpha * T);
    w[i] = wt;
    if (w_out && live) w_out[i] = wt;
  }
}

// ---- 2. weighted sums (renderers.py:113, :133-134, :214, :270) ----
struct RaySums {
  float c[3], acc, dsum;  // sum w rgb, sum w, sum w * bin midpoint (0 without DEPTH)
};
// w may be a global row: it is then copied to the LDS row w_copy (null: no copy) for the median scan.  Colours behind n_col count as zero;
// `clean` is the eval-mode nan_to_num on colours; DEPTH = false leaves the depth sum (and eb) out.  Every load of a sample stands in front
// of the first use and of the conditional store, so that the global rows are fetched in one round trip.
template <bool DEPTH>
__device__ __forceinline__ RaySums ray_weighted_sums(const float* w, float* w_copy, const float* col, int n_col, bool clean, const float* eb, int S,
                                                     int lane) {
#pragma clang fp contract(off)
  float cr = 0.f, cg = 0.f, cb = 0.f, acc = 0.f, dsum = 0.f;
  for (int i = lane; i < S; i += 64) {
    const float wi = w[i];
    float x = 0.f, y = 0.f, z = 0.f, e0 = 0.f, e1 = 0.f;
    if (i < n_col) { x = col[i * 3]; y = col[i * 3 + 1]; z = col[i * 3 + 2]; }
    if (DEPTH) { e0 = eb[i]; e1 = eb[i + 1]; }
    if (w_copy) w_copy[i] = wi;
    if (clean) { x = nan_to_num(x); y = nan_to_num(y); z = nan_to_num(z); }
    cr += wi * x; cg += wi * y; cb += wi * z;
    acc += wi;
    if (DEPTH) dsum += wi * ((e0 + e1) / 2.f);
  }
  RaySums s;
  s.c[0] = wave_sum(cr); s.c[1] = wave_sum(cg); s.c[2] = wave_sum(cb); s.acc = wave_sum(acc); s.dsum = DEPTH ? wave_sum(dsum) : 0.f;
  return s;
}

// ---- 3. median index (renderers.py:264-267) ----
// First index with cumsum(w) >= 0.5 (searchsorted left), clamped to S - 1, in every lane; the cumsum goes to the scratch row cum.
template <typename Sync>
__device__ __forceinline__ int ray_median_index(const float* w, float* cum, int S, int lane) {
  wave_scan_f64<false, false>(w, cum, S, lane);
  Sync::sync();
  int idx = S;
  for (int i = lane; i < S; i += 64)
    if (cum[i] >= 0.5f) { idx = i; break; }  // the cumsum of non-negative weights is monotone: the lane's first hit is its smallest
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(idx, off, 64); idx = o < idx ? o : idx; }
  return idx > S - 1 ? S - 1 : idx;
}
__device__ __forceinline__ float bin_midpoint(const float* eb, int i) {
#pragma clang fp contract(off)
  const float e0 = eb[i], e1 = eb[i + 1];
  return (e0 + e1) / 2.f;
}

// ---- 4. background colour and blend (renderers.py:113) ----
// bg_mode 0: row r of bg [R,3]; 2: the one colour bg[3]; 1 ("last_sample"): the colour `last`, cleaned in eval mode -- null in the
// training backwards, which have no such mode: zero.
__device__ __forceinline__ void ray_background(int bg_mode, const float* bg, int64_t r, const float* last, bool clean, float b[3]) {
  b[0] = 0.f; b[1] = 0.f; b[2] = 0.f;
  if (bg_mode == 0) { b[0] = bg[r * 3]; b[1] = bg[r * 3 + 1]; b[2] = bg[r * 3 + 2]; }
  else if (bg_mode == 2) { b[0] = bg[0]; b[1] = bg[1]; b[2] = bg[2]; }
  else if (last) {
    b[0] = last[0]; b[1] = last[1]; b[2] = last[2];
    if (clean) { b[0] = nan_to_num(b[0]); b[1] = nan_to_num(b[1]); b[2] = nan_to_num(b[2]); }
  }
}
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
// out = c + b (1 - acc), clamped in eval mode
__device__ __forceinline__ void ray_blend(const RaySums& s, const float b[3], bool clamp, float out[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float o = s.c[k] + b[k] * (1.f - s.acc);
    out[k] = clamp ? clamp01(o) : o;
  }
}

// ---- 5. render backward per sample: rgb_out = sum_s w_s rgb_s + bg (1 - sum_s w_s) ----
// the MSE image loss in front of it: go = go_scale * (rgb_out - target); returns the ray's squared error
__device__ __forceinline__ float mse_upstream(const float* out, const float* target, float go_scale, float go[3]) {
#pragma clang fp contract(off)
  const float d0 = out[0] - target[0], d1 = out[1] - target[1], d2 = out[2] - target[2];
  go[0] = d0 * go_scale; go[1] = d1 * go_scale; go[2] = d2 * go_scale;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}
// d / d w_s (without the accumulation's share) ...
__device__ __forceinline__ float render_bwd_gw(const float go[3], const float* c, const float b[3]) {
#pragma clang fp contract(off)
  return go[0] * (c[0] - b[0]) + go[1] * (c[1] - b[1]) + go[2] * (c[2] - b[2]);
}
// ... and d / d rgb_s
__device__ __forceinline__ void render_bwd_grgb(const float go[3], float w, float* g) {
  g[0] = go[0] * w; g[1] = go[1] * w; g[2] = go[2] * w;
}

// ---- 6. distortion loss (losses.py:125-136) ----
//   L_r = sum_i w_i sum_j w_j |m_i - m_j| + (1/3) sum_i w_i^2 (t_{i+1} - t_i),  m = bin midpoints
//   dL_r/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i (t_{i+1} - t_i)
// w is the LDS row of weights, m a scratch row for the midpoints of the s-space edges sb.  Returns L_r in every lane; where g is not null
// g[i] (+)= grad_scale * dL_r/dw_i.  The S x S interaction stays in LDS and registers.
template <typename Sync>
__device__ __forceinline__ float ray_distortion(const float* w, float* m, const float* sb, float grad_scale, float* g, bool accumulate, int S, int lane) {
#pragma clang fp contract(off)
  for (int i = lane; i < S; i += 64) {
    const float t0 = sb[i], t1 = sb[i + 1];
    m[i] = (t1 + t0) / 2.f;
  }
  Sync::sync();
  float total = 0.f;
  for (int i = lane; i < S; i += 64) {
    const float wi = w[i], mi = m[i];
    float inner = 0.f;
    for (int j = 0; j < S; ++j) inner += w[j] * fabsf(mi - m[j]);
    const float t0 = sb[i], t1 = sb[i + 1];
    const float dt = t1 - t0;
    total += wi * inner + wi * wi * dt / 3.f;
    if (g) {
      const float gv = (2.f * inner + 2.f * wi * dt / 3.f) * grad_scale;
      if (accumulate) g[i] += gv; else g[i] = gv;
    }
  }
  return wave_sum(total);
}

// ---- 7. weights backward: g_sigma_k = delta_k * ( g_k * T_k * exp(-dd_k) - sum_{i>k} g_i * w_i ) ----
// dd and aux as ray_optical_depth left them (aux becomes the suffix sums), gw = d loss / d weights (LDS or global), eb the ray's edges;
// a live ray's g_sigma goes to the global row gdens (+= with accumulate).  Returns whether a live ray met a value that autograd would have
// turned into a non-finite gradient (the reference's GradScaler then skips the step).
template <typename Sync>
__device__ __forceinline__ bool ray_weights_bwd(const float* dd, float* aux, const float* gw, const float* eb, float* gdens, bool accumulate, bool live,
                                                int S, int lane) {
#pragma clang fp contract(off)
  // gw_i * w_i (0 where the forward weight was non-finite: nan_to_num passes no gradient there)
  float gwterm[WSCAN_PER], Tk[WSCAN_PER], ek[WSCAN_PER];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < WSCAN_PER; ++k) {
    const int i = lane + 64 * k;
    gwterm[k] = 0.f; Tk[k] = 0.f; ek[k] = 0.f;
    if (i < S) {
      const float T = expf(-aux[i]);
      const float e = expf(-dd[i]);
      const float wraw = (1.f - e) * T;
      const float g = gw[i];
      const bool fin = (wraw == wraw) && fabsf(wraw) != INFINITY;
      Tk[k] = T; ek[k] = e;
      gwterm[k] = fin ? g * wraw : 0.f;
      // a non-finite weight (density = exp(x) overflowed to inf on a zero-width bin: 0 * inf) passes no gradient, as nan_to_num
      // does -- and must not leave a NaN factor behind: 0 * NaN is NaN (seen once in ~20 k training steps: one NaN here reaches
      // every parameter through the sigma net and the TV stencil within a few steps)
      if (!fin) { Tk[k] = 0.f; ek[k] = 0.f; bad = bad || live; }
    }
  }
  Sync::sync();
#pragma unroll
  for (int k = 0; k < WSCAN_PER; ++k) {
    const int i = lane + 64 * k;
    if (i < S) aux[i] = gwterm[k];
  }
  Sync::sync();
  wave_scan_f64<true, true>(aux, aux, S, lane);  // suffix sums: aux[i] = sum_{j > i}
  Sync::sync();
#pragma unroll
  for (int k = 0; k < WSCAN_PER; ++k) {
    const int i = lane + 64 * k;
    if (i < S && live) {
      const float g = gw[i];
      const float e0 = eb[i], e1 = eb[i + 1];
      const float gdd = g * Tk[k] * ek[k] - aux[i];
      float out = gdd * (e1 - e0);
      if (!(fabsf(out) <= 3.402823466e+38f)) { out = 0.f; bad = true; }  // inf * 0 / NaN: no gradient
      if (accumulate) gdens[i] += out; else gdens[i] = out;
    }
  }
  return bad;
}

}  // namespace snerf
