// Fused K-Planes field forward: plane gather -> sigma_net -> trunc_exp density, colour net -> rgb in ONE kernel.
// (A fused backward -- recomputed forward -> both nets' backward -> per-plane gradient vectors -- was built and parity-tested in round 2 and
// removed in round 3: 256 VGPRs + spills, 2.5 ms against 0.85 ms for the three unfused kernels, and with the quotient form of the scatter
// it would have saved only ~0.4 GB of the backward's traffic.  DESIGN.md section 4.2.)
//
// Replaces KPlanesField.get_density + get_outputs (NS/fields/kplanes_field.py:275-358): interpolate_kplanes (:77-126), sigma_net
// (:249-261: features 32 n_scales -> 128 -> 16), trunc_exp on the last output (:308-311), color_net on the 15 geometry features
// (:263-273 with disable_viewing_dependent: 15 -> 64 -> 64 -> 3, Sigmoid).  In the unfused path feat[N,160], h[N,16], gh[N,16] and
// gfeat[N,160] cross HBM between five launches; here a tile of 32 samples lives in LDS from the texel reads to density / rgb.  Only what
// other kernels need touches HBM: density [N], rgb [N,3] (compositing) and, for a training step, what the unfused backward kernels read:
// the operand-typed feature tile, the 16 sigma_net outputs, and the fp32 features (the quotient scatter's numerator).
//
// 16-bit MFMA operands with fp32 accumulation (v_mfma_f32_16x16x32_bf16 / _f16), the arithmetic of mlp_lp.hip: the fused kernels give
// bit-identical density / rgb / weight gradients to the unfused 16-bit kernels fed the same planes (tests/test_gpu_field_fused.py).
// The exact-fp32 parity path stays unfused (mlp.hip).
//
// The tile itself (work decomposition, LDS plan, gather / sigma_net / colour-net phases) lives in field_fused_common.hpp, shared with the
// render kernel of render_eval.hip.
#include "field_fused_common.hpp"

namespace snerf {

// field_fwd_kernel itself is defined in field_fused_common.hpp (a template over the plane count as well: field_fused_static.hip builds NP = 3).

// field_fwd_ordered_kernel, the same tiles walked in the order of a ray permutation, is defined there as well.

int validate_field(const snerf_kplanes_desc* d, const snerf_coords* c, int64_t N, const snerf_mlp_desc* sd, const snerf_mlp_desc* cd,
                   int max_scales) {
  SNERF_REQUIRE(d && c && sd && cd, "kplanes_field: null descriptor");
  SNERF_REQUIRE(d->C == 32 && (d->n_coords == 4 || d->n_coords == 3) && d->concat == 1 && d->n_scales >= 1 && d->n_scales <= max_scales,
                "kplanes_field: the fused kernels are built for six or three planes per scale (4 / 3 coordinates), C = 32, concatenated scales (<= %d); "
                "got C=%d coords=%d concat=%d scales=%d",
                max_scales, d->C, d->n_coords, d->concat, d->n_scales);
  SNERF_REQUIRE(sd->d_in == 32 * d->n_scales && sd->hidden == FF_H && sd->n_hidden == 1 && sd->d_out == 16 && sd->hidden_act == 1 && sd->out_act == 0,
                "kplanes_field: sigma_net must be %d -> 128 (ReLU) -> 16", 32 * d->n_scales);
  SNERF_REQUIRE((cd->d_in == FF_GEO || cd->d_in == 16 + FF_GEO) && cd->hidden == FF_HC && cd->n_hidden == 2 && cd->d_out == 3 && cd->hidden_act == 1 &&
                cd->out_act == 1, "kplanes_field: color_net must be 15 -> 64 -> 64 (ReLU) -> 3 (Sigmoid), or 31 -> 64 -> 64 -> 3 (view-dependent)");
  SNERF_REQUIRE((sd->operands == 1 || sd->operands == 2) && cd->operands == sd->operands,
                "kplanes_field: the fused kernels compute with bf16 / fp16 MFMA operands (operands = 1 / 2, both nets alike); fp32 runs unfused");
  SNERF_REQUIRE(N >= 0 && N < (1LL << 31), "kplanes_field: N=%lld", (long long)N);
  SNERF_REQUIRE(c->mode == 0 || c->mode == 1, "kplanes_field: coords.mode=%d", c->mode);
  SNERF_REQUIRE_CONTRACT(c, "kplanes_field");
  if (c->mode == 1) SNERF_REQUIRE(c->S >= 1 && N % c->S == 0, "kplanes_field: N=%lld not a multiple of S=%d", (long long)N, c->S);
  if (cd->d_in != FF_GEO && N > 0) SNERF_REQUIRE(c->mode == 1, "kplanes_field: the view-dependent colour net reads per-ray directions (coords.mode = 1)");
  // the kernels dereference these: a static scene (three coordinates) has no times, every other ray buffer and a 4-coordinate descriptor's times must be there
  if (N > 0)
    SNERF_REQUIRE(c->mode == 0 ? c->pts != nullptr : ray_coords_complete(c, d->n_coords),
                  "kplanes_field: incomplete coordinates (pts in mode 0; origins / dirs / ebins and, with four coordinates, times in mode 1)");
  return 0;
}

template <typename T, int NS, int KEEP, bool VD>
static int launch_field_fwd_k(const FieldArgs& a, const int32_t* ray_order, hipStream_t st) {
  using P = PlanFF<NS>;
  const int64_t n_tiles = (a.N + FF_TS - 1) / FF_TS;
  int64_t grid = field_fwd_grid<NS>(n_tiles);
  if (ray_order) {
    auto k = field_fwd_ordered_kernel<T, NS, KEEP, VD>;
    SNERF_ALLOW_LDS(k, LDS_LIMIT);
    if (grid >= 8) grid &= ~(int64_t)7;  // whole eights: one member count for the eight groups of the kernel's walk
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FF_NW * 64), P::BYTES, st, a, (uint32_t)n_tiles, ray_order, (uint32_t)(a.c.S / FF_TS));
  } else {
    auto k = field_fwd_kernel<T, NS, KEEP, VD, 6>;
    SNERF_ALLOW_LDS(k, LDS_LIMIT);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FF_NW * 64), P::BYTES, st, a, n_tiles);
  }
  SNERF_LAUNCH_CHECK("kplanes_field_fwd");
  return 0;
}
template <typename T, int NS, bool VD>
static int launch_field_fwd_vd(const FieldArgs& a, const int32_t* ray_order, hipStream_t st) {
  if (a.feat16 && a.feat32) return launch_field_fwd_k<T, NS, 2, VD>(a, ray_order, st);
  if (a.feat16) return launch_field_fwd_k<T, NS, 1, VD>(a, ray_order, st);
  return launch_field_fwd_k<T, NS, 0, VD>(a, ray_order, st);
}
template <typename T, int NS>
static int launch_field_fwd(const FieldArgs& a, const int32_t* ray_order, hipStream_t st, bool vd) {
  return vd ? launch_field_fwd_vd<T, NS, true>(a, ray_order, st) : launch_field_fwd_vd<T, NS, false>(a, ray_order, st);
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_kplanes_field_fwd_supported(const snerf_kplanes_desc* desc, const snerf_mlp_desc* sigma, const snerf_mlp_desc* color) {
  snerf_coords c = {};
  c.mode = 1;  // a shape probe: the view-dependent colour net needs per-ray coordinates, which a call then has to pass
  c.S = 1;
  return desc && sigma && color && validate_field(desc, &c, 0, sigma, color, 6) == 0 ? 1 : 0;
}

extern "C" int snerf_kplanes_field_fwd_ordered(const snerf_kplanes_desc* desc, const float* planes, const snerf_coords* coords, int64_t N,
                                               const snerf_mlp_desc* sigma, const float* W_sigma, const snerf_mlp_desc* color, const float* W_color,
                                               float* density, float* rgb, void* feat16, float* h, float* feat32, const int32_t* ray_order,
                                               snerf_stream_t stream) {
  int rc = validate_field(desc, coords, N, sigma, color, 6);
  if (rc) return rc;
  if (ray_order)
    SNERF_REQUIRE(coords->mode == 1 && coords->S % FF_TS == 0,
                  "kplanes_field_fwd_ordered: a ray order needs per-ray coordinates (coords.mode = 1) and S a multiple of %d; got mode=%d S=%d", FF_TS,
                  coords->mode, coords->S);
  if (ray_order)  // the frame-time walk exists for the time planes' rows
    SNERF_REQUIRE(desc->n_coords == 4, "kplanes_field_fwd_ordered: a ray order needs a 4-coordinate descriptor; got coords=%d", desc->n_coords);
  if (N == 0) return 0;
  SNERF_REQUIRE(planes && W_sigma && W_color && density && rgb, "kplanes_field_fwd: null buffer");
  FieldArgs a = {};
  a.d = *desc; a.planes = planes; a.c = *coords; a.N = N; a.Wsig = W_sigma; a.Wcol = W_color; a.dens = density; a.rgb = rgb;
  SNERF_REQUIRE((feat16 != nullptr) == (h != nullptr) && (!feat32 || feat16),
                "kplanes_field_fwd: the training outputs come as a set: feat16 and h together, feat32 only with them");
  a.feat16 = feat16; a.h = h; a.feat32 = feat32;
  if (coords->contract) return launch_field_fwd_contract(a, sigma->operands, ray_order, (hipStream_t)stream, color->d_in != FF_GEO);
  if (desc->n_coords == 3) return launch_field_fwd_static(a, sigma->operands, (hipStream_t)stream, color->d_in != FF_GEO);
  FF_DISPATCH_FWD(launch_field_fwd, sigma->operands, desc->n_scales, a, ray_order, (hipStream_t)stream, color->d_in != FF_GEO);
}

extern "C" int snerf_kplanes_field_fwd(const snerf_kplanes_desc* desc, const float* planes, const snerf_coords* coords, int64_t N,
                                       const snerf_mlp_desc* sigma, const float* W_sigma, const snerf_mlp_desc* color, const float* W_color,
                                       float* density, float* rgb, void* feat16, float* h, float* feat32, snerf_stream_t stream) {
  return snerf_kplanes_field_fwd_ordered(desc, planes, coords, N, sigma, W_sigma, color, W_color, density, rgb, feat16, h, feat32, nullptr, stream);
}
