// View-dependent colour input of the K-Planes field (KPlanesField with disable_viewing_dependent = False; NS/fields/kplanes_field.py:39-44
// get_normalized_directions, :206-216 the SH encoder, :260-262 in_dim_color = 16 + 15, :314-323 get_outputs): per sample
//   X = [ SH degree 4 of its ray's direction (16) | geometry features h[:, :15] (15) | 0 ]                      [N, 32] fp32
// for the generic MLP kernels (the exact-fp32 path, the unfused forward, deterministic mode), and the slice of their gX back into gh.  The 16-bit
// training path does not build X at all: the fused field forward (field_fused.hip) and the colour backward (mlp_rows.hip, snerf_kplanes_color_bwd_vd)
// form it on chip from the same per-ray directions.  The SH columns are sh4_common.hpp's, bit-identical to soccernerfs_amd/sh.py.
#include "mlp_args.hpp"
#include "sh4_common.hpp"

namespace snerf {

// one thread per (sample, float4 of the 32-wide row): quads 0..3 = SH, 4..7 = h columns 0..15 with column 15 (log density) replaced by 0
__global__ __launch_bounds__(256) void color_input_fwd_kernel(const float* __restrict__ dirs, int S, const float* __restrict__ h, int64_t N,
                                                             float* __restrict__ X) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = gid >> 3;
  const int q = (int)(gid & 7);
  if (n >= N) return;
  float4 v;
  if (q < 4) {
    const int64_t ray = N < (1LL << 31) ? (int64_t)((uint32_t)n / (uint32_t)S) : n / S;
    const float x = sh4_kplanes_input(dirs[ray * 3]), y = sh4_kplanes_input(dirs[ray * 3 + 1]), z = sh4_kplanes_input(dirs[ray * 3 + 2]);
    v = make_float4(sh4_coeff(4 * q, x, y, z), sh4_coeff(4 * q + 1, x, y, z), sh4_coeff(4 * q + 2, x, y, z), sh4_coeff(4 * q + 3, x, y, z));
  } else {
    v = *reinterpret_cast<const float4*>(h + n * 16 + 4 * (q - 4));
    if (q == 7) v.w = 0.f;
  }
  *reinterpret_cast<float4*>(X + n * 32 + 4 * q) = v;
}

// gh[:, :15] = gX[:, 16:31]; gh[:, 15] is left alone (the density enters the sigma_net backward through gaux)
__global__ __launch_bounds__(256) void color_input_bwd_kernel(const float* __restrict__ gX, int ldgx, int64_t N, float* __restrict__ gh) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = gid >> 4;
  const int c = (int)(gid & 15);
  if (n >= N || c == 15) return;
  gh[n * 16 + c] = gX[n * ldgx + 16 + c];
}

static int color_bwd_vd_impl(const snerf_mlp_desc* d, const float* W, const float* dirs, int32_t S, const float* h, int64_t N, const float* gY,
                             int32_t ldgy, float* gh, float* gW, float* ws, snerf_stream_t stream) {
  SNERF_REQUIRE(d && mlp_rows_vd_supported(d), "color_bwd_vd: the kernel is built for 31 -> 64 -> 64 -> 3 (ReLU, Sigmoid) with bf16 / fp16 operands");
  SNERF_REQUIRE(N >= 0 && N < (1LL << 31) && S >= 1 && N % S == 0, "color_bwd_vd: N=%lld S=%d", (long long)N, S);
  if (N == 0) return 0;
  SNERF_REQUIRE(W && dirs && h && gY && ldgy >= 3 && (gW || ws), "color_bwd_vd: null buffer / ldgy=%d", ldgy);
  // h rows are read as 8-float halves and gh written as float4s: 16-float rows, 16-byte aligned
  SNERF_REQUIRE((reinterpret_cast<uintptr_t>(h) & 15) == 0 && (!gh || (reinterpret_cast<uintptr_t>(gh) & 15) == 0), "color_bwd_vd: h / gh must be 16-byte aligned");
  MlpArgs a = {};
  a.d0 = 31; a.dout = 3; a.hidden_act = 1; a.out_act = 1; a.aux_col = -1;
  a.woff[0] = 0; a.woff[1] = 31 * 64; a.woff[2] = 31 * 64 + 64 * 64;
  a.X = h; a.ldx = 16; a.N = N; a.W = W; a.gY = gY; a.ldgy = ldgy; a.gX = gh; a.ldgx = 16;
  a.dirs = dirs; a.S = S;
  if (ws) {
    a.ws = ws; a.ws_rep = GW_REPLICAS; a.ws_stride = gw_ws_stride(d);  // snerf_mlp_gw_reduce folds it
  } else {
    a.gW = gW;
  }
  return mlp_rows_vd_dispatch(d, a, (hipStream_t)stream);
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_kplanes_color_input_fwd(const float* dirs, int32_t S, const float* h, int64_t N, float* X, snerf_stream_t stream) {
  SNERF_REQUIRE(N >= 0 && S >= 1 && N % S == 0, "color_input_fwd: N=%lld S=%d", (long long)N, S);
  if (N == 0) return 0;
  SNERF_REQUIRE(dirs && h && X, "color_input_fwd: null buffer");
  SNERF_REQUIRE((reinterpret_cast<uintptr_t>(h) & 15) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0, "color_input_fwd: h / X must be 16-byte aligned");
  const int64_t threads = N * 8;
  hipLaunchKernelGGL(color_input_fwd_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dirs, (int)S, h, N, X);
  SNERF_LAUNCH_CHECK("kplanes_color_input_fwd");
  return 0;
}

extern "C" int snerf_kplanes_color_input_bwd(const float* gX, int32_t ldgx, int64_t N, float* gh, snerf_stream_t stream) {
  SNERF_REQUIRE(N >= 0 && ldgx >= 31, "color_input_bwd: N=%lld ldgx=%d", (long long)N, ldgx);
  if (N == 0) return 0;
  SNERF_REQUIRE(gX && gh, "color_input_bwd: null buffer");
  const int64_t threads = N * 16;
  hipLaunchKernelGGL(color_input_bwd_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gX, (int)ldgx, N, gh);
  SNERF_LAUNCH_CHECK("kplanes_color_input_bwd");
  return 0;
}

extern "C" int snerf_kplanes_color_bwd_vd_supported(const snerf_mlp_desc* desc) { return desc && mlp_rows_vd_supported(desc) ? 1 : 0; }

extern "C" int snerf_kplanes_color_bwd_vd(const snerf_mlp_desc* desc, const float* W, const float* dirs, int32_t S, const float* h, int64_t N,
                                          const float* gY, int32_t ldgy, float* gh, float* gW, snerf_stream_t stream) {
  SNERF_REQUIRE(gW, "color_bwd_vd: null gW");
  return color_bwd_vd_impl(desc, W, dirs, S, h, N, gY, ldgy, gh, gW, nullptr, stream);
}

extern "C" int snerf_kplanes_color_bwd_vd_ws(const snerf_mlp_desc* desc, const float* W, const float* dirs, int32_t S, const float* h, int64_t N,
                                             const float* gY, int32_t ldgy, float* gh, float* workspace, snerf_stream_t stream) {
  SNERF_REQUIRE(workspace, "color_bwd_vd_ws: null workspace");
  return color_bwd_vd_impl(desc, W, dirs, S, h, N, gY, ldgy, gh, nullptr, workspace, stream);
}
