// The fused K-Planes field tile (plane gather -> sigma_net -> density, colour net -> rgb for 32 samples held in LDS), shared by the kernels
// built on it: field_fwd_kernel (field_fused.hip: density / rgb to HBM, the training leftovers) and field_render_kernel (render_eval.hip: a
// workgroup walks a whole ray and composites it on chip).  One copy of the arithmetic, so the two give the same bits per sample.
//
// Work decomposition of a tile (512 threads = 8 waves, tile = 32 samples):
//   gather   16 lanes per sample: (4-channel group) x (scale parity, by wave); float4 texel reads as kplanes_gather_fwd_kernel, the Hadamard
//            product of the six planes in registers, rounded once into the LDS A-operand image X [32][32 n_scales + 8]
//   sigma 0  wave w owns hidden units 16w..16w+15; ITS B operand of W0 (32 n_scales / 32 k-steps x 8 values) lives in registers for the
//            whole persistent loop, so the 160 x 128 matrix never enters LDS
//   sigma 1, colour 0/1/out: small products from LDS-resident weights (21 KB).
#pragma once
#include "kplanes_common.hpp"
#include "mlp_lp_common.hpp"
#include "sh4_common.hpp"

namespace snerf {

constexpr int FF_TS = 32;     // samples per tile
constexpr int FF_H = 128;     // sigma_net hidden width
constexpr int FF_HC = 64;     // color_net hidden width
constexpr int FF_GEO = 15;    // geometry features = colour-net inputs; output column 15 of sigma_net is the density pre-activation
constexpr int FF_NW = 8;      // waves per workgroup

struct FieldArgs {
  snerf_kplanes_desc d;
  const float* planes;
  snerf_coords c;
  int64_t N;
  const float* Wsig;  // [K0 x 128 | 128 x 16] row-major [in][out]
  const float* Wcol;  // [15 x 64 | 64 x 64 | 64 x 3]; view-dependent: [31 x 64 | 64 x 64 | 64 x 3]
  float* dens;        // [N]   exp(sigma_net(.)[15])
  float* rgb;         // [N,3] sigmoid(color_net(.))
  void* feat16;       // optional [N, 32 n_scales] in the operand type: the rounded feature tile, for an UNFUSED backward (snerf_mlp_bwd_x16)
  float* h;           // optional [N,16]: the raw sigma_net outputs (color_net's input, column 15 = log density)
  float* feat32;      // optional [N, 32 n_scales] fp32: the features before rounding, for the quotient form of the plane scatter
};

template <int NS>
struct PlanFF {
  static constexpr int K0 = 32 * NS, LK0 = ldb(K0), LKH = ldb(FF_H), LKC = ldb(FF_HC), LKX = ldb(32);
  static constexpr int SWOT = 0;                          // sigma out  [16][LKH]
  static constexpr int CW0T = SWOT + 16 * LKH;            // colour L0  [64][LKX]
  static constexpr int CW1T = CW0T + FF_HC * LKX;         // colour L1  [64][LKC]
  static constexpr int CWOT = CW1T + FF_HC * LKC;         // colour out [16][LKC]
  static constexpr int CX = CWOT + 16 * LKC;              // colour input tile [TS][LKX] (columns 15..31 stay zero; VD: SH 0..15, h 16..30, 31 zero)
  static constexpr int A1 = CX + FF_TS * LKX;             // sigma hidden tile [TS][LKH]
  static constexpr int XS = A1 + FF_TS * LKH;             // feature tile [TS][LK0]; the colour hidden tiles reuse it once sigma layer 0 is done
  static constexpr int XS_LEN = FF_TS * LK0 > 2 * FF_TS * LKC ? FF_TS * LK0 : 2 * FF_TS * LKC;
  static constexpr int TOTAL = XS + XS_LEN;
  static constexpr size_t BYTES = (size_t)TOTAL * 2;
};

// features of one sample for this lane's 4 channels and scale s: product over the NP planes -- six, or the three space planes of a static scene /
// of frozen time planes (interpolate_kplanes, kplanes_field.py:77-126; :95-99)
template <int NP = 6>
__device__ __forceinline__ float4 scale_features(const snerf_kplanes_desc& d, const float* __restrict__ planes, const float p[4], int s, int cg,
                                                 float4 (*v_out)[NP] = nullptr) {
  AxisTap tap[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) tap[k] = axis_tap(p[k], d.res[s][k] > 0 ? d.res[s][k] : 1);
  float4 prod = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const float4 v = plane_sample<32>(planes + d.off[s][q], d.res[s][pair_a<NP>(q)], tap[pair_a<NP>(q)], tap[pair_b<NP>(q)], cg);
    if (v_out) (*v_out)[q] = v;
    prod = f4_mul(prod, v);
  }
  return prod;
}

template <typename T>
__device__ __forceinline__ void relu4(f32x4& v) {
  v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
}

// this wave's B operand of sigma_net layer 0: hidden units 16 wave .. +15, k = 32 ks + 8 (lane >> 4) .. +8
template <typename T, int K0>
__device__ __forceinline__ void load_breg(const float* __restrict__ W0, int wave, int lane, typename Ops<T>::v8 (&breg)[K0 / 32]) {
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < K0 / 32; ++ks) {
    typename Ops<T>::v8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = Ops<T>::cvt(W0[(int64_t)(ks * 32 + lk * 8 + e) * FF_H + wave * 16 + lr]);
    breg[ks] = b;
  }
}

// gather phase: 16 lanes per sample = (4-channel group cg) x (scale parity sg); rounds the features into the A-operand image XS
template <typename T, int NS, bool F32OUT = false, int NP = 6, int CT = 0>
__device__ __forceinline__ void gather_tile(const FieldArgs& a, int64_t n0, T* XS) {
  using P = PlanFF<NS>;
  // waves 0-3 take the even scales, waves 4-7 the odd ones: the scale index is wave-uniform, so the descriptor reads stay scalar
  const int sample = (threadIdx.x & 255) >> 3, cg = threadIdx.x & 7, sg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
  const int64_t n = n0 + sample;
  float p[4];
  const bool live = n < a.N;
  if (live) load_coords<NP, CT>(a.c, n, p);
#pragma unroll 1  // one scale's 24 texel reads in flight at a time: unrolled, the three scales' loads cost ~160 VGPRs and the occupancy the kernel lives on
  for (int s = sg; s < NS; s += 2) {
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) f = scale_features<NP>(a.d, a.planes, p, s, cg);
    const typename Ops<T>::v4 t = {Ops<T>::cvt(f.x), Ops<T>::cvt(f.y), Ops<T>::cvt(f.z), Ops<T>::cvt(f.w)};
    *reinterpret_cast<typename Ops<T>::v4*>(XS + sample * P::LK0 + s * 32 + cg * 4) = t;
    if constexpr (F32OUT)
      if (live) *reinterpret_cast<float4*>(a.feat32 + n * (32 * NS) + s * 32 + cg * 4) = f;  // 8 lanes x 16 B = one 128-B row segment
  }
}

// sigma_net layer 0 from the register-resident B operand: A1 = relu(X W0), column block = wave
template <typename T, int NS>
__device__ __forceinline__ void sigma_layer0(const T* XS, const typename Ops<T>::v8 (&breg)[NS], T* A1, T* A1t, int ldt, int wave, int lane) {
  using P = PlanFF<NS>;
  constexpr int MT = FF_TS / 16;
  const int lr = lane & 15, lk = lane >> 4;
  f32x4 acc[MT] = {};
#pragma unroll
  for (int ks = 0; ks < NS; ++ks)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = Ops<T>::mfma(ld8(XS + (m * 16 + lr) * P::LK0 + ks * 32 + lk * 8), breg[ks], acc[m]);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    relu4<T>(acc[m]);
    store_rt<T>(A1, P::LKH, A1t, ldt, m, wave, acc[m], lane);
  }
}

// Once per workgroup: this wave's B operand of sigma_net layer 0 into registers, every other weight matrix into LDS, the colour input tile cleared.
// VD: the view-dependent colour net (kplanes_field.py:206-216, :260-262, :314-323): its input tile holds SH degree 4 of the sample's ray direction
// (coords mode 1, sh4_common.hpp: the bits of soccernerfs_amd/sh.py) in columns 0..15 and the geometry features in 16..30; layer 0 is 31 x 64.
template <typename T, int NS, bool VD>
__device__ __forceinline__ void field_stage_weights(const FieldArgs& a, T* smem, typename Ops<T>::v8 (&breg)[NS]) {
  using P = PlanFF<NS>;
  constexpr int K0 = P::K0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  T* CX = smem + P::CX;
  load_breg<T, K0>(a.Wsig, wave, lane, breg);
  stage_w<T>(a.Wsig + K0 * FF_H, FF_H, 16, FF_H, 16, nullptr, 0, smem + P::SWOT, P::LKH);
  constexpr int CIN = VD ? 16 + FF_GEO : FF_GEO;  // colour-net inputs
  stage_w<T>(a.Wcol, CIN, FF_HC, 32, FF_HC, nullptr, 0, smem + P::CW0T, P::LKX);
  stage_w<T>(a.Wcol + CIN * FF_HC, FF_HC, FF_HC, FF_HC, FF_HC, nullptr, 0, smem + P::CW1T, P::LKC);
  stage_w<T>(a.Wcol + CIN * FF_HC + FF_HC * FF_HC, FF_HC, 3, FF_HC, 16, nullptr, 0, smem + P::CWOT, P::LKC);
  for (int idx = threadIdx.x; idx < FF_TS * P::LKX; idx += blockDim.x) CX[idx] = (T)0.f;  // columns 15..31 stay zero for the whole kernel
}

// One tile: samples n0 .. n0 + 31 (those below a.N).  Opens with the workgroup barrier that separates it from the previous tile (or from
// field_stage_weights).  What leaves the tile goes through the two sinks -- dens(row in tile, n, density) from waves 0-1 after sigma_net,
// rgb(row in tile, n, channel, value) from waves 0-1 after the colour net -- so a caller decides where density and colour live.
// KEEP: what a training step leaves behind for its backward -- 0 nothing (eval), 1 the 16-bit feature tile + the sigma_net outputs,
// 2 those + the fp32 features (quotient scatter).  Compile-time: as run-time pointer tests these cost every variant registers.
// NP: planes per scale, 6 or 3 (a 3-coordinate descriptor); a template parameter too, so that the six-plane tile is the code it was.
// CT: 1 = contracted coordinates (snerf_coords.contract, load_coords_ray); a template parameter for the same reason -- these kernels sit at
// their register limit and the run-time branch cost several instantiations spilled registers.  The CT = 1 kernels are built by
// field_fused_contract.hip and render_eval_contract.hip.
template <typename T, int NS, int KEEP, bool VD, int NP = 6, int CT = 0, typename DensSink, typename RgbSink>
__device__ __forceinline__ void field_tile(const FieldArgs& a, int64_t n0, T* smem, const typename Ops<T>::v8 (&breg)[NS], DensSink&& dens_sink,
                                           RgbSink&& rgb_sink) {
  using P = PlanFF<NS>;
  constexpr int K0 = P::K0, MT = FF_TS / 16;
  constexpr int CH0 = VD ? 16 : 0;  // first column of the geometry features in CX
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  T *XS = smem + P::XS, *A1 = smem + P::A1, *CX = smem + P::CX, *CA1 = smem + P::XS, *CA2 = smem + P::XS + FF_TS * P::LKC;
  __syncthreads();  // weights staged / the previous tile's colour layers have read CA1, CA2 (= XS)
  gather_tile<T, NS, KEEP == 2, NP, CT>(a, n0, XS);
  if constexpr (VD) {  // one SH coefficient per thread: 32 samples x 16 (the previous tile's colour layer 0 read CX before the loop-top barrier)
    const int sample = threadIdx.x >> 4, k = threadIdx.x & 15;
    const int64_t n = n0 + sample;
    float v = 0.f;
    if (n < a.N) {
      const int64_t ray = (int64_t)((uint32_t)n / (uint32_t)a.c.S);  // N < 2^31 (validate_field)
      v = sh4_coeff(k, sh4_kplanes_input(a.c.dirs[ray * 3]), sh4_kplanes_input(a.c.dirs[ray * 3 + 1]), sh4_kplanes_input(a.c.dirs[ray * 3 + 2]));
    }
    CX[sample * P::LKX + k] = Ops<T>::cvt(v);
  }
  __syncthreads();
  if constexpr (KEEP >= 1) {  // the tile's rows are contiguous in feat16: one coalesced 16-B store per 8 features
    T* F16 = reinterpret_cast<T*>(a.feat16);
    for (int vi = threadIdx.x; vi < FF_TS * (K0 / 8); vi += FF_NW * 64) {
      const int r = vi / (K0 / 8), c8 = vi - r * (K0 / 8);
      if (n0 + r < a.N) *reinterpret_cast<typename Ops<T>::v8*>(F16 + (n0 + r) * K0 + c8 * 8) = ld8(XS + r * P::LK0 + c8 * 8);
    }
  }
  sigma_layer0<T, NS>(XS, breg, A1, nullptr, 0, wave, lane);
  __syncthreads();
  if (wave < MT) {  // sigma_net output layer: 16 columns; column 15 -> density, columns 0..14 -> colour-net input
    f32x4 acc[1] = {};
    mma_rr<1, FF_H>(A1 + wave * 16 * P::LKH, P::LKH, smem + P::SWOT, P::LKH, 0, acc, lane);
    const int col = lane & 15, row0 = wave * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float y = acc[0][r];
      const int64_t n = n0 + row0 + r;
      if (col == FF_GEO && n < a.N) dens_sink(row0 + r, n, expf(y));  // trunc_exp forward (activations.py:32)
      if constexpr (KEEP >= 1)
        if (n < a.N) a.h[n * 16 + col] = y;
      CX[(row0 + r) * P::LKX + CH0 + col] = col < FF_GEO ? Ops<T>::cvt(y) : (T)0.f;
    }
  }
  __syncthreads();
  {  // colour layer 0: K = 32 (15 used), 4 column blocks x MT row blocks = 8 blocks, one per wave
    f32x4 acc[1] = {};
    const int nt = wave & 3, mt = wave >> 2;
    mma_rr<1, 32>(CX + mt * 16 * P::LKX, P::LKX, smem + P::CW0T, P::LKX, nt, acc, lane);
    relu4<T>(acc[0]);
    store_rt<T>(CA1, P::LKC, nullptr, 0, mt, nt, acc[0], lane);
  }
  __syncthreads();
  {
    f32x4 acc[1] = {};
    const int nt = wave & 3, mt = wave >> 2;
    mma_rr<1, FF_HC>(CA1 + mt * 16 * P::LKC, P::LKC, smem + P::CW1T, P::LKC, nt, acc, lane);
    relu4<T>(acc[0]);
    store_rt<T>(CA2, P::LKC, nullptr, 0, mt, nt, acc[0], lane);
  }
  __syncthreads();
  if (wave < MT) {
    f32x4 acc[1] = {};
    mma_rr<1, FF_HC>(CA2 + wave * 16 * P::LKC, P::LKC, smem + P::CWOT, P::LKC, 0, acc, lane);
    const int col = lane & 15, row0 = wave * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (col < 3 && n0 + row0 + r < a.N) rgb_sink(row0 + r, n0 + row0 + r, col, 1.f / (1.f + expf(-acc[0][r])));
  }
}

// The forward kernel (field_fused.hip describes it): a persistent workgroup strides over the tiles; density and colour go to HBM.  NP = 6 is
// instantiated by field_fused.hip, NP = 3 (a 3-coordinate descriptor) by field_fused_static.hip.
template <typename T, int NS, int KEEP = 0, bool VD = false, int NP = 6, int CT = 0>
__global__ __launch_bounds__(FF_NW * 64, 4) void field_fwd_kernel(FieldArgs a, int64_t n_tiles) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  typename Ops<T>::v8 breg[NS];
  field_stage_weights<T, NS, VD>(a, smem, breg);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    field_tile<T, NS, KEEP, VD, NP, CT>(
        a, tile * FF_TS, smem, breg, [&](int, int64_t n, float v) { a.dens[n] = v; },
        [&](int, int64_t n, int col, float v) { a.rgb[n * 3 + col] = v; });
}

// The same tiles walked in the order of a ray permutation (snerf_kplanes_field_fwd_ordered: coords.mode = 1 and S % 32 == 0, so a tile is 32 samples
// of ONE ray): with tpr = S / 32, tile k of the walk is sub-tile k % tpr of ray ray_order[k / tpr].  All samples of a ray share t, so with the rays in
// order of frame time the tiles resident at one moment read the same two texel rows of every XT / YT / ZT plane.  Every sample's outputs go to that
// sample's own rows, whatever the walk: the results are those of field_fwd_kernel bit for bit.  A kernel of its own, so that field_fwd_kernel keeps
// its arguments and its registers.
template <typename T, int NS, int KEEP = 0, bool VD = false, int CT = 0>
__global__ __launch_bounds__(FF_NW * 64, 4) void field_fwd_ordered_kernel(FieldArgs a, uint32_t n_tiles, const int32_t* __restrict__ ray_order,
                                                                          uint32_t tpr) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  typename Ops<T>::v8 breg[NS];
  uint32_t k = blockIdx.x, k_end = n_tiles, step = gridDim.x;  // fewer than 8 workgroups: a plain stride over the ordered tiles
  // Workgroups with equal blockIdx.x % 8 share an XCD, and so an L2: group x walks the x-th contiguous eighth of the ordered tiles, gridDim.x / 8
  // members striding inside it, so that each L2 holds the rows of its own range of frame times, however many frames the batch spans.  Placement is
  // affinity only: the eight ranges tile [0, n_tiles) whatever runs where.  (The launcher makes the grid a multiple of 8; workgroups past the last
  // whole eight would have no place.)  Against a plain stride over the whole list, where every L2 sees the same one or two frame times: 274.5-274.8
  // against 276.3-276.8 us alone at the preset, 0.836 against 0.845 GB fetched (profiles/r23_fwd_order_INDEX.md).
  if (gridDim.x >= 8) {
    const uint32_t x = blockIdx.x & 7;
    step = gridDim.x >> 3;
    if ((blockIdx.x >> 3) >= step) return;
    k = (uint32_t)((uint64_t)x * n_tiles >> 3) + (blockIdx.x >> 3);
    k_end = (uint32_t)((uint64_t)(x + 1) * n_tiles >> 3);
  }
  field_stage_weights<T, NS, VD>(a, smem, breg);
  for (; k < k_end; k += step) {
    const uint32_t r = k / tpr, sub = k - r * tpr;
    field_tile<T, NS, KEEP, VD, 6, CT>(
        a, ((int64_t)ray_order[r] * tpr + sub) * FF_TS, smem, breg, [&](int, int64_t n, float v) { a.dens[n] = v; },
        [&](int, int64_t n, int col, float v) { a.rgb[n * 3 + col] = v; });
  }
}

// grid of the persistent forward: two 8-wave workgroups per CU where the LDS plan allows (125 VGPRs)
template <int NS>
inline int64_t field_fwd_grid(int64_t n_tiles) {
  int per_cu = (int)(LDS_LIMIT / PlanFF<NS>::BYTES);
  per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
  const int64_t grid = 256 * per_cu;
  return grid > n_tiles ? n_tiles : grid;
}

// the shapes the fused field kernels are built for (snerf_kplanes_field_fwd_supported)
int validate_field(const snerf_kplanes_desc* d, const snerf_coords* c, int64_t N, const snerf_mlp_desc* sd, const snerf_mlp_desc* cd, int max_scales = 6);

// the unordered forward for a 3-coordinate descriptor (field_fused_static.hip: the NP = 3 instantiations in a translation unit of their own)
int launch_field_fwd_static(const FieldArgs& a, int operands, hipStream_t st, bool vd);

// the forward with contracted coordinates (a.c.contract = 1), six or three planes, ordered walk included (field_fused_contract.hip)
int launch_field_fwd_contract(const FieldArgs& a, int operands, const int32_t* ray_order, hipStream_t st, bool vd);

#define FF_DISPATCH(FN, operands, ns, ...)                                                   \
  do {                                                                                       \
    if ((operands) == 2) {                                                                   \
      switch (ns) {                                                                          \
        case 1: return FN<fp16, 1>(__VA_ARGS__); case 2: return FN<fp16, 2>(__VA_ARGS__);    \
        case 3: return FN<fp16, 3>(__VA_ARGS__); case 4: return FN<fp16, 4>(__VA_ARGS__);    \
        default: return FN<fp16, 5>(__VA_ARGS__);                                            \
      }                                                                                      \
    }                                                                                        \
    switch (ns) {                                                                            \
      case 1: return FN<bf16, 1>(__VA_ARGS__); case 2: return FN<bf16, 2>(__VA_ARGS__);      \
      case 3: return FN<bf16, 3>(__VA_ARGS__); case 4: return FN<bf16, 4>(__VA_ARGS__);      \
      default: return FN<bf16, 5>(__VA_ARGS__);                                              \
    }                                                                                        \
  } while (0)

// six scales as well (BASELINE config 3: K0 = 192)
#define FF_DISPATCH_FWD(FN, operands, ns, ...)                                               \
  do {                                                                                       \
    if ((ns) == 6) {                                                                         \
      if ((operands) == 2) return FN<fp16, 6>(__VA_ARGS__);                                  \
      return FN<bf16, 6>(__VA_ARGS__);                                                       \
    }                                                                                        \
    FF_DISPATCH(FN, operands, ns, __VA_ARGS__);                                              \
  } while (0)

}  // namespace snerf
