// Fused proposal density backward: the mirror of density_fwd_kernel (proposal_fused.hip).  On a step that updates the proposal networks it
// replaces, per level, mlp_rows_bwd_kernel<T,16,64,1> (the 8 -> 64 -> 1 net's backward from gdens) and kplanes_gather_bwd_kernel<8,6> (the
// plane scatter from the [N,8] feature gradient), and the forward no longer writes the [N,8] features: the kernel rebuilds them from the texels
// the product rule needs anyway.  Both levels run in ONE launch (a workgroup table: the first g0 workgroups take level 0, the rest level 1;
// their buffers and parameter segments are disjoint).
//
// Why: alone the four kernels are small (0.29 + 0.04 ms per step), but in the step they ran beside the field planes' HBM-bound sweep and
// stretched 4-10x: the net backward's [N,8] reads / writes and the scatter's serial walk (one sample at a time, each sample's 12 texel loads
// dependent on its coordinates) both wait on memory latency.  Here a wave owns 32 consecutive samples ("pair"), issues all of their texel loads
// before the first use (as the forward does), keeps features and feature gradients on chip, and walks the samples for the run-length-combined
// atomics out of LDS.
//
// Arithmetic:
//  * features: density_fwd_kernel's (bilerp4, product over the planes in plane order) -> bit-identical to the forward's;
//  * net: mlp_rows_bwd_kernel<T,16,64,1> phase for phase (same operand images, same MFMA sequence, trunc_exp derivative on the aux column),
//    so gX is bit-identical to snerf_mlp_bwd_ws's; weight gradients stay in registers for the wave's whole range and are flushed once per
//    workgroup into the snerf_mlp_bwd_ws workspace layout (snerf_mlp_gw_reduce folds it as before);
//  * product rule: kplanes_gather_bwd_kernel's (the plane value as the scatter forms it, prefix / suffix products, then wx, then wy);
//    contributions are run-length combined along the wave's WHOLE range of samples (the unfused walk cut a run every 32 samples), so the
//    plane gradients are the same terms in a different grouping.
//
// Work decomposition (wave = 64 lanes, lane = 16 g + c):
//  * gather: lane (g, c) takes sample 16 (g >> 1) + c of the pair, channels 4 (g & 1) .. +3 (one 16-byte load per texel; the sample's two
//    lanes read its 32-byte texel together): 24 loads in flight per lane;
//  * net: lane (g, c) holds features 4g .. 4g+3 of sample c / 16 + c (mlp_rows' B-operand layout), moved there by one lane swap (xor 32);
//  * walk: 16 lanes per group, lane = 8 half + ch (x-corner, channel) as in the unfused kernel; group k owns the (plane, row) streams 3k .. 3k+2
//    of the 12; a sample's per-plane gradient factors (G = prefix * suffix, [32][6][8] fp32) and its four axis taps come from LDS.  The pair
//    is walked in blocks of U = 8 samples: one sample at a time every link (sample x stream) waited for its own LDS reads, and with one wave
//    per SIMD (the residency budget) nothing hid that; a block's 12 x 8 reads are issued together and the run logic works on registers.
#include <type_traits>

#include "kplanes_common.hpp"
#include "mlp_rows_common.hpp"

namespace snerf {

namespace pbwd {

constexpr int C = 8, K0P = 16, H = 64, HB = H / 16, HK = H / 32, NPL = 6;

// LDS plan in 16-bit elements: mlp_rows' PlanR<16,64,1> (weights, then one [32][80] + [32][16] image pair per wave), then per wave the
// walk's taps ([32 samples][4 axes] x {i0, i1, w0, w1}, 2 KB) and the per-plane values v_q ([32][6][8] fp32, 6 KB: kept out of the registers
// across the net).  The per-plane gradient factors reuse the wave's image pair (6 KB) once the weight-gradient products are done.
//
// The output layer has ONE output, so of mlp_rows' two 16-wide images of it only output 0 is stored: WOT keeps row 0 and WOR column block 0
// ([H][4]: outputs 0..3).  Every lane reads the stored part and the lanes of the other outputs (1..15 of WOT's rows, 4..15 of WOR's columns)
// replace what they read by the zeros those images held there, so the MFMA operands keep their values.  That is 4 208 B less (62 864 B), which
// is what lets one workgroup of this kernel and three of the field scatter's pass B (scatter_halfwave_kernel's s_rec, PASS_B_LDS each) share a
// CU: see the assert below and the launcher's budget.
// gfx950: 160 KB per CU.  The allocation step is taken as 320 dwords, the compiler's LDS granularity for this target and the coarser reading: in
// 128-dword steps the sum asserted below is 2 KB smaller.
constexpr int LDS_PER_CU = 160 * 1024, LDS_GRANULE = 1280, PASS_B_LDS = 32 * 1024;
constexpr size_t lds_alloc(size_t bytes) { return (bytes + LDS_GRANULE - 1) / LDS_GRANULE * LDS_GRANULE; }

template <int NW>
struct Plan {
  static constexpr int L0 = K0P + 4, LH = H + 8, LO = 4;
  static constexpr int W0T = 0;               // [H][L0]    forward layer 0: natural k (features)
  static constexpr int W0R = W0T + H * L0;    // [K0P][LH]  gX: k = hidden units, permuted
  static constexpr int WOT = W0R + K0P * LH;  // [1][LH]    output layer: row = output 0 (outputs 1..15 are zeros), k = hidden units, permuted
  static constexpr int WOR = WOT + LH;        // [H][LO]    gZ_last: row = hidden unit, k = outputs 0..3 (4..15 are zeros), natural
  static constexpr int WEND = (WOR + H * LO + 7) / 8 * 8;
  static constexpr int LIA = rows_img_ld(H), LIB = rows_img_ld(K0P);
  static constexpr int IMG_A = 32 * LIA, IMG_B = 32 * LIB;
  static constexpr int SCR = IMG_A + IMG_B;
  static constexpr int TAPS = WEND + NW * SCR;  // int32 region starts here (element index of the 16-bit view)
  static constexpr int TAP_WORDS = 32 * 4 * 4, V_WORDS = 32 * NPL * C, EXTRA_WORDS = TAP_WORDS + V_WORDS;
  static constexpr size_t BYTES = (size_t)TAPS * 2 + (size_t)NW * EXTRA_WORDS * 4;
  static constexpr int NGW = K0P * H + H * 16;  // floats of the workgroup's weight-gradient reduction
  static_assert((size_t)SCR * 2 >= (size_t)32 * NPL * C * 4, "the per-plane gradient factors fit the wave's image pair");
  static_assert((size_t)NGW * 4 <= (size_t)NW * SCR * 2, "the weight-gradient reduction reuses the waves' scratch");
  static_assert((TAPS * 2) % 16 == 0, "taps region 16-byte aligned");
  static_assert((WOT * 2) % 16 == 0 && (WOR * 2) % 8 == 0, "the output layer's images are read 16 and 8 bytes at a time");
  static_assert(NW != 4 || lds_alloc(BYTES) + 3 * lds_alloc(PASS_B_LDS) <= (size_t)LDS_PER_CU,
                "one workgroup of this kernel and three of the field scatter's pass B fit one CU's LDS");
};

struct Level {
  snerf_kplanes_desc d;
  snerf_coords c;
  const float* planes;
  const float* W;       // [8 x 64 | 64 x 1]
  const float* gdens;   // [N]
  float* gplanes;       // plane-gradient view (layout of planes)
  float* ws;            // weight-gradient workspace (snerf_mlp_bwd_ws layout)
  float* gX;            // optional [N,8]
  int64_t N, pairs, ws_stride;
  int g_first, g_count, relu;
};
struct Args {
  Level lv[2];
  int g0;  // workgroups of level 0
};

// value of a per-plane table at a lane-dependent plane index, by selects (a dynamic index into the kernel argument would go through scratch)
template <typename V>
__device__ __forceinline__ V pick6(int q, V v0, V v1, V v2, V v3, V v4, V v5) {
  V r = v5;
  r = q == 4 ? v4 : r;
  r = q == 3 ? v3 : r;
  r = q == 2 ? v2 : r;
  r = q == 1 ? v1 : r;
  r = q == 0 ? v0 : r;
  return r;
}

// two waves per SIMD (<= 256 registers, 0 B scratch: 236 VGPRs for bf16, 211-223 for fp16); with 4-wave workgroups and 62 KB of LDS that is two workgroups per CU, or one
// beside three workgroups of pass B (launch_density_bwd's budget)
// CT: 1 = contracted coordinates (snerf_coords.contract of both levels; load_coords_ray).  Compile time: the run-time branch cost the bf16
// kernel a spilled register.
// WIDE: 0 = a flush addresses its texel by a 32-bit byte offset from the level's gradient view (the launcher checks that the view ends below
// 2^31 bytes), 1 = by the 64-bit form.  U: samples per block of the walk.
template <typename T, int NW, int CT = 0, int WIDE = 0, int U = 8>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void density_bwd_kernel(Args args) {
  static_assert(32 % U == 0, "a pair is a whole number of blocks");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  using P = Plan<NW>;
  typedef typename Ops<T>::v8 v8t;
  typedef typename Ops<T>::v4 v4t;
  constexpr float GS = Ops<T>::GS;
  const int lvl = (int)blockIdx.x >= args.g0 ? 1 : 0;
  const Level& a = args.lv[lvl];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;

  // ---- weights -> LDS (mlp_rows_bwd_kernel's staging with d0 = 8, dout = 1) ----
  {
    constexpr int NT = NW * 64;
    const float* W0 = a.W;
#pragma unroll
    for (int i = 0; i < (H * K0P + NT - 1) / NT; ++i) {  // W0T[u][f] = W0[f][u];  W0R[f][p] = W0[f][pi(p)]
      const int idx = threadIdx.x + i * NT;
      if (idx < H * K0P) {
        const int u = idx / K0P, f = idx - u * K0P;
        const int f2 = idx / H, p2 = idx - f2 * H;
        const float v1 = W0[(int64_t)(f < C ? f : 0) * H + u], v2 = W0[(int64_t)(f2 < C ? f2 : 0) * H + rows_pi(p2)];
        smem[P::W0T + u * P::L0 + f] = Ops<T>::cvt(f < C ? v1 : 0.f);
        smem[P::W0R + f2 * P::LH + p2] = Ops<T>::cvt(f2 < C ? v2 : 0.f);
      }
    }
    const float* WO = a.W + C * H;
#pragma unroll
    for (int i = 0; i < (H * P::LO + NT - 1) / NT; ++i) {  // WOT[0][p] = WO[pi(p)][0];  WOR[u][o] = WO[u][o], o < 4
      const int idx = threadIdx.x + i * NT;
      if (idx < H) smem[P::WOT + idx] = Ops<T>::cvt(WO[rows_pi(idx)]);
      if (idx < H * P::LO) {
        const int u2 = idx / P::LO, o2 = idx - u2 * P::LO;
        const float v2 = WO[u2];
        smem[P::WOR + u2 * P::LO + o2] = Ops<T>::cvt(o2 < 1 ? v2 : 0.f);
      }
    }
  }
  __syncthreads();

  T* imgA = smem + P::WEND + wave * P::SCR;
  T* imgB = imgA + P::IMG_A;
  float* Gs = reinterpret_cast<float*>(imgA);                               // [32][6][8] per-plane gradient factors (after dW0)
  int* taps = reinterpret_cast<int*>(smem + P::TAPS) + wave * P::EXTRA_WORDS;  // [32][4] x {i0, i1, w0, w1}
  float* Vs = reinterpret_cast<float*>(taps + P::TAP_WORDS);                     // [32][6][8] per-plane values (each lane reads back its own)

  const bool relu = a.relu != 0;
  const int rlo = relu ? 0 : (int)0x80000000;
  const uint32_t nomask = relu ? 0u : 0xffffffffu;
  // mlp_rows_bwd_kernel's lane-level operand moves (mlp_rows_common.hpp)
  auto hact = [&](f32x4& v) { rows_hact(v, rlo); };
  auto mask_by = [&](v8t gq, v8t act) -> v8t { return rows_mask_by<T>(gq, act, nomask); };
  auto tr8 = [&](const T* img, int ld, int blk) -> v8t { return rows_tr8<T>(img, ld, blk, g, c); };
  auto put_packed = [&](T* img, int ld, int sl, const v8t (&pk)[HK]) { rows_put_packed<T, HK>(img, ld, sl, pk, g, c); };
  auto pack2 = [&](const f32x4& b0, const f32x4& b1, bool grad) -> v8t { return rows_pack2<T>(b0, b1, grad); };

  f32x4 dW0[HB] = {};
  f32x4 dWo[HB] = {};

  // ---- this wave's range of pairs (consecutive samples: runs combine along it) ----
  const int64_t wl = (int64_t)((int)blockIdx.x - a.g_first) * NW + wave, nwl = (int64_t)a.g_count * NW;
  const int64_t p_begin = a.pairs * wl / nwl, p_end = a.pairs * (wl + 1) / nwl;

  // ---- the walk: group k = lane >> 4 owns (plane, row) streams 3k .. 3k + 2; lane = 8 half + ch.  Pending run per stream ----
  // A texel's key is what a flush addresses it by: the byte offset of this lane's float from the level's gradient view, or (WIDE) the texel
  // index in its plane.  Both name the texel one to one within a stream, so runs end where they did.
  typedef typename std::conditional<WIDE != 0, int, uint32_t>::type key_t;
  key_t pend_key[3] = {(key_t)-1, (key_t)-1, (key_t)-1};
  float pend_val[3] = {0.f, 0.f, 0.f};
  // A group's three streams lie in TWO planes, qa = 3k >> 1 and qa + 1: streams 0 and 2 in the first and the second, stream 1 in the first
  // (even k) or the second (odd k); a stream's row is (j + k) & 1.  What belongs to the x axis (index, this lane's corner weight, the factor)
  // is read and multiplied once per plane.  Per plane e: where its numbers lie in a sample's tap row (words) and factor row, the key's row
  // step and lane term; per stream: where its y index lies (the y weight two words on).  Set before each pair's walk from a lane number the
  // compiler takes for new (set_streams' caller): held in registers across the net, they put the kernel over the registers it is allocated.
  int tXi[2], tXw[2], gQ[2], tYi[3];
  key_t kRow[2], kLane[2];
  int64_t wOff[3] = {0, 0, 0};  // WIDE, per stream: this lane's float of texel 0 of the plane
  bool odd = false;
  auto set_streams = [&](int ln) {
    const int gw = ln >> 4, lw = ln & 15;
    odd = (gw & 1) != 0;
    const int r0 = a.d.res[0][0] > 0 ? a.d.res[0][0] : 1, r1 = a.d.res[0][1] > 0 ? a.d.res[0][1] : 1, r2 = a.d.res[0][2] > 0 ? a.d.res[0][2] : 1;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int q = ((3 * gw) >> 1) + e;
      tXi[e] = 4 * pair_a<NPL>(q);
      tXw[e] = tXi[e] + 2 + (lw >> 3);
      gQ[e] = q * C + (lw & 7);
      const int W = pick6(q, r0, r0, r0, r1, r1, r2);
      const int64_t off = pick6(q, a.d.off[0][0], a.d.off[0][1], a.d.off[0][2], a.d.off[0][3], a.d.off[0][4], a.d.off[0][5]) + lw;
      kRow[e] = WIDE ? (key_t)W : (key_t)W * (key_t)(C * 4);
      kLane[e] = WIDE ? (key_t)0 : (key_t)off * (key_t)4;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int st = 3 * gw + j, q = st >> 1;
      tYi[j] = 4 * pair_b<NPL>(q) + (st & 1);
      if constexpr (WIDE != 0) wOff[j] = pick6(q, a.d.off[0][0], a.d.off[0][1], a.d.off[0][2], a.d.off[0][3], a.d.off[0][4], a.d.off[0][5]) + lw;
    }
  };
  char* const gbase = reinterpret_cast<char*>(a.gplanes);
  // a pending run's sum goes out under the lane's own predicate; zero sums (a clamped column, samples without gradient) are not sent
  auto flush = [&](int j, bool go) {
    if (go & (pend_val[j] != 0.f)) {  // ONE predicate, and not the selects' own: the compiler then keeps the selects and skips no block
      if constexpr (WIDE != 0) atomicAdd(a.gplanes + wOff[j] + (int64_t)pend_key[j] * C, pend_val[j]);
      else atomicAdd(reinterpret_cast<float*>(gbase + pend_key[j]), pend_val[j]);
    }
  };
  // UU consecutive samples of the pair from s0: every LDS read of the block is issued before the first use, keys and values are formed
  // lane-parallel, then the run logic goes over registers in sample order (per stream the additions and the flushes of the one-sample walk)
  auto walk = [&](int s0, auto nu) {
#pragma clang fp contract(off)
    constexpr int UU = decltype(nu)::value;
    int xi[UU][2], yi[UU][3];
    float wx[UU][2], gf[UU][2], wy[UU][3];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
      const int* ts = taps + (s0 + u) * 16;
      const float* gs = Gs + (s0 + u) * (NPL * C);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        xi[u][e] = ts[tXi[e]];
        wx[u][e] = __int_as_float(ts[tXw[e]]);
        gf[u][e] = gs[gQ[e]];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        yi[u][j] = ts[tYi[j]];
        wy[u][j] = __int_as_float(ts[tYi[j] + 2]);
      }
    }
    key_t key[UU][3];
    float val[UU][3];
    const key_t kRow1 = odd ? kRow[1] : kRow[0];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
      key_t kx[2];
      float gq[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        kx[e] = WIDE ? (key_t)xi[u][e] : (key_t)xi[u][e] * (key_t)(C * 4) + kLane[e];
        gq[e] = gf[u][e] * wx[u][e];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const key_t kxj = j == 0 ? kx[0] : (j == 2 ? kx[1] : (odd ? kx[1] : kx[0]));
        const key_t krj = j == 0 ? kRow[0] : (j == 2 ? kRow[1] : kRow1);
        const float gqj = j == 0 ? gq[0] : (j == 2 ? gq[1] : (odd ? gq[1] : gq[0]));
        key[u][j] = (key_t)yi[u][j] * krj + kxj;
        val[u][j] = gqj * wy[u][j];
      }
    }
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const bool cut = key[u][j] != pend_key[j];
        flush(j, cut);
        pend_val[j] = cut ? val[u][j] : pend_val[j] + val[u][j];
        pend_key[j] = key[u][j];
      }
  };

  const int sl_g = g >> 1, hc = g & 1;  // gather: sample 16 sl_g + c of the pair, channels 4 hc .. 4 hc + 3
  for (int64_t pair = p_begin; pair < p_end; ++pair) {
    // ---- gather: coordinates, taps, all 24 texel loads in flight ----
    const int64_t n = pair * 32 + 16 * sl_g + c;
    const bool live_g = n < a.N;
    const int64_t nn = live_g ? n : a.N - 1;
    float p[4];
    if (a.c.mode == 0) {
      const float4 v = *reinterpret_cast<const float4*>(a.c.pts + nn * 4);
      p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    } else {
      const uint32_t r = (uint32_t)nn / (uint32_t)a.c.S;  // N < 2^31 (checked by the launcher)
      load_coords_ray<6, CT>(a.c, (int64_t)r, (int)((uint32_t)nn - r * (uint32_t)a.c.S), p);
    }
    const float ga_g = a.gdens[nn];
    AxisTap tap[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tap[k] = axis_tap(p[k], a.d.res[0][k] > 0 ? a.d.res[0][k] : 1);
    float4 t[NPL][4];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
      const AxisTap& tx = tap[pair_a<NPL>(q)];
      const AxisTap& ty = tap[pair_b<NPL>(q)];
      const int W = a.d.res[0][pair_a<NPL>(q)];
      const float* base = a.planes + a.d.off[0][q] + hc * 4;
      const float* r0 = base + ((int64_t)ty.i0 * W) * C;
      const float* r1 = base + ((int64_t)ty.i1 * W) * C;
      t[q][0] = *reinterpret_cast<const float4*>(r0 + (int64_t)tx.i0 * C);
      t[q][1] = *reinterpret_cast<const float4*>(r0 + (int64_t)tx.i1 * C);
      t[q][2] = *reinterpret_cast<const float4*>(r1 + (int64_t)tx.i0 * C);
      t[q][3] = *reinterpret_cast<const float4*>(r1 + (int64_t)tx.i1 * C);
    }
    // the walk's taps of this sample (the image pair and tap rows of the previous pair are free: see the publish at the end of the loop)
    if (hc == 0) {
      int4* tr = reinterpret_cast<int4*>(taps + (16 * sl_g + c) * 16);
#pragma unroll
      for (int k = 0; k < 4; ++k) tr[k] = make_int4(tap[k].i0, tap[k].i1, __float_as_int(tap[k].w0), __float_as_int(tap[k].w1));
    }
    // features (density_fwd_kernel: bilerp4, product in plane order) and the per-plane values as the unfused scatter forms them
    float feat[4];
    {
      float pr[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
      for (int q = 0; q < NPL; ++q) {
        const AxisTap& tx = tap[pair_a<NPL>(q)];
        const AxisTap& ty = tap[pair_b<NPL>(q)];
        const float4 w = tap_weights(tx, ty);
        const float nw[4] = {t[q][0].x, t[q][0].y, t[q][0].z, t[q][0].w}, ne[4] = {t[q][1].x, t[q][1].y, t[q][1].z, t[q][1].w};
        const float sw[4] = {t[q][2].x, t[q][2].y, t[q][2].z, t[q][2].w}, se[4] = {t[q][3].x, t[q][3].y, t[q][3].z, t[q][3].w};
        float4 vq;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pr[e] *= bilerp4(nw[e], ne[e], sw[e], se[e], w.x, w.y, w.z, w.w);
          // kplanes_gather_bwd_kernel: part = wx * (wy0 * ta + wy1 * tb) per x-corner, v = part(x0) + part(x1)
          const float part0 = tx.w0 * (ty.w0 * nw[e] + ty.w1 * sw[e]);
          const float part1 = tx.w1 * (ty.w0 * ne[e] + ty.w1 * se[e]);
          const float vv = part0 + part1;
          if (e == 0) vq.x = vv; else if (e == 1) vq.y = vv; else if (e == 2) vq.z = vv; else vq.w = vv;
        }
        *reinterpret_cast<float4*>(Vs + (16 * sl_g + c) * (NPL * C) + q * C + 4 * hc) = vq;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) feat[e] = 0.f + pr[e];  // the unfused gather sums over its one scale from 0 (-0 -> +0)
    }

    // ---- net operands in mlp_rows' layout: lane (g, c), g < 2: features 4g .. 4g+3 of samples c (sl 0) and 16 + c (sl 1) ----
    v4t x4[2];
    float gac[2];
    {
      float other[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) other[e] = __shfl_xor(feat[e], 32, 64);
      const float ga_o = __shfl_xor(ga_g, 32, 64);
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) {
        const bool live = pair * 32 + 16 * sl + c < a.N;
        float xv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[e] = (live && g < 2) ? (sl == 0 ? feat[e] : other[e]) : 0.f;
        x4[sl] = v4t{Ops<T>::cvt(xv[0]), Ops<T>::cvt(xv[1]), Ops<T>::cvt(xv[2]), Ops<T>::cvt(xv[3])};
        gac[sl] = live ? ((sl == sl_g) ? ga_g : ga_o) : 0.f;
      }
    }

    // ---- forward, layer 0: Z1^T = W0^T X^T ----
    v8t A1[2][HK];
    {
      f32x4 d[2][HB];
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
        const T* wrow = smem + P::W0T + (16 * hb + c) * P::L0;
        f32x4 acc[2] = {};
        const v4t w = *reinterpret_cast<const v4t*>(wrow + 4 * g);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) acc[sl] = Ops16<T>::mfma(w, x4[sl], acc[sl]);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          hact(acc[sl]);
          d[sl][hb] = acc[sl];
        }
      }
#pragma unroll
      for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int s = 0; s < HK; ++s) A1[sl][s] = pack2(d[sl][2 * s], d[sl][2 * s + 1], false);
    }
    // ---- output layer + trunc_exp backward on the aux column (lane: output 4g + r of sample c) ----
    v4t G0[2];
    {
      f32x4 y[2] = {};
      const T* wrow = smem + P::WOT + 8 * g;
#pragma unroll
      for (int s = 0; s < HK; ++s) {
        v8t w = ld8(wrow + 32 * s);
        if (c >= 1) w = v8t{};  // rows 1..15 of the 16-wide image: zeros
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) y[sl] = Ops<T>::mfma(w, A1[sl][s], y[sl]);
      }
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) {
        float gv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = 4 * g + r;
          float gg = 0.f;
          gg += o == 0 ? gac[sl] * __expf(fminf(fmaxf(y[sl][r], -15.f), 15.f)) : 0.f;
          gv[r] = o < 1 ? gg * GS : 0.f;
        }
        G0[sl] = v4t{Ops<T>::cvtg(gv[0]), Ops<T>::cvtg(gv[1]), Ops<T>::cvtg(gv[2]), Ops<T>::cvtg(gv[3])};
      }
    }
    // ---- dWO += A1^T gZo ----
    put_packed(imgA, P::LIA, 0, A1[0]);
    put_packed(imgA, P::LIA, 1, A1[1]);
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) *reinterpret_cast<v4t*>(imgB + (16 * sl + c) * P::LIB + 4 * g) = G0[sl];
    wave_lds_publish();
    {
      const v8t b = tr8(imgB, P::LIB, 0);
#pragma unroll
      for (int ba = 0; ba < HB; ++ba) dWo[ba] = Ops<T>::mfma(tr8(imgA, P::LIA, ba), b, dWo[ba]);
    }
    // ---- gZ1^T = (WO gZo^T) .* relu'(A1) ----
    v8t GZ1[2][HK];
    {
      f32x4 d[2][HB];
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) {
        v4t w = *reinterpret_cast<const v4t*>(smem + P::WOR + (16 * hb + c) * P::LO);
        if (g >= 1) w = v4t{};  // columns 4..15 of the 16-wide image: zeros
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          f32x4 acc = {};
          d[sl][hb] = Ops16<T>::mfma(w, G0[sl], acc);
        }
      }
#pragma unroll
      for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int s = 0; s < HK; ++s) GZ1[sl][s] = mask_by(pack2(d[sl][2 * s], d[sl][2 * s + 1], true), A1[sl][s]);
    }
    // ---- gX^T = W0 gZ1^T (lane g < 2: features 4g .. 4g+3 of sample 16 sl + c) ----
    f32x4 gx[2];
    {
      const T* wrow = smem + P::W0R + c * P::LH + 8 * g;
      f32x4 acc[2] = {};
#pragma unroll
      for (int s = 0; s < HK; ++s) {
        const v8t w = ld8(wrow + 32 * s);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) acc[sl] = Ops<T>::mfma(w, GZ1[sl][s], acc[sl]);
      }
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) {
        gx[sl] = f32x4{acc[sl][0] * (1.f / GS), acc[sl][1] * (1.f / GS), acc[sl][2] * (1.f / GS), acc[sl][3] * (1.f / GS)};
        const int64_t ns = pair * 32 + 16 * sl + c;
        if (a.gX && g < 2 && ns < a.N) *reinterpret_cast<f32x4*>(a.gX + ns * C + 4 * g) = gx[sl];
      }
    }
    // ---- dW0 += X^T gZ1 (X -> the narrow image, gZ1 -> the wide one) ----
    wave_lds_publish();
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) *reinterpret_cast<v4t*>(imgB + (16 * sl + c) * P::LIB + 4 * g) = x4[sl];
    put_packed(imgA, P::LIA, 0, GZ1[0]);
    put_packed(imgA, P::LIA, 1, GZ1[1]);
    wave_lds_publish();
    {
      v8t b[HB];
#pragma unroll
      for (int bb = 0; bb < HB; ++bb) b[bb] = tr8(imgA, P::LIA, bb);
      const v8t av = tr8(imgB, P::LIB, 0);
#pragma unroll
      for (int bb = 0; bb < HB; ++bb) dW0[bb] = Ops<T>::mfma(av, b[bb], dW0[bb]);
    }
    wave_lds_publish();  // the image pair becomes the per-plane gradient factors

    // ---- product rule (kplanes_gather_bwd_kernel): G_q = (gX * v_0 * .. * v_{q-1}) * (v_{q+1} * .. * v_5), per sample and channel ----
    {
      float gup[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float o = __shfl_xor(gx[1][e], 32, 64);
        gup[e] = sl_g == 0 ? gx[0][e] : o;
      }
      float* grow = Gs + (16 * sl_g + c) * (NPL * C) + 4 * hc;
      float v[NPL][4];
#pragma unroll
      for (int q = 0; q < NPL; ++q) {
        const float4 t4 = *reinterpret_cast<const float4*>(Vs + (16 * sl_g + c) * (NPL * C) + q * C + 4 * hc);
        v[q][0] = t4.x; v[q][1] = t4.y; v[q][2] = t4.z; v[q][3] = t4.w;
      }
      float pre[4] = {gup[0], gup[1], gup[2], gup[3]};
      float suf[NPL + 1][4];
#pragma unroll
      for (int e = 0; e < 4; ++e) suf[NPL][e] = 1.f;
#pragma unroll
      for (int q = NPL - 1; q >= 0; --q)
#pragma unroll
        for (int e = 0; e < 4; ++e) suf[q][e] = suf[q + 1][e] * v[q][e];
#pragma unroll
      for (int q = 0; q < NPL; ++q) {
        float4 gq;
        gq.x = pre[0] * suf[q + 1][0]; gq.y = pre[1] * suf[q + 1][1]; gq.z = pre[2] * suf[q + 1][2]; gq.w = pre[3] * suf[q + 1][3];
#pragma unroll
        for (int e = 0; e < 4; ++e) pre[e] *= v[q][e];
        *reinterpret_cast<float4*>(grow + q * C) = gq;
      }
    }
    wave_lds_publish();
    // ---- walk: run-length combined scatter along the wave's range ----
    {
      const int cnt = (int)((a.N - pair * 32) < 32 ? (a.N - pair * 32) : 32);
      int ln = lane;
      asm volatile("" : "+v"(ln));  // opaque: the streams' constants are formed here, per pair, from a few selects
      set_streams(ln);
      int s = 0;  // whole blocks, then a short last pair's remainder one sample at a time (rows past cnt are never read)
      for (; s + U <= cnt; s += U) walk(s, std::integral_constant<int, U>{});
      for (; s < cnt; ++s) walk(s, std::integral_constant<int, 1>{});
    }
    wave_lds_publish();  // the walk's reads are done before the next pair's taps and images
  }
  set_streams(lane);
#pragma unroll
  for (int j = 0; j < 3; ++j) flush(j, true);

  // ---- weight gradients: sum the workgroup's waves through LDS (mlp_rows' fixed order), then one atomic per element into the workspace ----
  {
    float* red = reinterpret_cast<float*>(smem + P::WEND);
    constexpr int NB0 = HB, NBLK = NB0 + HB;
    __syncthreads();
    auto each_block = [&](auto&& f) {
#pragma unroll
      for (int bb = 0; bb < HB; ++bb) f(bb, dW0[bb]);
#pragma unroll
      for (int ba = 0; ba < HB; ++ba) f(NB0 + ba, dWo[ba]);
    };
    constexpr int CAP = (int)(((size_t)NW * P::SCR * 2) / ((size_t)P::NGW * 4));
    constexpr int COPIES = CAP >= NW ? NW : CAP;
    static_assert(COPIES >= 1, "no room for the weight-gradient reduction");
    for (int w0 = 0; w0 < NW; w0 += COPIES) {
      if (wave >= w0 && wave < w0 + COPIES) {
        float* mine = red + (wave - w0) * P::NGW;
        each_block([&](int blk, const f32x4& vv) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* cell = mine + (blk * 4 + r) * 64 + lane;
            *cell = (w0 == 0 ? 0.f : *cell) + vv[r];
          }
        });
      }
      __syncthreads();
    }
    const int wg = (int)blockIdx.x - a.g_first;
    float* ws = a.ws + (int64_t)(wg % GW_REPLICAS) * a.ws_stride;
    for (int i = wave; i < NBLK * 4; i += NW) {
      const int q = (i + 4 * wg) % (NBLK * 4);
      const int blk = q >> 2, r = q & 3;
      float vv = red[q * 64 + lane];
#pragma unroll
      for (int k = 1; k < COPIES; ++k) vv += red[k * P::NGW + q * 64 + lane];
      vv *= 1.f / GS;
      if (blk < NB0) {
        const int f = 4 * g + r, u = 16 * blk + c;
        if (f < C) atomicAdd(ws + (int64_t)f * H + u, vv);
      } else {
        const int u = 16 * (blk - NB0) + 4 * g + r;
        if (c < 1) atomicAdd(ws + C * H + u, vv);
      }
    }
  }
}

}  // namespace pbwd

static bool density_bwd_shape_ok(const snerf_kplanes_desc* d, const snerf_mlp_desc* m) {
  return d && m && d->C == 8 && d->n_coords == 4 && d->n_scales == 1 && m->d_in == 8 && m->hidden == 64 && m->n_hidden == 1 && m->d_out == 1 &&
         (m->operands == 1 || m->operands == 2) && m->out_act == 0 && (m->hidden_act == 0 || m->hidden_act == 1);
}

// max_workgroups: the residency budget (snerf_kplanes_density_bwd_budget); <= 0 = every workgroup the device holds at once.  The workgroups are
// persistent (each stays until its range of pairs is done), so two per CU leave a SIMD 16 registers and the CU 33 KB of LDS: nothing else starts
// a wave there until the launch ends.  A smaller grid gives each workgroup a longer range and leaves CUs, or half of every CU, to the stream beside it.
template <typename T, int CT, int WIDE>
static int launch_density_bwd(pbwd::Args& a, const int64_t* pairs, int n_levels, int max_workgroups, hipStream_t st) {
  constexpr int NW = 4;  // 8-wave workgroups (mlp_rows' shape) would need 121 KB of LDS: one per CU
  using P = pbwd::Plan<NW>;
  auto k = pbwd::density_bwd_kernel<T, NW, CT, WIDE>;
  SNERF_ALLOW_LDS(k, P::BYTES);
  // persistent grid sized to residency: as many workgroups as fit on the device at once, split between the levels by their pair counts
  static int resident = 0;
  if (!resident) {
    int dev = 0, cus = 256, per_cu = 0;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, NW * 64, P::BYTES) != hipSuccess || per_cu < 1) per_cu = 1;
    resident = cus * per_cu;
  }
  const int64_t total = pairs[0] + (n_levels > 1 ? pairs[1] : 0);
  const int64_t waves_needed = (total + 1) / 2;  // at least two pairs per wave
  int64_t grid = (waves_needed + NW - 1) / NW;
  if (grid > resident) grid = resident;
  if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
  if (grid < n_levels) grid = n_levels;
  int g0 = n_levels > 1 ? (int)((grid * pairs[0] + total / 2) / total) : (int)grid;
  if (n_levels > 1) {
    if (g0 < 1) g0 = 1;
    if (g0 > grid - 1) g0 = (int)grid - 1;
  }
  a.g0 = g0;
  a.lv[0].g_first = 0; a.lv[0].g_count = g0;
  if (n_levels > 1) { a.lv[1].g_first = g0; a.lv[1].g_count = (int)grid - g0; }
  else { a.lv[1] = a.lv[0]; }
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(NW * 64), P::BYTES, st, a);
  SNERF_LAUNCH_CHECK("kplanes_density_bwd");
  return 0;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_kplanes_density_bwd_supported(const snerf_kplanes_desc* desc, const snerf_mlp_desc* net) { return density_bwd_shape_ok(desc, net) ? 1 : 0; }

extern "C" int snerf_kplanes_density_bwd(const snerf_density_bwd_level* levels, int32_t n_levels, snerf_stream_t stream) {
  return snerf_kplanes_density_bwd_budget(levels, n_levels, 0, stream);
}

extern "C" int snerf_kplanes_density_bwd_budget(const snerf_density_bwd_level* levels, int32_t n_levels, int32_t max_workgroups, snerf_stream_t stream) {
  SNERF_REQUIRE(levels && (n_levels == 1 || n_levels == 2), "kplanes_density_bwd: n_levels=%d (1 or 2)", n_levels);
  pbwd::Args a = {};
  int64_t pairs[2] = {0, 0};
  int operands = 0, live = 0, contract = -1;
  bool wide = false;  // a level's gradient view reaches 2^31 bytes: the kernel's 32-bit texel offsets do not span it
  for (int l = 0; l < n_levels; ++l) {
    const snerf_density_bwd_level& L = levels[l];
    SNERF_REQUIRE(L.desc && L.coords && L.net, "kplanes_density_bwd: null descriptor (level %d)", l);
    SNERF_REQUIRE(density_bwd_shape_ok(L.desc, L.net), "kplanes_density_bwd: built for one scale of six C = 8 planes and the 8 -> 64 -> 1 net with 16-bit "
                  "operands (level %d: C=%d n_coords=%d n_scales=%d; net %d -> %d x %d -> %d, operands %d)", l, L.desc->C, L.desc->n_coords,
                  L.desc->n_scales, L.net->d_in, L.net->hidden, L.net->n_hidden, L.net->d_out, L.net->operands);
    SNERF_REQUIRE(l == 0 || L.net->operands == operands, "kplanes_density_bwd: the levels' nets have different operand types");
    operands = L.net->operands;
    SNERF_REQUIRE(L.N >= 0 && L.N < (1LL << 31), "kplanes_density_bwd: N=%lld (level %d)", (long long)L.N, l);
    SNERF_REQUIRE(L.coords->mode == 0 || (L.coords->mode == 1 && L.coords->S >= 1 && L.N % L.coords->S == 0), "kplanes_density_bwd: coords.mode=%d, N=%lld, S=%d",
                  L.coords->mode, (long long)L.N, L.coords->S);
    SNERF_REQUIRE_CONTRACT(L.coords, "kplanes_density_bwd");
    SNERF_REQUIRE(contract < 0 || L.coords->contract == contract, "kplanes_density_bwd: the levels' coords.contract differ (%d, %d)", contract, L.coords->contract);
    contract = L.coords->contract;
    for (int k = 0; k < 4; ++k) SNERF_REQUIRE(L.desc->res[0][k] >= 1, "kplanes_density_bwd: res[0][%d]=%d", k, L.desc->res[0][k]);
    if (L.N == 0) continue;
    SNERF_REQUIRE(L.planes && L.W && L.gdens && L.grad_planes && L.workspace, "kplanes_density_bwd: null buffer (level %d)", l);
    SNERF_REQUIRE(L.coords->mode == 0 ? L.coords->pts != nullptr
                                      : (L.coords->origins && L.coords->dirs && L.coords->ebins && L.coords->times && L.coords->S > 0),
                  "kplanes_density_bwd: incomplete coordinates (level %d)", l);
    SNERF_REQUIRE(!L.gX || (reinterpret_cast<uintptr_t>(L.gX) & 15) == 0, "kplanes_density_bwd: gX must be 16-byte aligned");
    for (int q = 0; q < pbwd::NPL; ++q) {
      SNERF_REQUIRE(L.desc->off[0][q] >= 0, "kplanes_density_bwd: off[0][%d]=%lld (level %d)", q, (long long)L.desc->off[0][q], l);
      const int64_t texels = (int64_t)L.desc->res[0][pair_a<pbwd::NPL>(q)] * L.desc->res[0][pair_b<pbwd::NPL>(q)];
      // one texel past the plane: the x0 + 1 corner of a clamped column forms (and never sends) that address
      if ((L.desc->off[0][q] + (texels + 1) * pbwd::C) * 4 >= (1LL << 31)) wide = true;
    }
    pbwd::Level& o = a.lv[live];
    o.d = *L.desc; o.c = *L.coords; o.planes = L.planes; o.W = L.W; o.gdens = L.gdens; o.gplanes = L.grad_planes; o.ws = L.workspace; o.gX = L.gX;
    o.N = L.N; o.pairs = (L.N + 31) / 32; o.ws_stride = (snerf_mlp_param_count(L.net) + 63) / 64 * 64; o.relu = L.net->hidden_act == 1;
    pairs[live] = o.pairs;
    ++live;
  }
  if (live == 0) return 0;
  auto launch = [&](auto ct, auto wd) {
    constexpr int CT = decltype(ct)::value, WD = decltype(wd)::value;
    return operands == 2 ? launch_density_bwd<fp16, CT, WD>(a, pairs, live, max_workgroups, (hipStream_t)stream)
                         : launch_density_bwd<bf16, CT, WD>(a, pairs, live, max_workgroups, (hipStream_t)stream);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (contract == 1) return wide ? launch(I1{}, I1{}) : launch(I1{}, I0{});
  return wide ? launch(I0{}, I1{}) : launch(I0{}, I0{});
}
