// Device helpers shared by the K-Planes kernels (kplanes.hip, kplanes_sorted.hip, kplanes_coords.hip and the fused field / proposal kernels).
#pragma once
#include "common.hpp"

namespace snerf {

struct AxisTap {
  int i0, i1;    // texel indices along the axis (i1 clamped for addressing)
  float w0, w1;  // weights of i0 / i1:  (i1 - x), (x - i0); w1 forced to 0 when i0+1 is out of range
};

// ATen grid_sampler semantics for align_corners=True + padding_mode="border":
//   x_pix = ((x + 1) / 2) * (size - 1), clipped to [0, size-1]; taps floor / floor+1.
// axis_pix is that pixel coordinate and axis_tap is built from it, so floor(axis_pix(x, size)) == axis_tap(x, size).i0 by construction: the
// sort keys and pass B's chunk-local sort words (kplanes_sorted.hip) take the floor alone and must name the cell that pass B's taps address.
__device__ __forceinline__ float axis_pix(float x, int size) {
  float fx = ((x + 1.f) / 2.f) * (float)(size - 1);
  return fminf((float)(size - 1), fmaxf(fx, 0.f));
}
__device__ __forceinline__ AxisTap tap_from_pix(float fx, int size) {
  float f0 = floorf(fx);
  AxisTap t;
  t.i0 = (int)f0;
  t.w0 = (f0 + 1.f) - fx;
  t.w1 = fx - f0;
  bool in = (t.i0 + 1) <= (size - 1);
  t.i1 = in ? t.i0 + 1 : t.i0;
  if (!in) t.w1 = 0.f;  // out-of-range corner contributes nothing (ATen within_bounds_2d)
  return t;
}
__device__ __forceinline__ AxisTap axis_tap(float x, int size) { return tap_from_pix(axis_pix(x, size), size); }

// Euclidean position of sample s of ray r: Frustums.get_positions, o + (d * (e[s] + e[s+1])) / 2 in that order
__device__ __forceinline__ void ray_position(const snerf_coords& c, int64_t r, int s, float pos[3]) {
  const float* eb = c.ebins + r * (c.S + 1) + s;
  const float mid = eb[0] + eb[1];
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[k] = c.origins[r * 3 + k] + (c.dirs[r * 3 + k] * mid) / 2.f;
}

// snerf_coords.contract = 1: SceneContraction(order=inf) and the K-Planes fields' halving, evaluated as the elementwise
// float32 expression  where(m < 1, pos, (2 - 1 / m) * (pos / m)) / 2  with m = max_k |pos_k|: every operation rounds on its own (no fused
// multiply-add, IEEE division), so the coordinate has the bits of that expression and of every other kernel's recomputation of it.
// m == 1 takes the second branch (it returns pos there as well: 2 - 1 = 1, pos / 1 = pos).
__device__ __forceinline__ void contract_inf_half(const float pos[3], float p[4]) {
#pragma clang fp contract(off)
  const float m = fmaxf(fmaxf(fabsf(pos[0]), fabsf(pos[1])), fabsf(pos[2]));
  const bool inside = m < 1.f;
  const float f = 2.f - 1.f / m;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float y = inside ? pos[k] : f * (pos[k] / m);
    p[k] = y / 2.f;
  }
}

// coordinate of sample s of ray r (snerf_coords mode 1: positions derived from rays + euclidean bin edges).  NP = 3 (static scene): there is no
// time axis and c.times, which may be null then, is never read.
// CT: where the contraction switch is decided.  -1 = at run time: c.contract is uniform over a launch and sits in the argument block, a scalar
// branch.  0 / 1 = at compile time, for the kernel families that live at their register limit (the fused field forward, its ordered walk and the
// render tail; the fused proposal backward; the coordinate gradient), where the run-time branch cost spilled registers or an occupancy step
// (DESIGN.md 4.15): their launchers pick the instantiation from coords.contract, and with CT = 0 the function is the text it always was.
template <int NP = 6, int CT = -1>
__device__ __forceinline__ void load_coords_ray(const snerf_coords& c, int64_t r, int s, float p[4]) {
  if (CT > 0 || (CT < 0 && c.contract)) {
    float pos[3];
    ray_position(c, r, s, pos);
    contract_inf_half(pos, p);
  } else {
    const float* eb = c.ebins + r * (c.S + 1) + s;
    float mid = eb[0] + eb[1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float pos = c.origins[r * 3 + k] + (c.dirs[r * 3 + k] * mid) / 2.f;
      float q = (pos - c.aabb_min[k]) / (c.aabb_max[k] - c.aabb_min[k]);
      p[k] = c.rescale ? q * 2.f - 1.f : q;
    }
  }
  if constexpr (NP == 6) p[3] = c.times[r] * 2.f - 1.f;
  else p[3] = 0.f;
}

// host: the ray buffers of mode-1 coordinates are all there.  A 4-coordinate descriptor needs the rays' times; a static scene has none to give.
inline bool ray_coords_complete(const snerf_coords* c, int n_coords) { return c->origins && c->dirs && c->ebins && (c->times || n_coords == 3); }

// host: what every entry that takes a snerf_coords checks about its contraction switch before it launches anything.  Returns the complaint,
// or null when the descriptor is fine.
inline const char* coords_contract_complaint(const snerf_coords* c) {
  if (c->contract != 0 && c->contract != 1) return "coords.contract must be 0 (none) or 1 (L-inf scene contraction)";
  if (c->contract == 1 && c->mode != 1) return "coords.contract = 1 needs coords.mode 1 (rays): the points of mode 0 are already final";
  return nullptr;
}
#define SNERF_REQUIRE_CONTRACT(c, who)                                                     \
  do {                                                                                     \
    const char* complaint_ = snerf::coords_contract_complaint(c);                          \
    SNERF_REQUIRE(complaint_ == nullptr, "%s: %s (contract=%d, mode=%d)", who, complaint_ ? complaint_ : "", (c)->contract, (c)->mode); \
  } while (0)

// coordinate of sample n along x,y,z,t in grid_sample's [-1,1] convention
template <int NP, int CT = -1>
__device__ __forceinline__ void load_coords(const snerf_coords& c, int64_t n, float p[4]) {
  if (c.mode == 0) {
    if (NP == 6) {
      float4 v = *reinterpret_cast<const float4*>(c.pts + n * 4);
      p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    } else {  // static scene: pts is [N,3]
      p[0] = c.pts[n * 3]; p[1] = c.pts[n * 3 + 1]; p[2] = c.pts[n * 3 + 2]; p[3] = 0.f;
    }
  } else {
    int64_t r = n / c.S;  // a 64-bit software division (~100 instructions): loops over consecutive samples step (r, s) themselves
    int s = (int)(n - r * c.S);
    load_coords_ray<NP, CT>(c, r, s, p);
  }
}

template <int NP> struct PlanePairs;
template <> struct PlanePairs<6> {  // XY XZ XT YZ YT ZT
  static constexpr int a[6] = {0, 0, 0, 1, 1, 2};
  static constexpr int b[6] = {1, 2, 3, 2, 3, 3};
};
template <> struct PlanePairs<3> {  // static scene: XY XZ YZ
  static constexpr int a[3] = {0, 0, 1};
  static constexpr int b[3] = {1, 2, 2};
};

// The same tables as arithmetic on the plane index.  Inside an unrolled plane loop q is a literal and these fold; indexing the constexpr
// arrays above did not always (kplanes_gather_bwd_kernel, field_fwd_kernel: the taps were kept in scratch and read back through a
// uniform-but-dynamic index, 16 dwords per sample -- profiles/r02_kernels.md).
template <int NP> __host__ __device__ constexpr int pair_a(int q) { return NP == 6 ? (q < 3 ? 0 : (q < 5 ? 1 : 2)) : (q < 2 ? 0 : 1); }
template <int NP> __host__ __device__ constexpr int pair_b(int q) { return NP == 6 ? (q < 3 ? q + 1 : (q < 5 ? q - 1 : 3)) : (q < 1 ? 1 : 2); }
static_assert(pair_a<6>(0) == 0 && pair_a<6>(2) == 0 && pair_a<6>(3) == 1 && pair_a<6>(4) == 1 && pair_a<6>(5) == 2, "pair_a<6>");
static_assert(pair_b<6>(0) == 1 && pair_b<6>(1) == 2 && pair_b<6>(2) == 3 && pair_b<6>(3) == 2 && pair_b<6>(4) == 3 && pair_b<6>(5) == 3, "pair_b<6>");
static_assert(pair_a<3>(0) == 0 && pair_a<3>(1) == 0 && pair_a<3>(2) == 1 && pair_b<3>(0) == 1 && pair_b<3>(1) == 2 && pair_b<3>(2) == 2, "pair_*<3>");

__device__ __forceinline__ float4 f4_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4_scale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// Bilinear blend of the four texels of a tap with a FIXED evaluation order and explicit roundings (no compiler-chosen contraction):
// the forward gather and the quotient form of the sorted scatter (kplanes_sorted.hip, QUOT) must produce the SAME bits for a plane's
// value at a sample -- the quotient G / v_q cancels the forward's v_q exactly only if pass B recomputes that very number (a value that is
// a small difference of large texels would otherwise come back with a large relative error).
__device__ __forceinline__ float bilerp4(float nw, float ne, float sw, float se, float w00, float w10, float w01, float w11) {
  float acc = __fmul_rn(nw, w00);
  acc = __fmaf_rn(ne, w10, acc);
  acc = __fmaf_rn(sw, w01, acc);
  acc = __fmaf_rn(se, w11, acc);
  return acc;
}
// the four corner weights of a tap pair: (x0,y0), (x1,y0), (x0,y1), (x1,y1)
__device__ __forceinline__ float4 tap_weights(const AxisTap& tx, const AxisTap& ty) {
  return make_float4(__fmul_rn(tx.w0, ty.w0), __fmul_rn(tx.w1, ty.w0), __fmul_rn(tx.w0, ty.w1), __fmul_rn(tx.w1, ty.w1));
}

// bilinear value of plane p for this lane's 4 channels
template <int C>
__device__ __forceinline__ float4 plane_sample(const float* __restrict__ base, int W, const AxisTap& tx, const AxisTap& ty, int cg) {
  const float* r0 = base + ((int64_t)ty.i0 * W) * C + cg * 4;
  const float* r1 = base + ((int64_t)ty.i1 * W) * C + cg * 4;
  float4 nw = *reinterpret_cast<const float4*>(r0 + (int64_t)tx.i0 * C);
  float4 ne = *reinterpret_cast<const float4*>(r0 + (int64_t)tx.i1 * C);
  float4 sw = *reinterpret_cast<const float4*>(r1 + (int64_t)tx.i0 * C);
  float4 se = *reinterpret_cast<const float4*>(r1 + (int64_t)tx.i1 * C);
  const float4 w = tap_weights(tx, ty);
  return make_float4(bilerp4(nw.x, ne.x, sw.x, se.x, w.x, w.y, w.z, w.w), bilerp4(nw.y, ne.y, sw.y, se.y, w.x, w.y, w.z, w.w),
                     bilerp4(nw.z, ne.z, sw.z, se.z, w.x, w.y, w.z, w.w), bilerp4(nw.w, ne.w, sw.w, se.w, w.x, w.y, w.z, w.w));
}

// ---- the product rule and the run-length combiner, shared by every plane-gradient kernel ----
__device__ __forceinline__ float loo_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 loo_mul(float4 a, float4 b) { return f4_mul(a, b); }

// Leave-one-out products of the Hadamard product over the planes: term[q] = g * prod_{p != q} v[p], the gradient with respect to plane q's
// interpolated value, for T = float (one channel) or float4 (four).  ONE fixed order for every kernel -- the planes in front are folded into
// g from the left (pre), the planes behind come as a suffix product built from the right:
//   pre = g;  term[q] = pre * suf[q + 1];  pre *= v[q]      with suf[q] = v[q] * suf[q + 1], suf[NP] = 1 (never multiplied: x * 1 is x).
// The quotient form divides g * prod_p v[p] by v[q] and its fix-up adds these very terms, so all of them have to round alike.
template <int NP, typename T>
__device__ __forceinline__ void leave_one_out(T g, const T (&v)[NP], T (&term)[NP]) {
  T suf[NP];
  suf[NP - 1] = v[NP - 1];
#pragma unroll
  for (int q = NP - 2; q >= 0; --q) suf[q] = loo_mul(suf[q + 1], v[q]);
  T pre = g;
#pragma unroll
  for (int q = 0; q < NP - 1; ++q) {
    term[q] = loo_mul(pre, suf[q + 1]);
    pre = loo_mul(pre, v[q]);
  }
  term[NP - 1] = pre;
}

// One pending run of a run-length combiner: contributions to the same key (a texel, in the caller's numbering) are summed in a register and
// sent -- flush(key, sum): the caller's address arithmetic and its atomicAdd or grad_add<FX> -- only when the key changes, and once more by
// drain() at the end of the walk.  A sum of exactly zero (a clamped tap's weight, no contribution yet) is never sent.
struct PendingRun {
  int key = -1;
  float val = 0.f;
  template <typename F>
  __device__ __forceinline__ void add(int k, float v, F&& flush) {
    if (k != key) {
      drain(flush);
      key = k;
      val = v;
    } else {
      val += v;
    }
  }
  template <typename F>
  __device__ __forceinline__ void drain(F&& flush) const {
    if (val != 0.f) flush(key, val);
  }
};

}  // namespace snerf

// the launcher FN<C, NP> of a descriptor `desc`: C = 8, 16, 32 channels, NP = 6 planes (x, y, z, t) or 3 (static scene)
#define DISPATCH_C_NP(FN, ...)                                                          \
  do {                                                                                  \
    if (desc->n_coords == 4) {                                                          \
      if (desc->C == 32) return FN<32, 6>(__VA_ARGS__);                                 \
      if (desc->C == 16) return FN<16, 6>(__VA_ARGS__);                                 \
      return FN<8, 6>(__VA_ARGS__);                                                     \
    } else {                                                                            \
      if (desc->C == 32) return FN<32, 3>(__VA_ARGS__);                                 \
      if (desc->C == 16) return FN<16, 3>(__VA_ARGS__);                                 \
      return FN<8, 3>(__VA_ARGS__);                                                     \
    }                                                                                   \
  } while (0)
