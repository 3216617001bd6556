// Building blocks of the wave-owns-rows MLP backward (mlp_rows.hip), shared with the fused proposal backward (proposal_bwd.hip), whose gX must stay
// bit-identical to it: the 16x16x16 MFMA, the permuted contraction index of the weight images, the image strides, and the lane-level operand moves
// (lane = 16 g + c; see the header of mlp_rows.hip for the layouts).
#pragma once
#include <stdint.h>

#include "mlp_lp_common.hpp"

namespace snerf {

typedef short rows_s4 __attribute__((ext_vector_type(4)));

template <typename T>
struct Ops16;
template <>
struct Ops16<bf16> {
  static __device__ __forceinline__ f32x4 mfma(Ops<bf16>::v4 a, Ops<bf16>::v4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(rows_s4, a), __builtin_bit_cast(rows_s4, b), c, 0, 0, 0);
  }
};
template <>
struct Ops16<fp16> {
  static __device__ __forceinline__ f32x4 mfma(Ops<fp16>::v4 a, Ops<fp16>::v4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};

// hidden unit held by contraction slot p of a permuted-k image (see the header of mlp_rows.hip)
__host__ __device__ constexpr int rows_pi(int p) { return (p & ~31) + 16 * ((p >> 2) & 1) + 4 * ((p >> 3) & 3) + (p & 3); }

// row stride (elements) of a [sample][width] scratch image: (stride in dwords) mod 64 is an odd multiple of 8, so the 8 rows a 32-lane half
// touches in one ds_read_b64_tr_b16 (4 rows x 32 B per 16-lane group, two groups) fall on 8 disjoint sets of 8 banks
__host__ __device__ constexpr int rows_img_ld(int width) { return width <= 16 ? 16 : (width <= 32 ? 48 : (width <= 64 ? 80 : 144)); }

// hidden activation on an accumulator fragment: relu = ONE v_max_i32 on the float's bits (negative floats are negative integers; fmaxf costs a
// second, canonicalising v_max); rlo = 0 for relu, INT_MIN for none
__device__ __forceinline__ void rows_hact(f32x4& v, int rlo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = __float_as_int(v[e]);
    v[e] = __int_as_float(b > rlo ? b : rlo);
  }
}

// gradient fragment .* relu'(activation fragment), both packed 16-bit: the activations are >= 0 after relu, so "positive" is "bits != 0";
// per 32-bit word min(a, 1) * 0xffff in packed u16 arithmetic gives the keep-mask of its two elements.  nomask = ~0 without relu.
template <typename T>
__device__ __forceinline__ typename Ops<T>::v8 rows_mask_by(typename Ops<T>::v8 gq, typename Ops<T>::v8 act, uint32_t nomask) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const uint32_t c_one2 = 0x00010001u, c_all2 = 0xffffffffu;
  u4 gw = __builtin_bit_cast(u4, gq);
  const u4 aw = __builtin_bit_cast(u4, act);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t m;  // VOP3P, both halves at once (the compiler's own lowering of the vector form went through v_cmp / v_cndmask / v_perm)
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(m) : "v"(aw[w]), "v"(c_one2));
    asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(m) : "v"(m), "v"(c_all2));
    gw[w] &= m | nomask;
  }
  return __builtin_bit_cast(typename Ops<T>::v8, gw);
}

// operand fragment of a weight-gradient product: block `blk` (16 columns) of a [32 samples][ld] image, contraction slot (g, j) <-> sample
// 4g + j (j < 4) / 16 + 4g + j - 4.  Lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3 of its 4 x 16 block.
template <typename T>
__device__ __forceinline__ typename Ops<T>::v8 rows_tr8(const T* img, int ld, int blk, int g, int c) {
  const int q = c >> 2, p = c & 3;
  const T* a0 = img + (4 * g + q) * ld + blk * 16 + 4 * p;
  typedef __attribute__((address_space(3))) rows_s4 lds_v4;
  const rows_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(a0));
  const rows_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(a0 + 16 * ld));
  typedef short s8 __attribute__((ext_vector_type(8)));
  const s8 w = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(typename Ops<T>::v8, w);
}

// a packed fragment set (k-step s holds unit blocks 2s and 2s + 1 of sample c) -> image rows 16 sl + c
template <typename T, int HK>
__device__ __forceinline__ void rows_put_packed(T* img, int ld, int sl, const typename Ops<T>::v8 (&pk)[HK], int g, int c) {
  typedef typename Ops<T>::v4 v4t;
#pragma unroll
  for (int s = 0; s < HK; ++s) {
    const v4t lo = {pk[s][0], pk[s][1], pk[s][2], pk[s][3]}, hi = {pk[s][4], pk[s][5], pk[s][6], pk[s][7]};
    T* row = img + (16 * sl + c) * ld + 32 * s + 4 * g;
    *reinterpret_cast<v4t*>(row) = lo;
    *reinterpret_cast<v4t*>(row + 16) = hi;
  }
}

// two accumulator blocks -> one packed 16-bit fragment (activations: cvt; gradients: cvtg)
template <typename T>
__device__ __forceinline__ typename Ops<T>::v8 rows_pack2(const f32x4& b0, const f32x4& b1, bool grad) {
  typename Ops<T>::v8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[e] = grad ? Ops<T>::cvtg(b0[e]) : Ops<T>::cvt(b0[e]);
    r[4 + e] = grad ? Ops<T>::cvtg(b1[e]) : Ops<T>::cvt(b1[e]);
  }
  return r;
}

}  // namespace snerf
