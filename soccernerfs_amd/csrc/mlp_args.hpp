// What the whole MLP kernel family shares (mlp.hip, mlp_lp.hip, mlp_rows.hip, mlp_rows128.hip, dense_lp.hip, color_vd.hip): the ONE kernel
// argument block, the weight-gradient add, the launch of a persistent-workgroup kernel and the prototypes of everything that is called from
// another translation unit.
#pragma once
#include "common.hpp"

namespace snerf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LDS_LIMIT = 160 * 1024;  // LDS of a gfx950 CU
constexpr int GW_REPLICAS = 16;        // replicas of a snerf_mlp_bwd_ws workspace
// floats between two replicas: the flat gradient padded to 64 floats
inline int64_t gw_ws_stride(const snerf_mlp_desc* d) {
  int64_t n = 0, prev = d->d_in;
  for (int l = 0; l < d->n_hidden; ++l) { n += prev * d->hidden; prev = d->hidden; }
  n += prev * d->d_out;
  return (n + 63) / 64 * 64;
}

struct MlpArgs {
  const float* X; int64_t N; int ldx; int d0;
  const float* W; int woff[4];
  int dout;
  float* Y; int ldy;
  int hidden_act, out_act;
  int aux_col; float* aux_out;
  const float* gY; int ldgy;
  const float* gaux;
  float* gX; int ldgx;
  float* gW;
  long long* gWfx;  // deterministic mode: weight gradients accumulate here as fixed point instead (common.hpp)
  int x16;          // X holds the 16-bit operand type (what snerf_kplanes_field_fwd wrote), not fp32: 16-bit kernels only
  // quotient epilogue of the backward (snerf_mlp_bwd_x16_quotient; 16-bit kernels, one hidden layer of 128): instead of gX the kernel writes
  // G = gX .* X (X = the 16-bit tile it holds in LDS) and lists the elements whose X vanished while gX did not (common.hpp: fix_append)
  float* G; int ldg;
  int32_t* fix_list; int fix_capacity;
  int32_t* fix_count; int32_t* fix_count_next;
  int variant;      // backward only: 0 = the default kernel for the shape, 1 = the workgroup-tile kernels of mlp_lp.hip (snerf_mlp_bwd_tile: A-B, cross-check)
  // weight-gradient workspace (snerf_mlp_bwd_ws; 16-bit kernels): ws_rep replicas of the flat gradient, ws_stride floats apart.  Workgroup b adds
  // into replica b % ws_rep instead of gW, so an address collects grid / ws_rep same-address atomics instead of one per workgroup (256 of
  // them took ~25 us at the end of every launch, whatever the element count); snerf_mlp_gw_reduce folds the replicas into gW later.
  float* ws; int ws_rep; int64_t ws_stride;
  // view-dependent colour backward (snerf_kplanes_color_bwd_vd, mlp_rows.hip): X = [SH4 of the ray direction | h[:, :15]] is formed in the
  // kernel from the per-ray directions [N / S, 3] and h (X above, row stride ldx = 16)
  const float* dirs; int S;
  // dense layers wider than one 128 x 128 block (snerf_dense_fwd / _bwd tile them; fp32 kernels): row stride of W in global memory (0 = dout), and
  // "add to what is there" for the forward's output (later K blocks of a linear layer) / the backward's input gradient (later column blocks)
  int ldw_g, acc_y, acc_gx;
};

// One weight-gradient element: into the fixed-point cells, this workgroup's workspace replica, or gW itself.  WS = false compiles the replica
// branch out: the exact-fp32 kernels are never handed a workspace (mlp.hip: mlp_bwd_impl gives them replica 0 as gW), and with the branch in,
// their 160- and 96-wide backwards spilled more (profiles/r13_mlp_INDEX.md).
template <bool WS = true>
__device__ __forceinline__ void gw_add(const MlpArgs& a, int64_t idx, float v) {
  if (a.gWfx) fx_atomic_add(a.gWfx + idx, v);
  else if (WS && a.ws) atomicAdd(a.ws + (int64_t)(blockIdx.x % (unsigned)a.ws_rep) * a.ws_stride + idx, v);
  else atomicAdd(a.gW + idx, v);
}

// Launch of a persistent-workgroup kernel Kernel(MlpArgs, n_tiles), whose workgroups walk the tiles: the grid is what the 256 CUs hold at once --
// LDS_LIMIT / lds_bytes workgroups per CU, at least one and at most `cap` (what registers and wave slots leave) -- and never more than n_tiles.
template <auto Kernel>
static int launch_persistent(const MlpArgs& a, int64_t n_tiles, size_t lds_bytes, int cap, int threads, hipStream_t st, const char* name) {
  int per_cu = (int)(LDS_LIMIT / lds_bytes);
  per_cu = per_cu < 1 ? 1 : (per_cu > cap ? cap : per_cu);
  int64_t grid = 256 * per_cu;
  if (grid > n_tiles) grid = n_tiles;
  SNERF_ALLOW_LDS(Kernel, LDS_LIMIT);
  hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(threads), lds_bytes, st, a, n_tiles);
  SNERF_LAUNCH_CHECK(name);
  return 0;
}

// ---- called across translation units ----
// 16-bit-operand kernels (mlp_lp.hip); the dispatch tries the wave-owns-rows backwards below first
bool mlp_bf16_supported(const snerf_mlp_desc* d);
int mlp_bf16_dispatch(const snerf_mlp_desc* d, const MlpArgs& a, bool bwd, hipStream_t st);
// wave-owns-rows backward of the 64-wide nets (mlp_rows.hip)
bool mlp_rows_supported(const snerf_mlp_desc* d, const MlpArgs& a);
int mlp_rows_dispatch(const snerf_mlp_desc* d, const MlpArgs& a, hipStream_t st);
// its view-dependent colour form (mlp_rows.hip; called from color_vd.hip)
bool mlp_rows_vd_supported(const snerf_mlp_desc* d);
int mlp_rows_vd_dispatch(const snerf_mlp_desc* d, const MlpArgs& a, hipStream_t st);
// wave-owns-rows backward of sigma_net (mlp_rows128.hip)
bool mlp_rows128_supported(const snerf_mlp_desc* d, const MlpArgs& a);
int mlp_rows128_dispatch(const snerf_mlp_desc* d, const MlpArgs& a, hipStream_t st);

}  // namespace snerf
