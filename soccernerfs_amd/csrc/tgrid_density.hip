// Fused proposal density of a temporal-grid field: table encode -> L*C -> 16 -> 1 net -> trunc_exp in ONE kernel per proposal level.
//
// Replaces TemporalHashMLPDensityField.density_fn (NS/fields/nerfplayer_nerfacto_field.py:83-104: TemporalGridEncoder, tcnn.Network
// {FullyFusedMLP, ReLU, None, 16 neurons, 1 hidden layer}, trunc_exp) as ProposalNetworkSampler.generate_ray_samples calls it per level
// (NS/model_components/ray_samplers.py:559-600).  Unfused that is tgrid_runs_kernel<false, true> -> [N, L*C] fp32 in HBM ->
// mlp_fwd_kernel<16,16,1,64> -> raw output and density: two launches and ~88 B per sample through HBM for a 176-weight net.  Here the
// features of a segment of a ray live in LDS only and the raw net output in a register.
//
// Arithmetic = the pair's, operation for operation, so densities are BIT-IDENTICAL to snerf_tgrid_encode_fwd + snerf_mlp_fwd (aux = trunc_exp,
// tests/test_gpu_tgrid_density.py):
//  * encode: tgrid.hip's run-length forward -- a group of 2 C lanes = (channel, a | b column) walks consecutive samples of one ray at one level
//    and keeps the current cell's eight corner values in registers; per sample tg_ray_x / tg_cell / tg_cell_interp of tgrid_common.hpp and the
//    same pair sum.  No contraction in this file (tgrid_common.hpp), as in tgrid.hip.
//  * net: mlp.hip's exact-fp32 kernels run v_mfma_f32_16x16x4_f32, which is a k-ordered fmaf chain from a zero accumulator, one rounding per
//    product; their zero padding of the input width adds +0 to an accumulator that is never -0.  The same chain is written out here as fmaf
//    on the VALU: 176 weights are 11 MFMA k-steps per 16 samples with 15 of 16 output columns idle, and would need the features in an
//    A-operand image.  Hidden unit j = fmaf over k = 0 .. L*C - 1 of x[k] * W0[k][j]; ReLU = fmaxf(., 0); output = fmaf over the 16 hidden units.
//
// Work decomposition: 256 threads; L * 2 C lanes (20 for the preset's L = 5, C = 2) own one segment of <= 32 samples of a ray, one lane group
// per level, so a workgroup holds G = min(16, 256 / (L * 2 C)) segments.  Phase 1: every group walks its segment and leaves the features in
// LDS ([G][32][L*C | 1] floats: the odd row stride spreads phase 2's row reads over the banks; 17 KB at the preset's shape, so the
// registers, not LDS, bound the waves per SIMD).  Phase 2: one thread per sample runs the net with the
// weights read from LDS at wave-uniform addresses (broadcast) and writes one float.  No atomics, no scratch.
#include "tgrid_common.hpp"

#pragma clang fp contract(off)

namespace snerf {

constexpr int TD_C = 2, TD_H = 16, TD_MAXF = 16, TD_RUN = 32, TD_NT = 256, TD_MAXG = 16;

struct TgridDensityArgs {
  snerf_tgrid_desc d;
  snerf_coords c;
  const float* emb;
  const float* times;  // [R]
  const float* W;      // [L*C x 16 | 16 x 1] row-major [in][out]
  float* dens;         // [R * S]
  int64_t R;
  int segs, run, G;    // segments per ray, samples per segment (<= TD_RUN), segments per workgroup
};

__host__ __device__ constexpr int td_ldf(int LC) { return LC | 1; }  // row stride of the feature tile: odd
__host__ __device__ constexpr int td_lds_floats(int G, int LC) { return G * TD_RUN * td_ldf(LC) + TD_MAXF * TD_H + TD_H; }

__global__ __launch_bounds__(TD_NT) void tgrid_density_kernel(TgridDensityArgs a, int64_t n_batches) {
  extern __shared__ __align__(16) float td_smem[];
  const int L = a.d.L, LC = L * TD_C, LPG = 2 * TD_C, LPS = L * LPG;  // lanes per (segment, level) and per segment
  const int G = a.G, S = a.c.S, LDF = td_ldf(LC);
  float* feat = td_smem;                    // [G][TD_RUN][LDF]
  float* W0s = td_smem + G * TD_RUN * LDF;  // [LC][16]
  float* WOs = W0s + TD_MAXF * TD_H;        // [16]
  for (int i = threadIdx.x; i < LC * TD_H + TD_H; i += TD_NT) {
    if (i < LC * TD_H) W0s[i] = a.W[i]; else WOs[i - LC * TD_H] = a.W[i];
  }
  // ---- this lane's slot of phase 1: segment g of the workgroup, level, channel, column ----
  const int g = threadIdx.x / LPS;
  const int k = threadIdx.x - g * LPS;
  const int level = k / LPG, ch = (k % LPG) >> 1, ab = k & 1;
  const bool slot = g < G;  // the lanes behind the last whole segment idle through phase 1
  const TgLevel lv = tg_level(a.d, slot ? level : 0, 3);
  const bool align = a.d.align_corners != 0;
  const int n_rows = a.d.grid_C - TD_C - 1;
  float ext[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) ext[d] = a.c.aabb_max[d] - a.c.aabb_min[d];
  const int64_t n_segs = a.R * a.segs;

  for (int64_t bt = blockIdx.x; bt < n_batches; bt += gridDim.x) {
    // ---- phase 1: features of this group's segment -> LDS ----
    {
      const int64_t sg = bt * G + g;
      int64_t r = 0;
      int s0 = 0, s1 = 0;  // no segment: the empty range of ray 0 (the pair sum below is a cross-lane operation of the full wave)
      if (slot && sg < n_segs) {
        r = sg / a.segs;
        s0 = (int)(sg - r * a.segs) * a.run;
        s1 = (s0 + a.run) < S ? (s0 + a.run) : S;
      }
      int col = 0;
      float wt = 0.f;
      tg_slot_from_time(a.times[r], TD_C, n_rows, ch, ab, col, wt);
      col = col < 0 ? 0 : (col >= a.d.grid_C ? a.d.grid_C - 1 : col);  // a time outside [0,1] reads a wrong column, never outside its row
      float o[3], dir[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        o[d] = a.c.origins[r * 3 + d];
        dir[d] = a.c.dirs[r * 3 + d];
      }
      const float* eb = a.c.ebins + r * (S + 1);
      uint32_t ppg[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};  // no cell yet (tgrid.hip)
      float reg[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) reg[i] = 0.f;
      float* frow = feat + (g * TD_RUN) * LDF + level * TD_C + ch;
      for (int i = 0; i < a.run; ++i) {  // a.run trips for every lane of the workgroup
        const int s = s0 + i;
        const bool have = s < s1;
        float acc = 0.f;
        bool oob = false;
        if (have) {
          const float mid = eb[s] + eb[s + 1];
          float x[3], fr[3];
          uint32_t pg[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) x[d] = tg_ray_x(o[d], dir[d], mid, a.c.aabb_min[d], ext[d]);
          oob = tg_out_of_range(x, 3);
          tg_cell(lv, align, x, 3, pg, fr);
          if (!oob && wt != 0.f) {  // an out-of-range sample reads nothing, a dead (channel, column) slot adds nothing
            if (pg[0] != ppg[0] || pg[1] != ppg[1] || pg[2] != ppg[2]) {
#pragma unroll
              for (int idx = 0; idx < 8; ++idx) reg[idx] = a.emb[tg_corner_entry(lv, a.d.grid_C, pg, idx, col)];
              ppg[0] = pg[0]; ppg[1] = pg[1]; ppg[2] = pg[2];
            }
            acc = tg_cell_interp(reg, fr, wt);
          }
        }
        acc += __shfl_xor(acc, 1, 64);  // column a + column b of this channel: a pair shares its segment
        if (have && ab == 0) frow[i * LDF] = oob ? 0.f : acc;
      }
    }
    __syncthreads();  // features (and, the first time, the weights) are in LDS
    // ---- phase 2: the net, one thread per sample ----
    for (int idx = threadIdx.x; idx < G * a.run; idx += TD_NT) {
      const int gg = idx / a.run, i = idx - gg * a.run;
      const int64_t sg = bt * G + gg;
      if (sg >= n_segs) continue;
      const int64_t r = sg / a.segs;
      const int s = (int)(sg - r * a.segs) * a.run + i;
      if (s >= S) continue;
      const float* x = feat + (gg * TD_RUN + i) * LDF;
      float h[TD_H];
#pragma unroll
      for (int j = 0; j < TD_H; ++j) h[j] = 0.f;
      for (int kk = 0; kk < LC; ++kk) {
        const float xk = x[kk];
        const float* w = W0s + kk * TD_H;
#pragma unroll
        for (int j = 0; j < TD_H; ++j) h[j] = fmaf(xk, w[j], h[j]);
      }
      float y = 0.f;
#pragma unroll
      for (int j = 0; j < TD_H; ++j) y = fmaf(fmaxf(h[j], 0.f), WOs[j], y);
      a.dens[r * S + s] = expf(y);  // trunc_exp forward (activations.py:32)
    }
    __syncthreads();  // the next batch overwrites the features
  }
}

static bool tgrid_density_shape_ok(const snerf_tgrid_desc* d, const snerf_mlp_desc* m) {
  return d && m && d->D == 3 && d->C == TD_C && d->L >= 1 && d->L * d->C <= TD_MAXF && d->grid_C > d->C + 1 && (d->gridtype == 0 || d->gridtype == 1) &&
         m->d_in == d->L * d->C && m->hidden == TD_H && m->n_hidden == 1 && m->d_out == 1 && m->hidden_act == 1 && m->out_act == 0 && m->operands == 0;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_tgrid_density_fwd_supported(const snerf_tgrid_desc* desc, const snerf_mlp_desc* net) { return tgrid_density_shape_ok(desc, net) ? 1 : 0; }

extern "C" int snerf_tgrid_density_fwd(const snerf_tgrid_desc* desc, const float* embeddings, const snerf_coords* coords, const float* times, int32_t S, int64_t N,
                                       const snerf_mlp_desc* net, const float* W, float* density, snerf_stream_t stream) {
  SNERF_REQUIRE(desc && coords && net, "tgrid_density_fwd: null descriptor");
  SNERF_REQUIRE(tgrid_density_shape_ok(desc, net), "tgrid_density_fwd: built for D = 3 tables of level_dim 2 with L * 2 <= %d features and the L*2 -> 16 -> 1 "
                "ReLU net with fp32 operands (D=%d C=%d L=%d grid_C=%d; net %d -> %d x %d -> %d, hidden_act %d, out_act %d, operands %d)", TD_MAXF, desc->D,
                desc->C, desc->L, desc->grid_C, net->d_in, net->hidden, net->n_hidden, net->d_out, net->hidden_act, net->out_act, net->operands);
  SNERF_REQUIRE(coords->mode == 1, "tgrid_density_fwd: coords.mode=%d: samples are derived from rays (mode 1)", coords->mode);
  SNERF_REQUIRE(coords->contract == 0, "tgrid_density_fwd: coords.contract=%d: the table encoders have no scene contraction", coords->contract);
  SNERF_REQUIRE(S >= 1 && coords->S == S && N >= 0 && N < (1LL << 31) && N % S == 0, "tgrid_density_fwd: S=%d coords.S=%d N=%lld", S, coords->S, (long long)N);
  if (N == 0) return 0;
  SNERF_REQUIRE(coords->origins && coords->dirs && coords->ebins, "tgrid_density_fwd: incomplete ray coordinates");
  SNERF_REQUIRE(embeddings && times && W && density, "tgrid_density_fwd: null buffer");
  TgridDensityArgs a = {};
  a.d = *desc; a.c = *coords; a.emb = embeddings; a.times = times; a.W = W; a.dens = density; a.R = N / S;
  a.segs = (S + TD_RUN - 1) / TD_RUN;
  a.run = (S + a.segs - 1) / a.segs;
  const int per = TD_NT / (desc->L * 2 * TD_C);
  a.G = per < TD_MAXG ? per : TD_MAXG;
  const int64_t n_batches = (a.R * a.segs + a.G - 1) / a.G;
  const int64_t grid = n_batches < 256 * 8 ? n_batches : 256 * 8;
  hipLaunchKernelGGL(tgrid_density_kernel, dim3((unsigned)grid), dim3(TD_NT), (size_t)td_lds_floats(a.G, desc->L * TD_C) * sizeof(float), (hipStream_t)stream, a, n_batches);
  SNERF_LAUNCH_CHECK("tgrid_density_fwd");
  return 0;
}
