// Temporal hash grid, backward w.r.t. the table in OWNER-COMPUTES form (round 6), optionally with the optimiser step of the table fused in.
//
// What it replaces: NS/field_components/cuda/csrc/temporal_gridencoder.cu:283-370 (kernel_grid_backward: one atomicAdd per sample, level, corner and
// live column) followed by torch.optim.Adam over the dense table (NS/configs/method_configs.py:648-657) and, in between, the temporal-TV gradient of two
// columns (NS/field_components/temporal_grid.py:352-376).
//
// Why: on camera rays tgrid_runs_kernel<true> (tgrid.hip) already runs AT the chip-wide rate of memory-side float atomics -- 22 M 64-B atomic requests of
// 12 useful bytes each in 1.26 ms for config 4's main grid (profiles/r06_tgrid_levels.json) -- and above the coarsest levels no two samples share a cell
// (196 608 samples -> 196 5xx distinct cells per level from level 11 on), so combining across rays cannot remove requests.  What can go is the atomic
// itself: every table row gets ONE owner.
//
//   1. bin (count, two scans, fill): every (sample, level, corner pair) is filed under the TILE of 2^k consecutive table rows its corner rows fall into
//      -- a counting sort with one LDS histogram per (sample chunk, level) workgroup and NO global atomics (per-chunk counts go into a [chunks, tiles]
//      matrix whose column prefix sums are the write offsets).  A record is 4 bytes: sample index, which (y, z) corner pair, which of its two x corners.
//   2. tiles: one workgroup per tile holds the tile's gradient rows in LDS (256 rows x 66 columns x 4 B = 67.6 KB: two workgroups per CU), walks the
//      tile's records (re-deriving cell, weights and the <= C + 1 live columns from the ray and its time, exactly as the scatter kernels do), adds with
//      LDS atomics, and then either
//        MODE 0: adds the tile into the dense gradient buffer with plain loads / stores (it is the only writer of those rows), or
//        MODE 1: runs Adam for its rows straight from LDS -- p, m, v are read and written once, the dense gradient buffer is not touched at all
//                (32 -> 24 B per parameter for the sweep, and the scatter's read-modify-write traffic is gone).
//
// The coarsest levels (few rows, thousands of samples per row: one tile would receive 10^4..10^5 records) stay with the run-length atomic kernel, where
// consecutive samples of a ray share cells and requests are few; in MODE 1 their tiles read (and clear) what that kernel left in the gradient buffer.
//
// Binning, the record walk and the MODE 0 epilogue are table_tiles_common.hpp's (shared with hashgrid_tiles.hip); this file holds what is the temporal grid's
// own: the positions pass, the <= C + 1 live time columns of a corner, the temporal-TV rows and the pipelined MODE 1 epilogue.
#include "plane_adam_common.hpp"  // adam_float4, ldnt4 / stnt4: compiled with the optimiser sweep's own contraction setting
#include "tgrid_common.hpp"       // no contraction from here on: cells and weights exactly as tgrid.hip derives them
#include "table_tiles_common.hpp"

namespace snerf {

struct TileArgs : TileCoreArgs {
  snerf_tgrid_desc d;
  snerf_coords c;
  const float* times;
  int spr;
  float4* pos4;        // [B]: (x, y, z in [0,1]^3 as tg_sample_x derives them, time) -- written by the binning entry, read by every later pass, so that the
                       // tile kernels never touch the caller's ray buffers (they may run on another stream while the next step's head rewrites those)
  float* gemb;         // MODE 0: accumulated into; MODE 1: optional contribution of the coarse levels (read and cleared)
  float* p; float* m; float* v;
  float step_size, b1, b2, inv_sqrt_bc2, eps;
  int col_a, col_b;    // temporal-TV columns (MODE 1; col_a < 0: none)
  const float* srow;   // [rows]: signed TV step per table row
};

// the temporal grid's tile policy (table_tiles_common.hpp)
template <int C>
struct TgTiles {
  TileArgs a;
  __host__ __device__ int levels() const { return a.d.L; }
  __host__ __device__ int row_floats() const { return a.d.grid_C; }
  __device__ __forceinline__ TableLevel level(int l) const { return tg_level(a.d, l, 3); }

  __device__ __forceinline__ bool cell(const TableLevel& lv, int l, int64_t b, uint32_t pg[3], float fr[3]) const {
    const float4 ps = a.pos4[b];
    const float x[3] = {ps.x, ps.y, ps.z};
    if ((x[0] < 0.f) || (x[0] > 1.f) || (x[1] < 0.f) || (x[1] > 1.f) || (x[2] < 0.f) || (x[2] > 1.f)) return false;  // .cu:119-124
    if (tile_gradient_is_zero<C>(a, a.d.L, l, b)) return false;
    tg_cell(lv, a.d.align_corners != 0, x, 3, pg, fr);
    return true;
  }

  struct Rec {
    uint32_t rec;
    float4 ps;  // the sample's pos4, requested one record ahead as well
  };
  __device__ __forceinline__ Rec fetch(int i) const {
    const uint32_t rec = a.records[i];
    return {rec, a.pos4[rec >> 4]};
  }

  struct Sample {
    float g[C];
    int r, pch;         // time row and the channel that blends two columns there
    float wa_p, wb_p;   // tg_slot_from_time: the blending channel's two weights
  };
  __device__ __forceinline__ Sample sample(const Rec& rc, const TableLevel& lv, int l, uint32_t pg[3], float fr[3]) const {
    const float x[3] = {rc.ps.x, rc.ps.y, rc.ps.z};
    tg_cell(lv, a.d.align_corners != 0, x, 3, pg, fr);
    const int n_trows = a.d.grid_C - C - 1;
    const float t = rc.ps.w;
    const float tv = t * (float)(n_trows - 1);
    Sample s;
    s.r = (int)tv;
    if (t == 1.f) s.r = n_trows - 1;
    s.pch = s.r % C;
    s.wa_p = (float)(s.r + 1) - tv;
    s.wb_p = tv - (float)s.r;
    const float* g = a.gout + (int64_t)(rc.rec >> 4) * (a.d.L * C) + l * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) s.g[ch] = g[ch];
    return s;
  }
  // one corner spreads over the <= C + 1 live time columns of its row
  __device__ __forceinline__ void add(const Sample& s, float* rowp, float w) const {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const int occ = s.r > ch ? C + ch + C * ((s.r - 1 - ch) / C) : ch;
      const float wt = ch == s.pch ? s.wa_p : 1.f;
      if (wt != 0.f) {
        const float val = w * (s.g[ch] * wt);
        if (val != 0.f) atomicAdd(rowp + occ, val);
      }
      if (ch == s.pch && s.wb_p != 0.f) {
        const float val = w * (s.g[ch] * s.wb_p);
        if (val != 0.f) atomicAdd(rowp + C + s.r, val);
      }
    }
  }
};

__global__ __launch_bounds__(256) void tt_positions_kernel(TileArgs a) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  float x[3];
  tg_sample_x(a.c, b, x);
  a.pos4[b] = make_float4(x[0], x[1], x[2], a.times[(uint32_t)b / (uint32_t)a.spr]);
}

// MODE 0: dense gradient += tile; MODE 1: Adam (+ temporal TV) for the tile's rows
template <int C, int MODE>
__global__ __launch_bounds__(TILE_NT) void tt_tiles_kernel(TgTiles<C> pol) {
  extern __shared__ float tt_acc[];
  const TileArgs& a = pol.a;
  const int tile = (int)blockIdx.x + a.tile0;
  TableLevel lv;
  const TileSpan s = tile_span(pol, tile, lv);
  const int gc = a.d.grid_C;
  const int64_t gb = s.gb, ge = s.ge, q0 = s.q0;
  const int nq = s.nq, ph = s.ph;
  // the float4 groups that lie wholly inside the tile: [qa, qb)
  const int qa = ph ? 1 : 0, qb = nq - ((ge & 3) ? 1 : 0);
  const bool coarse = s.level < a.pl.first_tiled_level;  // its gradient came through the atomic kernel into gemb
  // MODE 1, streaming part (below), software-pipelined: TT_U groups per thread and stage, the next stage's 3 x TT_U loads in flight while this one is
  // computed and stored; the FIRST stage is requested here, in front of the record walk, so that the memory system works while the tile is being summed
  constexpr int TT_U = 2;
  constexpr int STRIDE = TT_U * TILE_NT;
  float4 PA[TT_U], MA[TT_U], VA[TT_U], PB[TT_U], MB[TT_U], VB[TT_U];
  auto load = [&](float4* P, float4* M, float4* V, int qbase) {
#pragma unroll
    for (int u = 0; u < TT_U; ++u) {
      const int q = qbase + u * TILE_NT;
      if (q < qb) {
        const int64_t f0 = (q0 + q) << 2;
        P[u] = ldnt4(a.p + f0); M[u] = ldnt4(a.m + f0); V[u] = ldnt4(a.v + f0);
      }
    }
  };
  const bool stream = MODE == 1 && !(coarse && a.gemb);
  int cur = qa + (int)threadIdx.x;
  if (stream) load(PA, MA, VA, cur);

  // ---- the tile's records: this thread's first record and its position are requested before the LDS image is cleared (two dependent round trips) ----
  TileWalk<TgTiles<C>> walk = tile_walk_begin(pol, tile);
  tile_clear(tt_acc, nq);
  lds_barrier();
  tile_walk(pol, walk, s, lv, tt_acc);
  if (MODE == 1 && a.col_a >= 0) {
    // temporal TV (temporal_grid.py:352-376): srow[row] = weight / rows * sign(E[row, a] - E[row, b]) from the OLD table (tgrid_tv_sign_kernel); added with
    // LDS atomics like the records' terms, in the same phase (no barrier of its own)
    for (uint32_t lr = threadIdx.x; lr < s.nrows; lr += TILE_NT) {
      const float sv = a.srow[(int64_t)lv.off0 + s.row0 + lr];
      if (sv != 0.f) {
        atomicAdd(tt_acc + ph + (int)lr * gc + a.col_a, sv);
        atomicAdd(tt_acc + ph + (int)lr * gc + a.col_b, -sv);
      }
    }
  }
  lds_barrier();

  if (MODE == 0) {
    tile_accumulate(s, tt_acc, a.gemb);
    return;
  }
  // ---- MODE 1 epilogue over the float4 groups; a group that straddles the tile's first / last float is handled element by element ----
  const DynConsts dc = {a.step_size, a.inv_sqrt_bc2, 0};
  if (!stream) {
    for (int q = qa + (int)threadIdx.x; q < qb; q += TILE_NT) {
      const int64_t f0 = (q0 + q) << 2;
      const float4 gq = *reinterpret_cast<const float4*>(tt_acc + 4 * q);
      float4 pp = ldnt4(a.p + f0), mm = ldnt4(a.m + f0), vv = ldnt4(a.v + f0);
      const float4 extra = ldnt4(a.gemb + f0);
      if (extra.x != 0.f || extra.y != 0.f || extra.z != 0.f || extra.w != 0.f) stnt4(a.gemb + f0, make_float4(0.f, 0.f, 0.f, 0.f));
      adam_float4(pp, mm, vv, gq, extra, 1.f, a.b1, a.b2, a.eps, dc);
      stnt4(a.p + f0, pp);
      stnt4(a.m + f0, mm);
      stnt4(a.v + f0, vv);
    }
  } else {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    auto step = [&](float4* P, float4* M, float4* V, int qbase) {
#pragma unroll
      for (int u = 0; u < TT_U; ++u) {
        const int q = qbase + u * TILE_NT;
        if (q < qb) {
          const int64_t f0 = (q0 + q) << 2;
          const float4 gq = *reinterpret_cast<const float4*>(tt_acc + 4 * q);
          adam_float4(P[u], M[u], V[u], gq, zero, 1.f, a.b1, a.b2, a.eps, dc);
          stnt4(a.p + f0, P[u]);
          stnt4(a.m + f0, M[u]);
          stnt4(a.v + f0, V[u]);
        }
      }
    };
    while (cur < qb) {
      load(PB, MB, VB, cur + STRIDE);
      step(PA, MA, VA, cur);
      cur += STRIDE;
      if (cur >= qb) break;
      load(PA, MA, VA, cur + STRIDE);
      step(PB, MB, VB, cur);
      cur += STRIDE;
    }
  }
  // the (at most two) groups shared with a neighbouring tile: element by element, this tile's floats only
  if (threadIdx.x < 2) {
    const int q = threadIdx.x == 0 ? 0 : nq - 1;
    const bool partial = threadIdx.x == 0 ? (qa == 1) : (qb == nq - 1 && nq - 1 >= qa);
    if (partial && (threadIdx.x == 0 || nq > 1 || qa == 0)) {
      const int64_t f0 = (q0 + q) << 2;
      const float4 gq = *reinterpret_cast<const float4*>(tt_acc + 4 * q);
      float4 pp = make_float4(0.f, 0.f, 0.f, 0.f), mm = pp, vv = pp, extra = pp;
      float* P = &pp.x; float* M = &mm.x; float* V = &vv.x; float* E = &extra.x;
      for (int k = 0; k < 4; ++k)
        if (f0 + k >= gb && f0 + k < ge) {
          P[k] = a.p[f0 + k]; M[k] = a.m[f0 + k]; V[k] = a.v[f0 + k];
          if (coarse && a.gemb) { E[k] = a.gemb[f0 + k]; if (E[k] != 0.f) a.gemb[f0 + k] = 0.f; }
        }
      adam_float4(pp, mm, vv, gq, extra, 1.f, a.b1, a.b2, a.eps, dc);
      for (int k = 0; k < 4; ++k)
        if (f0 + k >= gb && f0 + k < ge) { a.p[f0 + k] = P[k]; a.m[f0 + k] = M[k]; a.v[f0 + k] = V[k]; }
    }
  }
}

static int tiles_lds_bytes(const snerf_tgrid_desc* d, int sh) { return (((1 << sh) * d->grid_C + 6) / 4 + 1) * 16; }

static int validate_tiles(const snerf_tgrid_desc* d, const snerf_tgrid_tile_plan* pl, int64_t B) {
  SNERF_REQUIRE(d && pl, "tgrid tiles: null descriptor");
  SNERF_REQUIRE(d->D == 3, "tgrid tiles: D=%d (3 only)", d->D);
  SNERF_REQUIRE(d->C == 1 || d->C == 2 || d->C == 4 || d->C == 8, "tgrid tiles: level_dim C=%d unsupported (1,2,4,8)", d->C);
  SNERF_REQUIRE(d->L >= 1 && d->L <= 32 && d->grid_C > d->C + 1 && (d->grid_C & 1) == 0, "tgrid tiles: L=%d grid_C=%d (even row length needed)", d->L, d->grid_C);
  return tile_plan_check("tgrid", tile_plan_from(*pl), d->L, B, 2);
}

template <int C>
static int bin_launch(const TileArgs& a, hipStream_t st) {
  if (a.B > 0) hipLaunchKernelGGL(tt_positions_kernel, dim3((unsigned)ceil_div(a.B, 256)), dim3(256), 0, st, a);
  return tile_bin_launch(TgTiles<C>{a}, st, "tgrid_bwd_bin");
}

template <int C, int MODE>
static int tiles_launch(const TileArgs& a, hipStream_t st) {
  TgTiles<C> pol{a};
  return tile_launch<TgTiles<C>, tt_tiles_kernel<C, MODE>, MODE>(pol, tiles_lds_bytes(&a.d, a.pl.tile_rows_log2), st, MODE == 0 ? "tgrid_bwd_tiles" : "tgrid_bwd_tiles_adam");
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_tgrid_tile_plan_make(const snerf_tgrid_desc* desc, int64_t B, int32_t tile_rows_log2, int32_t first_tiled_level,
                                          snerf_tgrid_tile_plan* plan) {
  SNERF_REQUIRE(desc && plan, "tgrid_tile_plan_make: null argument");
  SNERF_REQUIRE(desc->L >= 1 && desc->L <= 32 && desc->grid_C >= 2 && B >= 0, "tgrid_tile_plan_make: L=%d grid_C=%d B=%lld", desc->L, desc->grid_C, (long long)B);
  // automatic tile: the largest whose LDS image lets two workgroups share a CU's 160 KB; levels with fewer than 2^16 rows (the coarsest dense ones: 10^4..10^5
  // records per tile) stay with the run-length atomic kernel
  const TilePlanRules rules = {2, 16, 72 * 1024, 1 << 16};
  TilePlan p;
  int rc = tile_plan_make("tgrid", desc->offsets, desc->L, B, tile_rows_log2, first_tiled_level, rules, [&](int sh) { return tiles_lds_bytes(desc, sh); }, &p);
  if (rc) return rc;
  tile_plan_to(p, plan);
  return 0;
}

extern "C" int snerf_tgrid_bwd_bin(const snerf_tgrid_desc* desc, const snerf_tgrid_tile_plan* plan, const snerf_coords* coords, const float* times,
                                   int32_t samples_per_row, int64_t B, const float* grad_out, float* pos4, int32_t* counts, int32_t* tile_base,
                                   uint32_t* records, snerf_stream_t stream) {
  int rc = validate_tiles(desc, plan, B);
  if (rc) return rc;
  SNERF_REQUIRE(coords && times && samples_per_row >= 1, "tgrid_bwd_bin: coords / times / samples_per_row");
  SNERF_REQUIRE(coords->mode == 0 || coords->mode == 1, "tgrid_bwd_bin: coords.mode=%d", coords->mode);
  SNERF_REQUIRE(coords->contract == 0, "tgrid_bwd_bin: coords.contract=%d: the table encoders have no scene contraction", coords->contract);
  if (coords->mode == 0) SNERF_REQUIRE(coords->pts || B == 0, "tgrid_bwd_bin: pts is null");
  if (coords->mode == 1) SNERF_REQUIRE(coords->S >= 1 && B % coords->S == 0 && coords->origins && coords->dirs && coords->ebins, "tgrid_bwd_bin: bad ray coords");
  SNERF_REQUIRE(counts && tile_base && (pos4 || B == 0) && (records || plan->record_capacity == 0), "tgrid_bwd_bin: null buffer");
  SNERF_REQUIRE(((uintptr_t)pos4 & 15) == 0, "tgrid_bwd_bin: pos4 must be 16-byte aligned");
  TileArgs a = {};
  a.d = *desc; a.c = *coords; a.pl = tile_plan_from(*plan); a.times = times; a.spr = samples_per_row; a.B = B; a.gout = grad_out;
  a.pos4 = reinterpret_cast<float4*>(pos4); a.counts = counts; a.tile_base = tile_base; a.records = records;
#define TT_CALL(C_) bin_launch<C_>(a, (hipStream_t)stream)
  TILE_DISPATCH_1248(desc->C, TT_CALL)
#undef TT_CALL
}

extern "C" int snerf_tgrid_bwd_tiles(const snerf_tgrid_desc* desc, const snerf_tgrid_tile_plan* plan, int64_t B, const float* grad_out, const float* pos4,
                                     const int32_t* tile_base, const uint32_t* records, float* grad_embeddings, snerf_stream_t stream) {
  int rc = validate_tiles(desc, plan, B);
  if (rc) return rc;
  if (B == 0) return 0;
  SNERF_REQUIRE(tile_base && records && grad_out && pos4 && grad_embeddings, "tgrid_bwd_tiles: null buffer");
  SNERF_REQUIRE((((uintptr_t)grad_embeddings | (uintptr_t)pos4) & 15) == 0, "tgrid_bwd_tiles: grad_embeddings / pos4 must be 16-byte aligned");
  TileArgs a = {};
  a.d = *desc; a.pl = tile_plan_from(*plan); a.B = B; a.gout = grad_out; a.pos4 = reinterpret_cast<float4*>(const_cast<float*>(pos4));
  a.tile_base = const_cast<int32_t*>(tile_base); a.records = const_cast<uint32_t*>(records); a.gemb = grad_embeddings;
  a.col_a = -1;
#define TT_CALL(C_) tiles_launch<C_, 0>(a, (hipStream_t)stream)
  TILE_DISPATCH_1248(desc->C, TT_CALL)
#undef TT_CALL
}

extern "C" int snerf_tgrid_bwd_tiles_adam(const snerf_tgrid_desc* desc, const snerf_tgrid_tile_plan* plan, int64_t B, const float* grad_out, const float* pos4,
                                          int32_t* tile_base, const uint32_t* records, float* grad_embeddings, float* p, float* m, float* v, float lr,
                                          float beta1, float beta2, float eps, int32_t step, int32_t col_a, int32_t col_b, const float* srow,
                                          snerf_stream_t stream) {
  int rc = validate_tiles(desc, plan, B);
  if (rc) return rc;
  SNERF_REQUIRE(tile_base && (records || B == 0) && (grad_out || B == 0) && (pos4 || B == 0) && p && m && v, "tgrid_bwd_tiles_adam: null buffer");
  SNERF_REQUIRE(step >= 1, "tgrid_bwd_tiles_adam: step=%d (1-based)", step);
  SNERF_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)grad_embeddings | (uintptr_t)pos4) & 15) == 0,
                "tgrid_bwd_tiles_adam: buffers must be 16-byte aligned");
  SNERF_REQUIRE(plan->first_tiled_level == 0 || grad_embeddings, "tgrid_bwd_tiles_adam: levels [0, %d) go through the atomic kernel: pass their gradient buffer",
                plan->first_tiled_level);
  SNERF_REQUIRE(col_a < 0 || (srow && col_b >= 0 && col_a < desc->grid_C && col_b < desc->grid_C && col_a != col_b), "tgrid_bwd_tiles_adam: TV columns (%d,%d)", col_a,
                col_b);
  TileArgs a = {};
  a.d = *desc; a.pl = tile_plan_from(*plan); a.B = B; a.gout = grad_out; a.pos4 = reinterpret_cast<float4*>(const_cast<float*>(pos4));
  a.tile_base = tile_base; a.records = const_cast<uint32_t*>(records); a.gemb = grad_embeddings;
  a.p = p; a.m = m; a.v = v; a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  adam_consts(lr, beta1, beta2, step, a.step_size, a.inv_sqrt_bc2);
  a.col_a = col_a; a.col_b = col_b; a.srow = srow;
#define TT_CALL(C_) tiles_launch<C_, 1>(a, (hipStream_t)stream)
  TILE_DISPATCH_1248(desc->C, TT_CALL)
#undef TT_CALL
}
