// Static hash grid (the full NeRFPlayer's "stationary field"), backward w.r.t. the table in OWNER-COMPUTES form with the optimiser step fused in (round 6).
//
// What it replaces: the table half of tcnn's HashGrid backward (Mueller et al. 2022, grid.h kernel_grid_backward: one atomicAdd per sample, level, corner and
// feature; tiny-cuda-nn v1.6 is an un-vendored dependency of the reference, NS/fields/nerfplayer_field.py:242-252) followed by torch.optim.Adam over the table
// (NS/configs/method_configs.py:598-607).  hashgrid_kernel<F, true, 1> (hashgrid.hip) runs at the chip's float-atomic request rate: 2 x 196 608 points x 16
// levels x 4..8 requests = 1.7 ms per step of the full NeRFPlayer.  Same construction as tgrid_tiles.hip: the batch's (point, level, corner pair) touches are
// filed under tiles of 2^k consecutive table rows by a counting sort without global atomics; one workgroup per tile sums its rows in LDS (ds_add_f32) and runs
// Adam over them from there (MODE 1: no dense gradient for this table) or adds them into the dense gradient with plain stores (MODE 0).  The coordinate gradient
// (the deformation net's input) stays with hashgrid_kernel, called without a table gradient: it is a gather.
#include "plane_adam_common.hpp"  // adam_float4, ldnt4 / stnt4: compiled with the optimiser sweep's own contraction setting
#include "hashgrid_common.hpp"     // ht_level, ht_cell: the level and cell that hashgrid.hip derives too
#include "table_tiles_common.hpp"  // no contraction from here on

namespace snerf {

struct HtArgs : TileCoreArgs {
  snerf_hashgrid_desc d;
  const float* x;      // [B, 3]
  float* gtable;       // MODE 0: accumulated into; MODE 1: the coarse (atomic) levels' contribution, read and cleared (may be null when every level is tiled)
  float* p; float* m; float* v;
  float step_size, b1, b2, inv_sqrt_bc2, eps;
};

// the static hash grid's tile policy (table_tiles_common.hpp)
template <int F>
struct HtTiles {
  HtArgs a;
  __host__ __device__ int levels() const { return a.d.L; }
  __host__ __device__ int row_floats() const { return F; }
  __device__ __forceinline__ TableLevel level(int l) const { return ht_level(a.d, l, 3); }

  __device__ __forceinline__ bool cell(const TableLevel& lv, int l, int64_t b, uint32_t pg[3], float fr[3]) const {
    if (tile_gradient_is_zero<F>(a, a.d.L, l, b)) return false;
    const float x[3] = {a.x[b * 3], a.x[b * 3 + 1], a.x[b * 3 + 2]};  // no bounds check on coordinates, as tcnn
    ht_cell(lv, x, 3, pg, fr);
    return true;
  }

  struct Rec { uint32_t rec; };
  __device__ __forceinline__ Rec fetch(int i) const { return {a.records[i]}; }

  struct Sample { float g[F]; };
  __device__ __forceinline__ Sample sample(const Rec& rc, const TableLevel& lv, int l, uint32_t pg[3], float fr[3]) const {
    const int64_t b = (int64_t)(rc.rec >> 4);
    const float x[3] = {a.x[b * 3], a.x[b * 3 + 1], a.x[b * 3 + 2]};
    ht_cell(lv, x, 3, pg, fr);
    const float* gp = a.gout + b * (a.d.L * F) + l * F;
    Sample s;
#pragma unroll
    for (int f = 0; f < F; ++f) s.g[f] = gp[f];
    return s;
  }
  __device__ __forceinline__ void add(const Sample& s, float* rowp, float w) const {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const float val = w * s.g[f];
      if (val != 0.f) atomicAdd(rowp + f, val);
    }
  }
};

// MODE 0: dense gradient += tile; MODE 1: Adam for the tile's rows
template <int F, int MODE>
__global__ __launch_bounds__(TILE_NT) void ht_tiles_kernel(HtTiles<F> pol) {
  extern __shared__ float ht_acc[];
  const HtArgs& a = pol.a;
  const int tile = (int)blockIdx.x + a.tile0;
  TableLevel lv;
  const TileSpan s = tile_span(pol, tile, lv);  // a whole number of float4 groups (ph = 0): levels and tiles are multiples of 8 rows
  const bool coarse = s.level < a.pl.first_tiled_level;  // its gradient came through the atomic kernel into gtable
  TileWalk<HtTiles<F>> walk = tile_walk_begin(pol, tile);
  tile_clear(ht_acc, s.nq);
  lds_barrier();
  tile_walk(pol, walk, s, lv, ht_acc);
  lds_barrier();
  if (MODE == 0) {
    tile_accumulate(s, ht_acc, a.gtable);
    return;
  }
  const DynConsts dc = {a.step_size, a.inv_sqrt_bc2, 0};
  for (int q = threadIdx.x; q < s.nq; q += TILE_NT) {
    const int64_t f0 = s.gb + 4 * (int64_t)q;
    const float4 gq = *reinterpret_cast<const float4*>(ht_acc + 4 * q);
    float4 pp = ldnt4(a.p + f0), mm = ldnt4(a.m + f0), vv = ldnt4(a.v + f0);
    float4 extra = make_float4(0.f, 0.f, 0.f, 0.f);
    if (coarse && a.gtable) {
      extra = ldnt4(a.gtable + f0);
      if (extra.x != 0.f || extra.y != 0.f || extra.z != 0.f || extra.w != 0.f) stnt4(a.gtable + f0, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    adam_float4(pp, mm, vv, gq, extra, 1.f, a.b1, a.b2, a.eps, dc);
    stnt4(a.p + f0, pp);
    stnt4(a.m + f0, mm);
    stnt4(a.v + f0, vv);
  }
}

static int ht_lds_bytes(const snerf_hashgrid_desc* d, int sh) { return (1 << sh) * d->F * 4; }

static int ht_validate(const snerf_hashgrid_desc* d, const snerf_hashgrid_tile_plan* pl, int64_t B) {
  SNERF_REQUIRE(d && pl, "hashgrid tiles: null descriptor");
  SNERF_REQUIRE(d->D == 3, "hashgrid tiles: D=%d (3 only)", d->D);
  SNERF_REQUIRE(d->F == 1 || d->F == 2 || d->F == 4 || d->F == 8, "hashgrid tiles: F=%d", d->F);
  SNERF_REQUIRE(d->L >= 1 && d->L <= 32 && d->offsets[d->L] > 0, "hashgrid tiles: descriptor not laid out");
  return tile_plan_check("hashgrid", tile_plan_from(*pl), d->L, B, 3);
}

template <int F, int MODE>
static int ht_tiles_launch(const HtArgs& a, hipStream_t st) {
  HtTiles<F> pol{a};
  return tile_launch<HtTiles<F>, ht_tiles_kernel<F, MODE>, MODE>(pol, ht_lds_bytes(&a.d, a.pl.tile_rows_log2), st, MODE == 0 ? "hashgrid_bwd_tiles" : "hashgrid_bwd_tiles_adam");
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_hashgrid_tile_plan_make(const snerf_hashgrid_desc* desc, int64_t B, int32_t tile_rows_log2, int32_t first_tiled_level,
                                             snerf_hashgrid_tile_plan* plan) {
  SNERF_REQUIRE(desc && plan, "hashgrid_tile_plan_make: null argument");
  SNERF_REQUIRE(desc->L >= 1 && desc->L <= 32 && desc->offsets[desc->L] > 0 && B >= 0, "hashgrid_tile_plan_make: descriptor not laid out / B=%lld", (long long)B);
  // automatic tile: 2^11 rows (fewer when the image would not fit 64 KB): a level of 2^19 rows is 256 tiles, so that a batch's ~4.5 records per (point, level)
  // spread over enough workgroups (a tile of 2^13 rows of the NeRFPlayer preset receives 27 k records: 54 dependent rounds of its 512 threads); levels with
  // fewer than 2^18 rows stay with the atomic kernel: every point of the batch lands in their few tiles (level 0 of the preset: 4096 rows)
  const TilePlanRules rules = {3, 11, 64 * 1024, 1 << 18};
  TilePlan p;
  int rc = tile_plan_make("hashgrid", desc->offsets, desc->L, B, tile_rows_log2, first_tiled_level, rules, [&](int sh) { return ht_lds_bytes(desc, sh); }, &p);
  if (rc) return rc;
  tile_plan_to(p, plan);
  return 0;
}

extern "C" int snerf_hashgrid_bwd_bin(const snerf_hashgrid_desc* desc, const snerf_hashgrid_tile_plan* plan, const float* x, int64_t B, const float* grad_out,
                                      int32_t* counts, int32_t* tile_base, uint32_t* records, snerf_stream_t stream) {
  int rc = ht_validate(desc, plan, B);
  if (rc) return rc;
  SNERF_REQUIRE(counts && tile_base && (records || B == 0) && (x || B == 0), "hashgrid_bwd_bin: null buffer");
  HtArgs a = {};
  a.d = *desc; a.pl = tile_plan_from(*plan); a.x = x; a.B = B; a.gout = grad_out; a.counts = counts; a.tile_base = tile_base; a.records = records;
#define HT_CALL(F_) tile_bin_launch(HtTiles<F_>{a}, (hipStream_t)stream, "hashgrid_bwd_bin")
  TILE_DISPATCH_1248(desc->F, HT_CALL)
#undef HT_CALL
}

extern "C" int snerf_hashgrid_bwd_tiles(const snerf_hashgrid_desc* desc, const snerf_hashgrid_tile_plan* plan, const float* x, int64_t B, const float* grad_out,
                                        const int32_t* tile_base, const uint32_t* records, float* grad_table, snerf_stream_t stream) {
  int rc = ht_validate(desc, plan, B);
  if (rc) return rc;
  if (B == 0) return 0;
  SNERF_REQUIRE(tile_base && records && x && grad_out && grad_table && ((uintptr_t)grad_table & 15) == 0, "hashgrid_bwd_tiles: null / misaligned buffer");
  HtArgs a = {};
  a.d = *desc; a.pl = tile_plan_from(*plan); a.x = x; a.B = B; a.gout = grad_out; a.tile_base = const_cast<int32_t*>(tile_base); a.records = const_cast<uint32_t*>(records);
  a.gtable = grad_table;
#define HT_CALL(F_) ht_tiles_launch<F_, 0>(a, (hipStream_t)stream)
  TILE_DISPATCH_1248(desc->F, HT_CALL)
#undef HT_CALL
}

extern "C" int snerf_hashgrid_bwd_tiles_adam(const snerf_hashgrid_desc* desc, const snerf_hashgrid_tile_plan* plan, const float* x, int64_t B, const float* grad_out,
                                             const int32_t* tile_base, const uint32_t* records, float* grad_table, float* p, float* m, float* v, float lr,
                                             float beta1, float beta2, float eps, int32_t step, snerf_stream_t stream) {
  int rc = ht_validate(desc, plan, B);
  if (rc) return rc;
  SNERF_REQUIRE(tile_base && (records || B == 0) && (x || B == 0) && (grad_out || B == 0) && p && m && v, "hashgrid_bwd_tiles_adam: null buffer");
  SNERF_REQUIRE(step >= 1 && (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)grad_table) & 15) == 0, "hashgrid_bwd_tiles_adam: step=%d (1-based) / 16-byte alignment", step);
  SNERF_REQUIRE(plan->first_tiled_level == 0 || grad_table, "hashgrid_bwd_tiles_adam: levels [0, %d) go through the atomic kernel: pass their gradient buffer", plan->first_tiled_level);
  HtArgs a = {};
  a.d = *desc; a.pl = tile_plan_from(*plan); a.x = x; a.B = B; a.gout = grad_out; a.tile_base = const_cast<int32_t*>(tile_base); a.records = const_cast<uint32_t*>(records);
  a.gtable = grad_table; a.p = p; a.m = m; a.v = v; a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  adam_consts(lr, beta1, beta2, step, a.step_size, a.inv_sqrt_bc2);
#define HT_CALL(F_) ht_tiles_launch<F_, 1>(a, (hipStream_t)stream)
  TILE_DISPATCH_1248(desc->F, HT_CALL)
#undef HT_CALL
}
