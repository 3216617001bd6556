// The owner-computes ("tiled") table backward, the part that does not depend on which table it is (tgrid_tiles.hip: temporal hash grid; hashgrid_tiles.hip:
// static hash grid; construction and reasons: the head of tgrid_tiles.hip).  A multi-level table is cut into tiles of 2^k consecutive rows;
//   bin:   every (sample, level, (y, z) corner pair) is filed under the tile its corner rows fall into -- a counting sort with one LDS histogram per (sample
//          chunk, level) workgroup and NO global atomics (per-chunk counts go into a [chunks, tiles] matrix whose column prefix sums are the write offsets);
//   tiles: one workgroup per tile walks the tile's records, re-derives cell and corner weights, and sums the tile's rows in LDS.
// A grid supplies a POLICY: a struct that the kernels take by value, holding the grid's arguments as member `a` (derived from TileCoreArgs), with
//   int levels(), int row_floats()               (host and device) levels of the table, floats per table row
//   TableLevel level(int l)
//   bool cell(lv, l, b, pg, fr)                  binning: cell and in-cell position of sample b at level l; false = the sample files nothing there
//   Rec fetch(int i)                             record i (Rec::rec) and whatever else the grid wants in flight one record ahead
//   Sample sample(rec, lv, l, pg, fr)            tile pass: the same cell from a fetched record, plus the sample's gradient (and time weights)
//   void add(sample, rowp, w)                    tile pass: the LDS adds of one live corner of weight w into its row's image
// Must be included AFTER plane_adam_common.hpp (adam_float4 keeps the optimiser sweep's contraction setting); everything here is evaluated as written, so
// that cells and weights match the scatter kernels bit for bit.
#pragma once
#include "table_level.hpp"

#pragma clang fp contract(off)

namespace snerf {

constexpr int TILE_NT = 512;                // threads of a tile workgroup
constexpr int TILE_BIN_NT = 256;            // threads of a binning workgroup
constexpr int TILE_MAX_LEVEL_TILES = 8192;  // LDS histogram of the binning kernels: 2 ints per tile of one level

// The plan, internally.  The two public structs hold these fields in different orders: copied field by field, never cast.
struct TilePlan {
  int32_t tile_rows_log2, n_tiles, n_chunks, chunk, first_tiled_level, lds_bytes;
  int32_t tile_start[33];
  int64_t count_ints, record_capacity;
};
template <typename PUB>
static TilePlan tile_plan_from(const PUB& s) {
  TilePlan p = {s.tile_rows_log2, s.n_tiles, s.n_chunks, s.chunk, s.first_tiled_level, s.lds_bytes, {}, s.count_ints, s.record_capacity};
  for (int l = 0; l < 33; ++l) p.tile_start[l] = s.tile_start[l];
  return p;
}
template <typename PUB>
static void tile_plan_to(const TilePlan& p, PUB* s) {
  s->tile_rows_log2 = p.tile_rows_log2; s->n_tiles = p.n_tiles; s->n_chunks = p.n_chunks; s->chunk = p.chunk;
  s->first_tiled_level = p.first_tiled_level; s->lds_bytes = p.lds_bytes; s->count_ints = p.count_ints; s->record_capacity = p.record_capacity;
  for (int l = 0; l < 33; ++l) s->tile_start[l] = p.tile_start[l];
}

// what every pass of either grid is handed
struct TileCoreArgs {
  TilePlan pl;
  int64_t B;
  const float* gout;   // [B, levels * channels per level]
  int32_t* counts;     // [n_chunks][n_tiles]: per-chunk record counts, then (scan) the chunk's write offset inside the tile
  int32_t* tile_base;  // [n_tiles + 1]
  uint32_t* records;
  int tile0;           // first tile of a tile-pass launch
};

// a grid's two defaults: the automatic tile size (the largest 2^k <= 2^auto_max_rows_log2 rows whose LDS image stays within auto_lds_bytes) and the row count
// below which a level stays with the atomic kernel
struct TilePlanRules {
  int min_rows_log2, auto_max_rows_log2, auto_lds_bytes, atomic_below_rows;
};

// offsets [L + 1]: first table row of each level; lds_of(k): LDS bytes of a tile of 2^k rows.  Host arithmetic only.
template <typename LDS>
static int tile_plan_make(const char* who, const int32_t* offsets, int L, int64_t B, int tile_rows_log2, int first_tiled_level, const TilePlanRules& r, LDS&& lds_of,
                          TilePlan* plan) {
  int64_t max_rows = 0;
  for (int l = 0; l < L; ++l) max_rows = offsets[l + 1] - offsets[l] > max_rows ? offsets[l + 1] - offsets[l] : max_rows;
  int sh = tile_rows_log2;
  if (sh <= 0) {
    sh = r.min_rows_log2;
    while (sh < r.auto_max_rows_log2 && lds_of(sh + 1) <= r.auto_lds_bytes) ++sh;
  }
  while (sh < 16 && ((max_rows + (1LL << sh) - 1) >> sh) > TILE_MAX_LEVEL_TILES) ++sh;  // no more tiles per level than the binning histogram holds
  SNERF_REQUIRE(sh >= r.min_rows_log2 && sh <= 16 && lds_of(sh) <= 156 * 1024, "%s_tile_plan_make: a tile of 2^%d rows does not fit LDS", who, sh);
  plan->tile_rows_log2 = sh;
  int t = 0;
  for (int l = 0; l < L; ++l) {
    plan->tile_start[l] = t;
    t += (int)((offsets[l + 1] - offsets[l] + (1LL << sh) - 1) >> sh);
  }
  for (int l = L; l < 33; ++l) plan->tile_start[l] = t;
  plan->n_tiles = t;
  plan->chunk = 4096;
  plan->n_chunks = (int)((B + plan->chunk - 1) / plan->chunk);
  int lc = first_tiled_level;
  if (lc < 0) {
    lc = 0;
    while (lc < L && offsets[lc + 1] - offsets[lc] < r.atomic_below_rows) ++lc;
  }
  plan->first_tiled_level = lc > L ? L : lc;
  plan->lds_bytes = lds_of(sh);
  plan->count_ints = (int64_t)(plan->n_chunks > 0 ? plan->n_chunks : 1) * plan->n_tiles;
  plan->record_capacity = B * (L - plan->first_tiled_level) * 8;
  return 0;
}

// does the plan belong to a table of L levels and a batch of B samples?
static int tile_plan_check(const char* who, const TilePlan& pl, int L, int64_t B, int min_rows_log2) {
  SNERF_REQUIRE(B >= 0 && B < (1LL << 28), "%s tiles: B=%lld (< 2^28)", who, (long long)B);
  SNERF_REQUIRE(pl.tile_rows_log2 >= min_rows_log2 && pl.tile_rows_log2 <= 16 && pl.n_tiles == pl.tile_start[L] && pl.chunk >= 1 &&
                    pl.n_chunks == (int)((B + pl.chunk - 1) / pl.chunk) && pl.first_tiled_level >= 0 && pl.first_tiled_level <= L,
                "%s tiles: the plan does not belong to this descriptor / batch (snerf_%s_tile_plan_make)", who, who);
  return 0;
}

// (sample, level) pairs whose gradient is all zero add nothing.  Binning may run before the gradient exists (grad_out = NULL: every sample is filed; a zero
// gradient then adds nothing in the tile pass).
template <int CH>
__device__ __forceinline__ bool tile_gradient_is_zero(const TileCoreArgs& a, int levels, int level, int64_t b) {
  if (!a.gout) return false;
  const float* g = a.gout + b * (levels * CH) + level * CH;
  bool any = false;
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) any |= g[ch] != 0.f;
  return !any;
}

// count (FILL = false) / fill (FILL = true): grid (chunks, tiled levels).  A record is 4 bytes: (sample << 4) | ((y, z) corner pair << 2) | which of its two
// x corners.
template <typename P, bool FILL>
__global__ __launch_bounds__(TILE_BIN_NT) void tile_bin_kernel(P p) {
  extern __shared__ int tile_hist[];
  const auto& a = p.a;
  const int level = (int)blockIdx.y + a.pl.first_tiled_level, chunk = (int)blockIdx.x;
  const int T0 = a.pl.tile_start[level], nt = a.pl.tile_start[level + 1] - T0;
  int* hist = tile_hist;
  int* base = tile_hist + nt;
  int32_t* mine = a.counts + (int64_t)chunk * a.pl.n_tiles + T0;
  for (int i = threadIdx.x; i < nt; i += TILE_BIN_NT) {
    hist[i] = 0;
    if (FILL) base[i] = a.tile_base[T0 + i] + mine[i];
  }
  __syncthreads();
  const TableLevel lv = p.level(level);
  const int64_t b0 = (int64_t)chunk * a.pl.chunk;
  const int64_t b1 = b0 + a.pl.chunk < a.B ? b0 + a.pl.chunk : a.B;
  auto emit = [&](uint32_t t, uint32_t rec) {
    const int rank = atomicAdd(&hist[t], 1);
    if (FILL) a.records[base[t] + rank] = rec;
  };
  for (int64_t b = b0 + threadIdx.x; b < b1; b += TILE_BIN_NT) {
    uint32_t pg[3];
    float fr[3];
    if (!p.cell(lv, level, b, pg, fr)) continue;
    // per (y, z) corner pair: its two x corners share a tile unless a tile boundary lies between their rows (hashed levels: rows r and r ^ 1 mostly), then
    // one record each
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
      const uint32_t cy = pg[1] + (uint32_t)(yz & 1), cz = pg[2] + (uint32_t)(yz >> 1);
      const uint32_t t0 = lv.row_of(pg[0], cy, cz) >> a.pl.tile_rows_log2, t1 = lv.row_of(pg[0] + 1u, cy, cz) >> a.pl.tile_rows_log2;
      const uint32_t rec = ((uint32_t)b << 4) | ((uint32_t)yz << 2);
      if (t0 == t1) emit(t0, rec | 3u);
      else { emit(t0, rec | 1u); emit(t1, rec | 2u); }
    }
  }
  if (!FILL) {
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += TILE_BIN_NT) mine[i] = hist[i];
  }
}

// per tile: counts[chunk][tile] -> the chunk's offset inside the tile (exclusive prefix over the chunks); totals[tile] = the tile's records
static __global__ __launch_bounds__(256) void tile_scan_chunks_kernel(int32_t* __restrict__ counts, int n_chunks, int n_tiles, int t_first, int32_t* __restrict__ totals) {
  const int t = t_first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n_tiles) return;
  int run = 0;
  for (int c = 0; c < n_chunks; ++c) {
    const int v = counts[(int64_t)c * n_tiles + t];
    counts[(int64_t)c * n_tiles + t] = run;
    run += v;
  }
  totals[t] = run;
}

// exclusive prefix over the tiles (one workgroup): tile_base[t] = records in front of tile t; tile_base[n_tiles] = all of them, the last word written.  In place.
static __global__ __launch_bounds__(1024) void tile_scan_tiles_kernel(int32_t* __restrict__ tile_base, int n_tiles, int t_first) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int t = tid; t < t_first; t += 1024) tile_base[t] = 0;  // tiles of the coarse (atomic) levels hold no records
  const int per = (n_tiles - t_first + 1023) / 1024;
  const int i0 = t_first + tid * per;
  int local = 0;
  for (int k = 0; k < per; ++k)
    if (i0 + k < n_tiles) local += tile_base[i0 + k];
  int incl = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int before = 0;
  for (int k = 0; k < w; ++k) before += wsum[k];
  int run = before + incl - local;
  for (int k = 0; k < per; ++k)
    if (i0 + k < n_tiles) {
      const int v = tile_base[i0 + k];
      tile_base[i0 + k] = run;
      run += v;
    }
  if (tid == 1023) {
    int total = 0;
    for (int k = 0; k < 16; ++k) total += wsum[k];
    tile_base[n_tiles] = total;
  }
}

// count, two scans, fill -- or, with no level to tile or no sample, the scan alone (every tile_base word becomes zero)
template <typename P>
static int tile_bin_launch(const P& p, hipStream_t st, const char* what) {
  const auto& a = p.a;
  const int L = p.levels(), Lc = a.pl.first_tiled_level;
  if (Lc >= L || a.B == 0) {
    hipLaunchKernelGGL(tile_scan_tiles_kernel, dim3(1), dim3(1024), 0, st, a.tile_base, a.pl.n_tiles, a.pl.n_tiles);
    SNERF_LAUNCH_CHECK(what);
    return 0;
  }
  int max_nt = 0;
  for (int l = Lc; l < L; ++l) max_nt = a.pl.tile_start[l + 1] - a.pl.tile_start[l] > max_nt ? a.pl.tile_start[l + 1] - a.pl.tile_start[l] : max_nt;
  const size_t lds = (size_t)max_nt * 2 * sizeof(int);
  const dim3 grid((unsigned)a.pl.n_chunks, (unsigned)(L - Lc));
  const int t_first = a.pl.tile_start[Lc];
  hipLaunchKernelGGL((tile_bin_kernel<P, false>), grid, dim3(TILE_BIN_NT), lds, st, p);
  hipLaunchKernelGGL(tile_scan_chunks_kernel, dim3((unsigned)ceil_div(a.pl.n_tiles - t_first, 256)), dim3(256), 0, st, a.counts, a.pl.n_chunks, a.pl.n_tiles, t_first,
                     a.tile_base);
  hipLaunchKernelGGL(tile_scan_tiles_kernel, dim3(1), dim3(1024), 0, st, a.tile_base, a.pl.n_tiles, t_first);
  hipLaunchKernelGGL((tile_bin_kernel<P, true>), grid, dim3(TILE_BIN_NT), lds, st, p);
  SNERF_LAUNCH_CHECK(what);
  return 0;
}

// ---- the tile pass: what a grid's tile kernel is put together from ----

// a tile's place: its level, its rows [row0, row0 + nrows) of that level, its floats [gb, ge) of the table and the float4 groups [q0, q0 + nq) that overlap
// them -- the first / last group may belong to a neighbouring tile in part when a row is no multiple of 4 floats; ph = the tile's first float inside group q0
struct TileSpan {
  int level;
  uint32_t row0, nrows;
  int64_t gb, ge, q0;
  int nq, ph;
};
template <typename P>
__device__ __forceinline__ TileSpan tile_span(const P& p, int tile, TableLevel& lv) {
  const auto& a = p.a;
  TileSpan s;
  s.level = 0;
  while (s.level + 1 < p.levels() && tile >= a.pl.tile_start[s.level + 1]) ++s.level;
  lv = p.level(s.level);
  const int sh = a.pl.tile_rows_log2;
  s.row0 = (uint32_t)(tile - a.pl.tile_start[s.level]) << sh;
  s.nrows = (lv.rows - s.row0) < (1u << sh) ? (lv.rows - s.row0) : (1u << sh);
  s.gb = ((int64_t)lv.off0 + s.row0) * p.row_floats();
  s.ge = s.gb + (int64_t)s.nrows * p.row_floats();
  s.q0 = s.gb >> 2;
  s.nq = (int)(((s.ge + 3) >> 2) - s.q0);
  s.ph = (int)(s.gb - (s.q0 << 2));
  return s;
}

// The tile's records, summed into the LDS image `acc` (float4 group q of the span at acc + 4 q).  In two halves, so that a kernel can request this thread's
// first record BEFORE it clears the image (two dependent round trips): tile_walk_begin, clear + lds_barrier, tile_walk.
template <typename P>
struct TileWalk {
  int i, end;
  typename P::Rec next;
};
template <typename P>
__device__ __forceinline__ TileWalk<P> tile_walk_begin(const P& p, int tile) {
  TileWalk<P> w;
  w.i = p.a.tile_base[tile] + (int)threadIdx.x;
  w.end = p.a.tile_base[tile + 1];
  w.next = typename P::Rec{};
  if (w.i < w.end) w.next = p.fetch(w.i);
  return w;
}
template <typename P>
__device__ __forceinline__ void tile_walk(const P& p, TileWalk<P>& w, const TileSpan& s, const TableLevel& lv, float* acc) {
  for (int i = w.i; i < w.end; i += TILE_NT) {
    const typename P::Rec r = w.next;
    if (i + TILE_NT < w.end) w.next = p.fetch(i + TILE_NT);  // the next record of this thread (tiles of the coarse levels hold thousands)
    const int yz = (int)(r.rec >> 2) & 3, xm = (int)(r.rec & 3u);
    uint32_t pg[3];
    float fr[3];
    const typename P::Sample smp = p.sample(r, lv, s.level, pg, fr);
    const uint32_t cy = pg[1] + (uint32_t)(yz & 1), cz = pg[2] + (uint32_t)(yz >> 1);
#pragma unroll
    for (int xb = 0; xb < 2; ++xb) {
      if (!((xm >> xb) & 1)) continue;
      const float wgt = table_corner_weight(fr, 3, xb | (yz << 1));  // the scatter kernels' own
      const uint32_t row = lv.row_of(pg[0] + (uint32_t)xb, cy, cz);
      p.add(smp, acc + s.ph + (int)(row - s.row0) * p.row_floats(), wgt);
    }
  }
}

__device__ __forceinline__ void tile_clear(float* acc, int nq) {
  for (int q = threadIdx.x; q < nq; q += TILE_NT) *reinterpret_cast<float4*>(acc + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// MODE 0: dense gradient += tile with plain loads / stores (the tile is the only writer of its rows), all-zero groups skipped; a group that straddles the
// tile's first / last float is handled element by element
__device__ __forceinline__ void tile_accumulate(const TileSpan& s, const float* acc, float* gtable) {
  for (int q = threadIdx.x; q < s.nq; q += TILE_NT) {
    const int64_t f0 = (s.q0 + q) << 2;
    const float4 gq = *reinterpret_cast<const float4*>(acc + 4 * q);
    if (gq.x == 0.f && gq.y == 0.f && gq.z == 0.f && gq.w == 0.f) continue;
    if (f0 >= s.gb && f0 + 4 <= s.ge) {
      float4 o = *reinterpret_cast<const float4*>(gtable + f0);
      o.x += gq.x; o.y += gq.y; o.z += gq.z; o.w += gq.w;
      *reinterpret_cast<float4*>(gtable + f0) = o;
    } else {
      const float* G = &gq.x;
      for (int k = 0; k < 4; ++k)
        if (f0 + k >= s.gb && f0 + k < s.ge && G[k] != 0.f) gtable[f0 + k] += G[k];
    }
  }
}

// one workgroup per tile; MODE 0 (accumulate) starts at the first tiled level: tiles of the coarse levels hold no records
template <typename P, void (*KERNEL)(P), int MODE>
static int tile_launch(P& p, int lds, hipStream_t st, const char* what) {
  SNERF_ALLOW_LDS(KERNEL, lds);
  p.a.tile0 = MODE == 0 ? p.a.pl.tile_start[p.a.pl.first_tiled_level] : 0;
  const int n = p.a.pl.n_tiles - p.a.tile0;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)n), dim3(TILE_NT), (size_t)lds, st, p);
  SNERF_LAUNCH_CHECK(what);
  return 0;
}

// channels per level (C or F) are a template argument of both grids' kernels: 1, 2, 4 or 8, checked by the caller
#define TILE_DISPATCH_1248(N_, CALL) \
  switch (N_) {                      \
    case 1: return CALL(1);          \
    case 2: return CALL(2);          \
    case 4: return CALL(4);          \
    default: return CALL(8);         \
  }

}  // namespace snerf
