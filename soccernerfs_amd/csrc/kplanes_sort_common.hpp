// The sort order of the sorted plane-gradient scatter (kplanes_sorted.hip: two-level binned sort + pass B): segment table, Morton keys, the
// plan of the two levels.  (Split out in round 3 for an owner-computes scatter + Adam kernel that looked cells up in the sort's scanned
// histogram; that kernel measured slower than pass B + sweep and was removed -- profiles/r03_tile_adam_experiment.md.)
#pragma once
#include "kplanes_common.hpp"

namespace snerf {

struct SegTable {
  int n_planes;
  int per_scale;    // pass B's switch "every (scale, plane) segment has its own order"; the sort builds one order per plane: always 0
  int fine[4];      // sort-grid resolution of each axis = its finest resolution over the scales
  int fine_rm[4];   // sort grid for the minor axis of row-major (time) planes: several samples share a (time row, texel)
                    // there, and only a (near-)true sort by x keeps every scale's texel index monotone inside a row
  int row_major[6]; // 1: key = i0_b * fine_rm[a] + i0_a(fine_rm) (time planes: the time row is exact at every scale); 0: Morton(i0_a, i0_b)
  int cells[6];     // keys of plane q lie in [0, cells[q])
};

// Morton interleave of two 16-bit integers (x -> even bits, y -> odd bits)
__device__ __forceinline__ uint32_t part1by1(uint32_t v) {
  v &= 0x0000ffffu;
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}
__device__ __forceinline__ uint32_t morton2(uint32_t x, uint32_t y) { return part1by1(x) | (part1by1(y) << 1); }

// (QUOT_TINY, the "vanished" threshold of the quotient form, lives in common.hpp: the sigma_net backward's epilogue uses it too)


inline int build_segs(const snerf_kplanes_desc* d, SegTable& st) {
  const int NP = d->n_coords == 4 ? 6 : 3;
  st.n_planes = NP;
  for (int k = 0; k < 4; ++k) {
    int fine = 1;
    for (int s = 0; s < d->n_scales; ++s) {
      const int r = d->res[s][k] > 0 ? d->res[s][k] : 1;
      fine = r > fine ? r : fine;
    }
    st.fine[k] = fine;  // measured: aligning the sort grid to the coarsest scale, or a finer grid for the time planes, does not pay
    SNERF_REQUIRE(st.fine[k] <= 32768, "kplanes_sort: resolution %d too large for the Morton key", st.fine[k]);
    st.fine_rm[k] = fine;
  }
  // one shared order per plane (a separate global sort per scale costs +0.5 ms of sorting for -0.3 ms of pass B: profiles/r01_kernels.md)
  st.per_scale = 0;
  for (int q = 0; q < 6; ++q) st.row_major[q] = 0, st.cells[q] = 1;
  for (int q = 0; q < NP; ++q) {
    const int a = NP == 6 ? pair_a<6>(q) : pair_a<3>(q), b = NP == 6 ? pair_b<6>(q) : pair_b<3>(q);
    // planes whose row axis is time: time is not multiscale, so (time row, fine x) row-major keeps every scale's runs whole
    st.row_major[q] = (NP == 6 && b == 3) ? 1 : 0;
    int64_t cells;
    if (st.row_major[q]) {
      cells = (int64_t)st.fine_rm[a] * st.fine[b];
    } else {
      const int m = st.fine[a] > st.fine[b] ? st.fine[a] : st.fine[b];
      int bits = 0;
      while ((1 << bits) < m) ++bits;
      cells = (int64_t)1 << (2 * bits);  // Morton codes of a (2^bits)^2 square
    }
    SNERF_REQUIRE(cells <= (1LL << 28), "kplanes_sort: too many sort cells in plane %d (%lld)", q, (long long)cells);
    st.cells[q] = (int)cells;
  }
  return 0;
}

// ---- the two levels of the sort ----
// Level 1 files every (sample, plane) under the coarse bin key >> shift[q] (an LDS histogram per workgroup of SORT_CHUNK samples, a
// [chunks][bins] count matrix, one small scan over the chunks: no global atomics, nothing to clear); level 2 orders one bin per workgroup by the low
// shift[q] bits with 2^shift[q] LDS counters.  The cost follows the entries: the bins are few (<= SORT_BINS per plane) however many cells.
constexpr int SORT_NT = 256;       // threads of every sort workgroup
constexpr int SORT_CHUNK = 2048;   // samples per level-1 workgroup
constexpr int SORT_BINS = 2048;    // coarse bins per plane: 8 KB of LDS counters in level 1
constexpr int SORT_SHIFT_MAX = 11;  // 8 KB of LDS counters in level 2: planes of up to 2^22 sort cells (finest resolution 2048), the largest that is tested

struct SortPlan {
  int shift[6];  // low key bits that level 2 orders
  int bin0[7];   // first coarse bin of each plane; [n_planes] = all bins
  int n_chunks;
  int lds1, lds2;  // dynamic LDS bytes of the level-1 / level-2 kernels
  // the opaque workspace `hist`, in int32 elements: intermediate records, count matrix, bin totals, bin bases
  int64_t tmp_off, counts_off, totals_off, base_off, total;
};

inline int sort_plan_make(const SegTable& st, int64_t N, SortPlan& sp) {
  SNERF_REQUIRE(N >= 0 && (int64_t)st.n_planes * N < (1LL << 31), "kplanes_sort: n_planes * N = %lld (< 2^31)", (long long)(st.n_planes * N));
  int bins = 0, max_bins = 1, max_shift = 0;
  for (int q = 0; q < 6; ++q) sp.shift[q] = 0;
  for (int q = 0; q < st.n_planes; ++q) {
    const int64_t last = (int64_t)st.cells[q] - 1;
    int sh = 0;
    while ((last >> sh) + 1 > SORT_BINS) ++sh;
    // larger planes would need more counters per workgroup than the side stream should take, and no test covers them: refused, not planned
    SNERF_REQUIRE(sh <= SORT_SHIFT_MAX, "kplanes_sort: plane %d has %d sort cells, more than %d (finest resolution above 2048)", q, st.cells[q],
                  SORT_BINS << SORT_SHIFT_MAX);
    const int nb = (int)(last >> sh) + 1;
    sp.shift[q] = sh;
    sp.bin0[q] = bins;
    bins += nb;
    max_bins = nb > max_bins ? nb : max_bins;
    max_shift = sh > max_shift ? sh : max_shift;
  }
  for (int q = st.n_planes; q < 7; ++q) sp.bin0[q] = bins;
  sp.n_chunks = (int)((N + SORT_CHUNK - 1) / SORT_CHUNK);
  sp.lds1 = max_bins * (int)sizeof(int32_t);
  sp.lds2 = (1 << max_shift) * (int)sizeof(int32_t);
  sp.tmp_off = 0;  // float4 records first: the workspace's own alignment is theirs
  sp.counts_off = 4 * (int64_t)st.n_planes * N;
  sp.totals_off = sp.counts_off + (int64_t)sp.n_chunks * bins;
  sp.base_off = sp.totals_off + bins;
  sp.total = sp.base_off + bins + 1;
  return 0;
}

}  // namespace snerf
