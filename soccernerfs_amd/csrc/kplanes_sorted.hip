// K-Planes plane-gradient scatter, sorted variant: ~6x fewer atomic requests than the sample-major scatter.
//
// Why: fp32 atomics on gfx950 cost ~one memory-side 64-B request each (MI355X_MICROARCH.md "Global float atomics"), and the
// sample-major scatter (kplanes.hip) can only merge contributions of CONSECUTIVE samples of one ray.  Counted on real
// training batches (tools/scatter_stats.py, 262 144 samples, 30 planes): 6.8 M (plane,row) flushes early in training, 3.7 M
// after 3 k steps -- but only 0.7-0.9 M DISTINCT (plane, row, x0) keys: the three time planes have just n_times x W
// texels, and coarse spatial planes a few thousand.  Sorting the samples of every (scale, plane) segment by texel key
// makes equal keys adjacent, so run-length combining removes ~85 % of the requests.
//
// ONE sort per plane serves every scale: the key is the Z-order (Morton) code of the sample's texel at the FINEST scale, so
// the samples of any coarser texel (a ~power-of-two block of fine texels) are (almost always) contiguous too.
//
// Pipeline (NP plane segments, each with exactly N entries):
//   S  sort    : key = morton(x0, row0 at the finest scale) (time planes: row0 * W + x0), ordered in two LDS-binned levels whose cost
//                follows the entries, not the cells (kplanes_sort_common.hpp: SortPlan) -- no global atomics, nothing to clear:
//     S1 count / scan / fill : one workgroup per (chunk of samples, plane) counts its samples per COARSE bin (key >> shift) in LDS and
//                writes its row of a [chunks][bins] matrix; a scan over the chunks gives every chunk its offset inside a bin and the bins'
//                totals; the fill pass scans its plane's totals in LDS, recomputes the keys, takes chunk-local slots from LDS and writes
//                {n, coord_a, coord_b, key} to the bin's range
//     S2 place   : one workgroup per coarse bin orders the bin by the low key bits with 2^shift LDS counters (count, scan, place) and
//                writes sorted_rec = {n, coord_a, coord_b, 0} (sample id + its two normalised coordinates on that plane).
//                Positions depend only on the sample coordinates, so the sort runs on a side stream under the forward / MLP
//                backward, and pass B never has to touch the ray buffers again
//   A  gradvec : sample-major, float4 per lane (like the forward gather): g_q = dL/d(interp of plane q) -> gvec[seg][n][C]
//   B  scatter : per segment, lane groups of 2*C lanes (x-corner, channel) walk RUN consecutive SORTED entries, multiply by
//                the bilinear weights, run-length-combine per row and flush with one 256-B atomic instruction per run.
#include <stdlib.h>

#include "kplanes_sort_common.hpp"

namespace snerf {

// ---- the sort: level 1 (coarse bins), two small scans, level 2 (inside a bin) ----
// what a workgroup needs to form plane q's keys: the axis pair, the two sort-grid resolutions, Morton or row-major
struct PlaneKey {
  int a, b, ra, rb, row_major;
};
template <int NP>
__device__ __forceinline__ PlaneKey plane_key_of(const SegTable& st, int q) {
  PlaneKey k;
  k.a = pair_a<NP>(q); k.b = pair_b<NP>(q);
  k.row_major = st.row_major[q];
  const int fa = k.row_major ? st.fine_rm[k.a] : st.fine[k.a], fb = st.fine[k.b];
  k.ra = fa > 0 ? fa : 1; k.rb = fb > 0 ? fb : 1;
  return k;
}
// the plane's two coordinates of a sample (selects, so that p[] stays in registers)
__device__ __forceinline__ void plane_coords(const PlaneKey& k, const float p[4], float& pa, float& pb) {
  pa = k.a == 0 ? p[0] : (k.a == 1 ? p[1] : p[2]);
  pb = k.b == 1 ? p[1] : (k.b == 2 ? p[2] : p[3]);
}
// the sample's cell on the sort grid (floor of axis_pix: kplanes_common.hpp)
__device__ __forceinline__ uint32_t plane_key(const PlaneKey& k, float pa, float pb) {
  const int ia = (int)floorf(axis_pix(pa, k.ra)), ib = (int)floorf(axis_pix(pb, k.rb));
  return k.row_major ? (uint32_t)(ib * k.ra + ia) : morton2((uint32_t)ia, (uint32_t)ib);
}

// This lane's slot under LDS counter idx: one returning LDS add per lane -- or, where every active lane of the wave names the same counter
// (a batch planted in one cell; the 64 samples of a ray on one time row), a single add for the wave instead of 64 serialised ones.
__device__ __forceinline__ int lds_take(int32_t* ctr, int idx) {
  const int first = __builtin_amdgcn_readfirstlane(idx);
  const unsigned long long act = __ballot(1);
  if (__ballot(idx == first) == act) {
    const int before = __popcll(act & ((1ull << (threadIdx.x & 63)) - 1ull));
    int base = 0;
    if (before == 0) base = atomicAdd(ctr + first, __popcll(act));
    return __builtin_amdgcn_readfirstlane(base) + before;  // the first active lane is the one that added
  }
  return atomicAdd(ctr + idx, 1);
}

// Exclusive prefix sums of the LDS words a[0, n), in place, starting at `start`: thread t owns words [t * per, (t + 1) * per).  Called by all SORT_NT
// threads, with a barrier in front (a[] complete) and one behind (before anyone reads another thread's words); wsum: SORT_NT / 64 words of LDS.
__device__ __forceinline__ void block_exclusive_scan(int32_t* a, int n, int start, int* wsum) {
  const int per = (n + SORT_NT - 1) / SORT_NT;
  const int c0 = (int)threadIdx.x * per, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int local = 0;
  for (int k = 0; k < per; ++k)
    if (c0 + k < n) local += a[c0 + k];
  int incl = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int run = start + incl - local;
  for (int k = 0; k < w; ++k) run += wsum[k];
  for (int k = 0; k < per; ++k)
    if (c0 + k < n) {
      const int v = a[c0 + k];
      a[c0 + k] = run;
      run += v;
    }
}

// Level 1, grid (chunks, planes).  FILL = false: count the chunk's samples per coarse bin, write the chunk's row of counts[chunks][bins] (every word,
// so nothing has to be cleared).  FILL = true: the LDS counters start at the chunk's first slot of each bin -- the bin's base, an exclusive scan of
// the plane's bin totals that every workgroup makes for itself in LDS (a plane's bins hold exactly N entries, so plane q starts at q * N: no scan
// across planes, no kernel of its own), plus the chunk's scanned count -- and every sample's intermediate record {n, p_a, p_b, key} goes to the slot
// it takes.  The workgroups of chunk 0 leave the bin bases in bin_base[] for level 2.
template <int NP, bool FILL>
__global__ __launch_bounds__(SORT_NT) void sort_bin_kernel(snerf_coords c, SegTable st, SortPlan sp, int64_t N, int32_t* __restrict__ counts,
                                                          const int32_t* __restrict__ totals, int32_t* __restrict__ bin_base, float4* __restrict__ tmp) {
  extern __shared__ int32_t s_sort[];
  __shared__ int s_wsum[SORT_NT / 64];
  const int q = (int)blockIdx.y, chunk = (int)blockIdx.x;
  const int B0 = sp.bin0[q], nb = sp.bin0[q + 1] - B0, sh = sp.shift[q];
  int32_t* mine = counts + (int64_t)chunk * sp.bin0[NP] + B0;
  if (FILL) {
    for (int i = threadIdx.x; i < nb; i += SORT_NT) s_sort[i] = totals[B0 + i];
    __syncthreads();
    block_exclusive_scan(s_sort, nb, (int)(q * N), s_wsum);
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += SORT_NT) {
      const int base = s_sort[i];
      s_sort[i] = base + mine[i];
      if (chunk == 0) bin_base[B0 + i] = base;
    }
    if (chunk == 0 && q == NP - 1 && threadIdx.x == 0) bin_base[sp.bin0[NP]] = (int)(NP * N);
  } else {
    for (int i = threadIdx.x; i < nb; i += SORT_NT) s_sort[i] = 0;
  }
  __syncthreads();
  const PlaneKey pk = plane_key_of<NP>(st, q);
  const int64_t n0 = (int64_t)chunk * SORT_CHUNK;
  const int64_t n1 = n0 + SORT_CHUNK < N ? n0 + SORT_CHUNK : N;
  for (int64_t n = n0 + threadIdx.x; n < n1; n += SORT_NT) {
    float p[4], pa, pb;
    load_coords<NP>(c, n, p);
    plane_coords(pk, p, pa, pb);
    const uint32_t key = plane_key(pk, pa, pb);
    const int slot = lds_take(s_sort, (int)(key >> sh));
    if (FILL) tmp[slot] = make_float4(__int_as_float((int)n), pa, pb, __int_as_float((int)key));
  }
  if (!FILL) {
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += SORT_NT) mine[i] = s_sort[i];
  }
}

// Per bin: counts[chunk][bin] -> the chunk's offset inside the bin (exclusive prefix over the chunks); totals[bin] = the bin's entries.  A workgroup
// takes 64 bins x 4 quarters of the chunks: a column's loads are independent of each other (a running sum with its store between the loads made
// this the longest kernel of the sort), the quarters meet in LDS, and the second walk over the column finds it in cache.
__global__ __launch_bounds__(256) void sort_scan_chunks_kernel(int32_t* __restrict__ counts, int n_chunks, int n_bins, int32_t* __restrict__ totals) {
  __shared__ int s_part[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int t = (int)blockIdx.x * 64 + lane;
  const bool live = t < n_bins;
  const int per = (n_chunks + 3) / 4;
  const int c0 = g * per < n_chunks ? g * per : n_chunks, c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
  int32_t* col = counts + (live ? t : 0);
  int sum = 0;
  if (live) {
#pragma unroll 8
    for (int ch = c0; ch < c1; ++ch) sum += col[(int64_t)ch * n_bins];
  }
  s_part[g][lane] = sum;
  __syncthreads();
  if (!live) return;
  int run = 0;
  for (int k = 0; k < g; ++k) run += s_part[k][lane];
  if (g == 3) totals[t] = run + sum;
  int ch = c0;
  for (; ch + 8 <= c1; ch += 8) {  // eight loads in flight, then their stores
    int v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = col[(int64_t)(ch + k) * n_bins];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      col[(int64_t)(ch + k) * n_bins] = run;
      run += v[k];
    }
  }
  for (; ch < c1; ++ch) {
    const int v = col[(int64_t)ch * n_bins];
    col[(int64_t)ch * n_bins] = run;
    run += v;
  }
}


// Level 2, one workgroup per coarse bin: a counting sort of the bin's intermediate records by the low `shift` key bits.  LDS holds the 2^shift
// counters only; the bin's range [bin_base[bin], bin_base[bin + 1]) is walked twice (count, place), however long it is.  Writes the final record
// {n, p_a, p_b, 0}.
__global__ __launch_bounds__(SORT_NT) void sort_place_kernel(SortPlan sp, const int32_t* __restrict__ bin_base, const float4* __restrict__ tmp,
                                                            float4* __restrict__ sorted_rec) {
  extern __shared__ int32_t s_sort[];
  __shared__ int s_wsum[SORT_NT / 64];
  const int bin = (int)blockIdx.x;
  const int beg = bin_base[bin], end = bin_base[bin + 1];
  if (beg == end) return;  // most bins of a real batch
  int q = 0;
  while (bin >= sp.bin0[q + 1]) ++q;
  const int sh = sp.shift[q], nc = 1 << sh;
  const uint32_t mask = (uint32_t)nc - 1u;
  if (sh == 0 || end - beg == 1) {  // one cell per bin, or one entry: level 1 has ordered it
    for (int i = beg + (int)threadIdx.x; i < end; i += SORT_NT) {
      const float4 r = tmp[i];
      sorted_rec[i] = make_float4(r.x, r.y, r.z, 0.f);
    }
    return;
  }
  for (int i = threadIdx.x; i < nc; i += SORT_NT) s_sort[i] = 0;
  __syncthreads();
#pragma unroll 4
  for (int i = beg + (int)threadIdx.x; i < end; i += SORT_NT) atomicAdd(&s_sort[(uint32_t)__float_as_int(tmp[i].w) & mask], 1);
  __syncthreads();
  block_exclusive_scan(s_sort, nc, beg, s_wsum);
  __syncthreads();
  for (int i = beg + (int)threadIdx.x; i < end; i += SORT_NT) {
    const float4 r = tmp[i];
    const int slot = lds_take(s_sort, (int)((uint32_t)__float_as_int(r.w) & mask));
    sorted_rec[slot] = make_float4(r.x, r.y, r.z, 0.f);
  }
}


// gvec rows are fp32 (exact: the parity path) or bf16 (half the 2 GB round trip between pass A and pass B; the scatter still accumulates
// in fp32, each contribution carries a 2^-9 relative rounding)
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_gq(float* gv, int64_t idx, float4 g) { *reinterpret_cast<float4*>(gv + idx) = g; }
__device__ __forceinline__ void store_gq(__bf16* gv, int64_t idx, float4 g) {
  const bf16x4 b = {(__bf16)g.x, (__bf16)g.y, (__bf16)g.z, (__bf16)g.w};
  *reinterpret_cast<bf16x4*>(gv + idx) = b;
}
__device__ __forceinline__ float load_g(const float* gv, int64_t idx) { return gv[idx]; }
__device__ __forceinline__ float load_g(const __bf16* gv, int64_t idx) { return (float)gv[idx]; }

// ---- pass A: gradient w.r.t. each plane's interpolated value, sample-major ----
template <int C, int NP, typename GV>
__global__ __launch_bounds__(256) void gradvec_kernel(snerf_kplanes_desc d, const float* __restrict__ planes, snerf_coords c, int64_t N,
                                                     const float* __restrict__ gout, GV* __restrict__ gvec) {
  constexpr int LPS = C / 4;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = gid / LPS;
  const int cg = (int)(gid % LPS);
  if (n >= N) return;
  float p[4];
  load_coords<NP>(c, n, p);
  const int out_w = d.concat ? C * d.n_scales : C;
  const float* grow = gout + n * out_w + cg * 4;
  constexpr auto& A = PlanePairs<NP>::a;
  constexpr auto& B = PlanePairs<NP>::b;
  for (int s = 0; s < d.n_scales; ++s) {
    AxisTap tap[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tap[k] = axis_tap(p[k], d.res[s][k] > 0 ? d.res[s][k] : 1);
    float4 v[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) v[q] = plane_sample<C>(planes + d.off[s][q], d.res[s][A[q]], tap[A[q]], tap[B[q]], cg);
    float4 gq[NP];
    leave_one_out<NP>(*reinterpret_cast<const float4*>(grow + (d.concat ? s * C : 0)), v, gq);
#pragma unroll
    for (int q = 0; q < NP; ++q) store_gq(gvec, ((int64_t)(s * NP + q) * N + n) * C + cg * 4, gq[q]);
  }
}

// ---- pass B: what a lane group works on ----
// Lane group `group` of a launch that starts at segment seg_begin takes `len` consecutive sorted entries, [i0, i0 + cnt), of segment seg = (scale s,
// plane q): a W x H plane whose sorted records of these entries start at rec (the plane's order is shared by all scales unless per_scale).
struct PassBSeg {
  int seg, s, q, W, H, cnt;
  int64_t i0;
  const float4* rec;
};
// false: the group lies beyond the last segment (d ends at the launch's last scale) or beyond the last entry and has nothing to do
template <int NP>
__device__ __forceinline__ bool passb_segment(const snerf_kplanes_desc& d, int64_t N, const float4* __restrict__ sorted_rec, int64_t group,
                                              int64_t groups_per_seg, int seg_begin, int per_scale, int len, PassBSeg& g) {
  g.seg = seg_begin + (int)(group / groups_per_seg);
  if (g.seg >= d.n_scales * NP) return false;
  g.i0 = (group - (int64_t)(g.seg - seg_begin) * groups_per_seg) * len;
  if (g.i0 >= N) return false;
  g.cnt = (int)((N - g.i0) < len ? (N - g.i0) : len);
  g.s = g.seg / NP;
  g.q = g.seg % NP;
  constexpr auto& A = PlanePairs<NP>::a;
  constexpr auto& B = PlanePairs<NP>::b;
  g.W = d.res[g.s][A[g.q]];
  g.H = d.res[g.s][B[g.q]] > 0 ? d.res[g.s][B[g.q]] : 1;
  g.rec = sorted_rec + (int64_t)(per_scale ? g.seg : g.q) * N + g.i0;
  return true;
}

// ---- pass B: sorted run-length scatter ----
// One lane group (2*C lanes = (x-corner, channel)) walks RUN consecutive SORTED records {n, fx, fy}.  Records are read
// UNROLL at a time (wave-uniform addresses), the UNROLL gvec rows are fetched together, then combined in order.
template <int C, int NP, typename GV>
__global__ __launch_bounds__(256) void scatter_sorted_kernel(snerf_kplanes_desc d, int64_t N, const GV* __restrict__ gvec,
                                                            const float4* __restrict__ sorted_rec, float* __restrict__ gplanes, int run,
                                                            int64_t groups_per_seg, int seg_begin, int per_scale) {
  constexpr int LPS = 2 * C;
  constexpr int UNROLL = 8;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // LPS == 64: one lane group = one wave, so the group index (and everything derived from it) is wave-uniform; readfirstlane
  // lets the compiler keep it in SGPRs and branch scalar
  const int64_t group = LPS == 64 ? (int64_t)blockIdx.x * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : gid / LPS;
  const int li = (int)(gid % LPS);
  const int half = li / C, ch = li % C;
  PassBSeg sg;
  if (!passb_segment<NP>(d, N, sorted_rec, group, groups_per_seg, seg_begin, per_scale, run, sg)) return;
  const int cnt = sg.cnt, W = sg.W, H = sg.H;
  const float4* rec = sg.rec;
  const GV* gv = gvec + (int64_t)sg.seg * N * C + ch;
  float* gbase = gplanes + d.off[sg.s][sg.q] + li;
  PendingRun pend[2];  // rows y0 and y0 + 1 of this lane's x-corner; key = the texel (row, x0)
  const auto flush = [&](int key, float val) { atomicAdd(gbase + (int64_t)key * C, val); };
  if (LPS == 64) {
    // The per-entry work (two bilinear taps, keys) is the same for all 64 lanes: do it LANE-PARALLEL for 64 entries at a time
    // (lane l handles entry base + l), then walk the 64 entries in order broadcasting the precomputed values with
    // v_readlane -- ~3x fewer vector instructions per entry than recomputing the taps in every lane.
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < cnt; base += 64) {
      const int e = base + lane;
      const float4 r = rec[e < cnt ? e : cnt - 1];
      const AxisTap tx = axis_tap(r.y, W);
      const AxisTap ty = axis_tap(r.z, H);
      const int nn = __float_as_int(r.x);
      const int k0 = ty.i0 * W + tx.i0, k1 = ty.i1 * W + tx.i0;
      const float wxa = tx.w0, wxb = tx.w1, wya = ty.w0, wyb = ty.w1;
      const int m = (cnt - base) < 64 ? (cnt - base) : 64;
      for (int u0 = 0; u0 < m; u0 += UNROLL) {
        float g[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const int uu = (u0 + u) < m ? (u0 + u) : (m - 1);
          g[u] = load_g(gv, (int64_t)__builtin_amdgcn_readlane(nn, uu) * C);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          const int uu = u0 + u;
          if (uu < m) {
            const float wx0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wxa), uu));
            const float wx1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wxb), uu));
            const float wx = half ? wx1 : wx0;
            const float gx = g[u] * wx;
            const int key[2] = {__builtin_amdgcn_readlane(k0, uu), __builtin_amdgcn_readlane(k1, uu)};
            const float wy[2] = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(wya), uu)),
                                 __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wyb), uu))};
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) pend[rr].add(key[rr], gx * wy[rr], flush);
          }
        }
      }
    }
  } else
  for (int i = 0; i < cnt; i += UNROLL) {
    float4 r[UNROLL];
    float g[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) r[u] = rec[i + u < cnt ? i + u : cnt - 1];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) g[u] = load_g(gv, (int64_t)__float_as_int(r[u].x) * C);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (i + u < cnt) {
        const AxisTap tx = axis_tap(r[u].y, W);
        const AxisTap ty = axis_tap(r[u].z, H);
        const float gx = g[u] * (half ? tx.w1 : tx.w0);
        pend[0].add(ty.i0 * W + tx.i0, gx * ty.w0, flush);
        pend[1].add(ty.i1 * W + tx.i0, gx * ty.w1, flush);
      }
    }
  }
  pend[0].drain(flush);
  pend[1].drain(flush);
}

// ---- pass B, C = 32: chunk-local regrouping by THIS scale's texel key, run-length combining, x-carry ----
// The shared Z-order of the finest scale keeps a chunk of 256 consecutive entries spatially compact at every scale, but the
// `res-1` scaling of align_corners=True does not nest coarse texel edges in fine ones, so a coarse cell's samples arrive in
// several runs (2.0 M flushes for 0.93 M distinct cells; a separate global sort per scale brings pass B from 0.81 to 0.53 ms but
// costs 0.5 ms more sorting).  Here every wave re-sorts ITS 256 entries by the segment's own key (row * W + x0) with an in-register
// bitonic network (36 rounds, ~550 instructions, no memory traffic) and walks them in that order: equal keys are adjacent, and
// inside a row x0 ascends, so for x-adjacent cells the shared texel (x0+1 of one cell = x0 of the next) is CARRIED in registers
// from half 1 to half 0 instead of being flushed twice.  What bounds this pass is the number of lane-level atomic operations
// (profiles/r01_kernels.md); regrouping + carry cut them by more than half.
template <int J>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
  if (J >= 32) return (uint32_t)__shfl_xor((int)v, J, 64);
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (J << 10) | 0x1f);  // bit mode: lane ^ J inside each group of 32
}

template <int K, int J>
__device__ __forceinline__ void bitonic_round(uint32_t (&w)[4], int lane) {
  if (J >= 64) {  // partner is another register of the same lane
    constexpr int JR = J / 64;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((r & JR) == 0) {
        const bool up = (((r * 64) & K) == 0);  // K >= 128 here: direction depends on the register index only
        const uint32_t a = w[r], b = w[r | JR];
        const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
        w[r] = up ? lo : hi;
        w[r | JR] = up ? hi : lo;
      }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t other = lane_xor<J>(w[r]);
      const int e = r * 64 + lane;
      const bool up = (e & K) == 0, lower = (lane & J) == 0;
      const uint32_t lo = w[r] < other ? w[r] : other, hi = w[r] < other ? other : w[r];
      w[r] = (lower == up) ? lo : hi;
    }
  }
}

template <int K, int J>
struct BitonicJ {
  static __device__ __forceinline__ void run(uint32_t (&w)[4], int lane) {
    bitonic_round<K, J>(w, lane);
    BitonicJ<K, J / 2>::run(w, lane);
  }
};
template <int K>
struct BitonicJ<K, 0> {
  static __device__ __forceinline__ void run(uint32_t (&)[4], int) {}
};
template <int K>
struct BitonicK {
  static __device__ __forceinline__ void run(uint32_t (&w)[4], int lane) {
    BitonicK<K / 2>::run(w, lane);
    BitonicJ<K, K / 2>::run(w, lane);
  }
};
template <>
struct BitonicK<1> {
  static __device__ __forceinline__ void run(uint32_t (&)[4], int) {}
};

// The chunk prelude of both kernels below.  The wave re-sorts ITS chunk (<= 256 entries of segment g, entry e = r * 64 + lane) by the segment's
// own texel key and leaves one 8-dword record per entry in R (this wave's LDS), in WALK order:
//   {hd.x, x0 | y0 << 16 (the cell: what the walk compares), hd.z, hd.w, w(x0y0), w(x0y1), w(x1y0), w(x1y1)}
// with hd.x, hd.z, hd.w from pack(hd, sample id, tx, ty): the kernel's own offsets (elements or bytes) and flags.  Positions >= cnt hold a null
// record: a key no cell has, zero offsets, zero weights.  Everything per-entry is prepared here lane-parallel (4 entries per lane) so that the walk --
// one or two entries per wave instruction -- costs ~10 VALU instructions per entry: the first version spent ~60 and was VALU-issue bound.
template <typename Pack>
__device__ __forceinline__ void passb_chunk_records(const PassBSeg& g, int lane, uint32_t* R, Pack&& pack) {
  const int W = g.W, H = g.H, cnt = g.cnt;
  const bool sortable = (int64_t)W * H <= (1 << 23);  // key << 8 | index must fit 31 bits
  // 1. sort words: (row * W + x0) << 8 | entry
  uint32_t word[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = r * 64 + lane;
    word[r] = 0xffffffffu;
    if (e < cnt) {
      const float4 rc = g.rec[e];
      const int x0 = (int)floorf(axis_pix(rc.y, W)), y0 = (int)floorf(axis_pix(rc.z, H));
      word[r] = sortable ? (((uint32_t)(y0 * W + x0) << 8) | (uint32_t)e) : (uint32_t)e;
    }
  }
  // 2. in-wave bitonic sort (ascending; 0xffffffff pads go last).  Not sortable (> 2^23 texels): the words are already ascending.
  if (sortable) BitonicK<256>::run(word, lane);
  // 3. the records, written at their position in the sorted order
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = r * 64 + lane;
    uint4 hd = make_uint4(0u, 0xffffffffu, 0u, 0u);
    float4 wt = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < cnt) {
      const float4 rc = g.rec[word[r] & 255u];
      const AxisTap tx = axis_tap(rc.y, W);
      const AxisTap ty = axis_tap(rc.z, H);
      hd.y = (uint32_t)tx.i0 | ((uint32_t)ty.i0 << 16);
      pack(hd, (uint32_t)__float_as_int(rc.x), tx, ty);
      const float4 tw = tap_weights(tx, ty);     // (x0y0, x1y0, x0y1, x1y1): the forward's products, bit for bit
      wt = make_float4(tw.x, tw.z, tw.y, tw.w);  // stored (x0y0, x0y1 | x1y0, x1y1): one float2 per x-corner; a clamped second tap has weight 0
    }
    *reinterpret_cast<uint4*>(R + e * 8) = hd;
    *reinterpret_cast<float4*>(R + e * 8 + 4) = wt;
  }
  // the records were stored one lane per entry and are read back by every lane of the wave: order the LDS stores before the loads
  // explicitly (same wave, so no s_barrier -- but neither the compiler nor the LDS queue may move a load above these stores)
  wave_lds_publish();
}

// QUOT (the quotient form, snerf_kplanes_scatter_quotient): gvec is ONE tensor G[N][row_stride] = gfeat .* feat (feat = the forward's product
// over the six planes), and the gradient vector of plane q at an entry is G / v_q with v_q re-interpolated here from the entry's cell --
// the 4 texels this lane group is about to add into, so the reads follow the sorted order and stay in cache.  lane = (x-corner, channel):
// each half interpolates its x-column, v_permlane32_swap adds the two halves.  v_q == 0 (then G == 0 as well: the information is gone)
// yields 0 here and the exact term is added by quotient_fixup_kernel.
template <int NP, typename GV, bool QUOT = false>
__global__ __launch_bounds__(256) void scatter_grouped_kernel(snerf_kplanes_desc d, int64_t N, const GV* __restrict__ gvec,
                                                             const float4* __restrict__ sorted_rec, float* __restrict__ gplanes,
                                                             int64_t groups_per_seg, int seg_begin, int per_scale,
                                                             const float* __restrict__ planes = nullptr, int row_stride = 0) {
  constexpr int C = 32, CH = 256, UNROLL = 16;
  // per wave, per entry (in WALK order) 8 dwords: {gvec row offset (elements), x0 | y0 << 16, QUOT: texel (x0, y0) offset in the plane (elements),
  // QUOT: x1-exists | y1-exists << 1, wx0*wy0, wx0*wy1, wx1*wy0, wx1*wy1}
  __shared__ __align__(16) uint32_t s_rec[4][CH * 8];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int half = lane >> 5, ch = lane & 31;
  PassBSeg sg;
  if (!passb_segment<NP>(d, N, sorted_rec, (int64_t)blockIdx.x * 4 + wave, groups_per_seg, seg_begin, per_scale, CH, sg)) return;
  const int cnt = sg.cnt, W = sg.W, s = sg.s, q = sg.q;
  // wave-uniform base; rows are addressed with 32-bit element offsets (the launcher guarantees N * C < 2^31)
  const GV* gseg = QUOT ? gvec + (int64_t)s * C : gvec + (int64_t)sg.seg * N * C;
  const uint32_t rstride = QUOT ? (uint32_t)row_stride : (uint32_t)C;
  float* gch = gplanes + d.off[s][q] + ch;
  const float* pch = QUOT ? planes + d.off[s][q] + ch : nullptr;
  uint32_t* R = s_rec[wave];
  passb_chunk_records(sg, lane, R, [&](uint4& hd, uint32_t n, const AxisTap& tx, const AxisTap& ty) {
    hd.x = n * rstride;
    if (QUOT) {
      hd.z = (uint32_t)(ty.i0 * W + tx.i0) * (uint32_t)C;
      hd.w = (tx.i1 != tx.i0 ? 1u : 0u) | (ty.i1 != ty.i0 ? 2u : 0u);
    }
  });
  // the walk.  One pending cell (x0 | y0 << 16 = ppk) with two accumulators per lane: rows y0 and y0 + 1; lane = (x-corner, channel).
  //    A row or column beyond the border only ever accumulates zeros and is never flushed (guards on != 0).
  uint32_t ppk = 0xfffffff0u;  // matches no record, nor record - 1
  float p0 = 0.f, p1 = 0.f;
  const uint32_t* Rl = R + 4 + half * 2;  // this lane's weight pair of an entry
  const int64_t rowC = (int64_t)W * C;
  const uint32_t rowC32 = (uint32_t)W * (uint32_t)C;
  for (int e0 = 0; e0 < cnt; e0 += UNROLL) {
    // UNROLL gvec rows in flight per wave (the pass streams 1 GB of them: with 8 in flight it was latency-bound, 0.61 vs 0.56 ms at 16);
    // the small per-entry fields are re-read from LDS when the entry is processed, so only g[] stays in registers
    float g[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) g[u] = load_g(gseg, (int64_t)(R[(e0 + u) * 8] + ch));  // wave-uniform LDS address: broadcast
    float t0[QUOT ? UNROLL : 1], t1[QUOT ? UNROLL : 1];  // QUOT: this lane's x-column of the entry's cell, rows y0 and y0 + 1
    if constexpr (QUOT) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        // element offset of texel (x0, y0) and the "x0 + 1 / y0 + 1 exist" flags were prepared lane-parallel with the record (a clamped
        // corner has weight 0 and re-reads the unclamped texel, as the forward's taps do; a null record reads texel 0 with zero weights)
        const uint32_t toff = (uint32_t)__builtin_amdgcn_readfirstlane((int)R[(e0 + u) * 8 + 2]);
        const uint32_t fl = (uint32_t)__builtin_amdgcn_readfirstlane((int)R[(e0 + u) * 8 + 3]);
        const uint32_t o0 = toff + (half ? (fl & 1u) * (uint32_t)C : 0u);
        t0[u] = pch[o0];
        t1[u] = pch[o0 + ((fl & 2u) ? rowC32 : 0u)];
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint32_t packed = (uint32_t)__builtin_amdgcn_readfirstlane((int)R[(e0 + u) * 8 + 1]);
      const float2 wt = *reinterpret_cast<const float2*>(Rl + (e0 + u) * 8);
      float gq = g[u];
      if constexpr (QUOT) {
        // the plane's value at the entry, with the forward's own formula and order (bilerp4): both x-columns in every lane
        const float4 w4 = *reinterpret_cast<const float4*>(R + (e0 + u) * 8 + 4);  // wave-uniform address: broadcast
        const auto s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t0[u]), __float_as_uint(t0[u]), false, false);  // row y0: [0] = x0 column, [1] = x1
        const auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t1[u]), __float_as_uint(t1[u]), false, false);  // row y0 + 1
        const float vq = bilerp4(__uint_as_float(s0[0]), __uint_as_float(s0[1]), __uint_as_float(s1[0]), __uint_as_float(s1[1]), w4.x, w4.z, w4.y, w4.w);
        gq = fabsf(vq) >= QUOT_TINY ? gq * __builtin_amdgcn_rcpf(vq) : 0.f;  // zero or subnormal (v_rcp_f32 may flush it): left to the fix-up
      }
      const float v0 = gq * wt.x, v1 = gq * wt.y;
      if (packed == ppk) {
        p0 += v0; p1 += v1;
      } else if (packed == ppk + 1u) {
        // x-adjacent cell of the same row pair: texel column pX is complete (flush it, 32 lanes), column pX + 1 carries over from
        // half 1 to half 0
        float* dst = gch + ((int64_t)(ppk >> 16) * W + (ppk & 0xffffu)) * C;
        if (half == 0 && p0 != 0.f) atomicAdd(dst, p0);
        if (half == 0 && p1 != 0.f) atomicAdd(dst + rowC, p1);
        const float m0 = __shfl_xor(p0, 32, 64), m1 = __shfl_xor(p1, 32, 64);
        p0 = (half == 0 ? m0 : 0.f) + v0;
        p1 = (half == 0 ? m1 : 0.f) + v1;
        ppk = packed;
      } else {
        float* dst = gch + ((int64_t)(ppk >> 16) * W + (ppk & 0xffffu) + half) * C;
        if (p0 != 0.f) atomicAdd(dst, p0);
        if (p1 != 0.f) atomicAdd(dst + rowC, p1);
        ppk = packed; p0 = v0; p1 = v1;
      }
    }
  }
  {
    float* dst = gch + ((int64_t)(ppk >> 16) * W + (ppk & 0xffffu) + half) * C;
    if (p0 != 0.f) atomicAdd(dst, p0);
    if (p1 != 0.f) atomicAdd(dst + rowC, p1);
  }
}

// ---- pass B, round 4: lane = channel, each HALF of the wave walks its own 128 of the wave's 256 re-sorted entries ----
// scatter_grouped_kernel above spends a wave instruction per entry on 64 lanes = (x-corner, channel): both halves interpolate the same v_q, the
// per-entry scalars go through v_readfirstlane, the x-carry through ds_bpermute, and every run end costs ~100 issued instructions (64-bit
// texel addresses, four exec-masked atomics) -- ~125 per entry, issue-bound at 0.35 of the HBM roofline (profiles/r03_kernels.md section 1).
// Here a lane owns ONE channel of ALL FOUR texels of the cell: it loads the four texels itself (no lane swaps; v_q is computed once per
// channel), keeps four accumulators, and an x-adjacent next cell moves the x0 + 1 column's accumulators to the x0 column IN THE LANE.  Two
// entries advance per wave instruction (lanes 0-31: entries [0, 128) of the walk order, lanes 32-63: [128, 256)), so everything per-entry is
// either lane-parallel (records, prepared as before) or costs half an instruction; the run-end logic is branch-free selects plus atomics
// under the lanes' own predicates, addressed with 32-bit byte offsets from wave-uniform bases (saddr form).  Same arithmetic per
// contribution as before except that the weighted add is one fma (gq * w + acc).
template <int NP, bool QUOT, int UNROLL = 8>
__global__ __launch_bounds__(256) void scatter_halfwave_kernel(snerf_kplanes_desc d, int64_t N, const float* __restrict__ gvec,
                                                              const float4* __restrict__ sorted_rec, float* __restrict__ gplanes,
                                                              int64_t groups_per_seg, int seg_begin, int per_scale,
                                                              const float* __restrict__ planes, int row_stride) {
  constexpr int C = 32, CH = 256, HALF = CH / 2;
  static_assert(HALF % UNROLL == 0, "a half's records must not run into the other half's");
  // per wave, per entry (in WALK order) 8 dwords: {gvec row BYTE offset, x0 | y0 << 16, texel (x0, y0) BYTE offset in the plane,
  // x1-exists ? 128 : 0 | y1-exists << 31, w(x0y0), w(x0y1), w(x1y0), w(x1y1)}
  __shared__ __align__(16) uint32_t s_rec[4][CH * 8];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int half = lane >> 5, ch = lane & 31;
  PassBSeg sg;
  if (!passb_segment<NP>(d, N, sorted_rec, (int64_t)blockIdx.x * 4 + wave, groups_per_seg, seg_begin, per_scale, CH, sg)) return;
  const int cnt = sg.cnt, W = sg.W, s = sg.s, q = sg.q;
  const char* gseg = reinterpret_cast<const char*>(QUOT ? gvec + (int64_t)s * C : gvec + (int64_t)sg.seg * N * C);
  const uint32_t rstrideB = (QUOT ? (uint32_t)row_stride : (uint32_t)C) * 4u;
  char* gbase = reinterpret_cast<char*>(gplanes + d.off[s][q]);
  const char* pbase = QUOT ? reinterpret_cast<const char*>(planes + d.off[s][q]) : nullptr;
  uint32_t* R = s_rec[wave];
  const uint32_t rowB = (uint32_t)W * (uint32_t)(C * 4);
  passb_chunk_records(sg, lane, R, [&](uint4& hd, uint32_t n, const AxisTap& tx, const AxisTap& ty) {
    hd.x = n * rstrideB;
    hd.z = (uint32_t)(ty.i0 * W + tx.i0) * (uint32_t)(C * 4);
    hd.w = (tx.i1 != tx.i0 ? (uint32_t)(C * 4) : 0u) | (ty.i1 != ty.i0 ? 0x80000000u : 0u);
  });
  // the walk: this half's entries are R[half * HALF + i]; pending cell = (pk, pa: byte offset of its (x0, y0) texel + this lane's channel,
  // pdx / pdy: byte steps to its x0 + 1 column / y0 + 1 row, 0 where clamped) with accumulators p00 (x0,y0), p01 (x0,y1), p10 (x1,y0), p11 (x1,y1).
  // The pending cell starts as the half's FIRST entry with empty accumulators, so no flush ever sees an invalid cell.  Zero sums (a clamped
  // column / row, a null record of the chunk's tail) are not sent: measured 0.445 -> 0.431 ms, 13 % fewer atomic requests.
  const uint32_t* Rh = R + half * (HALF * 8);
  const uint32_t chB = (uint32_t)ch * 4u;
  uint32_t pk, pa, pdx, pdy;
  {
    const uint4 hd = *reinterpret_cast<const uint4*>(Rh);
    pk = hd.y; pa = hd.z + chB; pdx = hd.w & 0xffu; pdy = (hd.w >> 31) ? rowB : 0u;
  }
  float p00 = 0.f, p01 = 0.f, p10 = 0.f, p11 = 0.f;
  auto add = [&](uint32_t off, float v) {
    if (v != 0.f) atomicAdd(reinterpret_cast<float*>(gbase + off), v);
  };
  const int iters = cnt > HALF ? HALF : cnt;  // half 1 walks null records where the chunk is short
  for (int e0 = 0; e0 < iters; e0 += UNROLL) {
    float g[UNROLL];
    float t00[QUOT ? UNROLL : 1], t10[QUOT ? UNROLL : 1], t01[QUOT ? UNROLL : 1], t11[QUOT ? UNROLL : 1];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint4 hd = *reinterpret_cast<const uint4*>(Rh + (e0 + u) * 8);
      g[u] = *reinterpret_cast<const float*>(gseg + (hd.x + chB));
      if constexpr (QUOT) {
        const uint32_t o00 = hd.z + chB, dx = hd.w & 0xffu, dy = (hd.w >> 31) ? rowB : 0u;
        t00[u] = *reinterpret_cast<const float*>(pbase + o00);
        t10[u] = *reinterpret_cast<const float*>(pbase + (o00 + dx));
        t01[u] = *reinterpret_cast<const float*>(pbase + (o00 + dy));
        t11[u] = *reinterpret_cast<const float*>(pbase + (o00 + dx + dy));
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint4 hd = *reinterpret_cast<const uint4*>(Rh + (e0 + u) * 8);
      const float4 w = *reinterpret_cast<const float4*>(Rh + (e0 + u) * 8 + 4);
      float gq = g[u];
      if constexpr (QUOT) {
        const float vq = bilerp4(t00[u], t10[u], t01[u], t11[u], w.x, w.z, w.y, w.w);  // the forward's own number
        const bool normal = fabsf(vq) >= QUOT_TINY;
        gq = normal ? gq * __builtin_amdgcn_rcpf(vq) : 0.f;  // v_q == 0: G is 0 too, the fix-up supplies the exact term
        // a SUBNORMAL v_q beside a usable G (the other planes' product is large): v_rcp_f32 may flush it, the IEEE division does not
        // (G != 0 implies v_q != 0 for a G formed from this forward's features; the inner test only guards callers' inconsistent inputs)
        if (__builtin_expect(!normal && g[u] != 0.f, 0)) gq = vq != 0.f ? __fdiv_rn(g[u], vq) : 0.f;
      }
      const uint32_t key = hd.y;
      const bool same = key == pk, adj = key == pk + 1u;
      if (!same) {
        add(pa, p00);
        add(pa + pdy, p01);
        if (!adj) {
          add(pa + pdx, p10);
          add(pa + pdx + pdy, p11);
        }
      }
      const float n00 = same ? p00 : (adj ? p10 : 0.f), n01 = same ? p01 : (adj ? p11 : 0.f);
      const float n10 = same ? p10 : 0.f, n11 = same ? p11 : 0.f;
      p00 = __fmaf_rn(gq, w.x, n00);
      p01 = __fmaf_rn(gq, w.y, n01);
      p10 = __fmaf_rn(gq, w.z, n10);
      p11 = __fmaf_rn(gq, w.w, n11);
      pk = key;
      pa = hd.z + chB;
      pdx = hd.w & 0xffu;
      pdy = (hd.w >> 31) ? rowB : 0u;
    }
  }
  add(pa, p00);
  add(pa + pdy, p01);
  add(pa + pdx, p10);
  add(pa + pdx + pdy, p11);
}

// ---- quotient form, the two small kernels around pass B ----
// The fix list holds ELEMENTS (round 4; rows before): {index into the [N, C n_scales] feature tensor, the feature gradient there} for every
// element whose feature vanished (zero, or below the smallest normal float) while its gradient did not: G / v_q cannot give plane q's gradient
// there (v_q == 0 took the other planes' product with it, or the product of six normal values underflowed).  Producers: quotient_prepare_kernel
// below, or the sigma_net backward's epilogue (mlp_lp.hip: snerf_mlp_bwd_x16_quotient), which forms G from the feature tile it holds in LDS.
// G = gfeat .* feat (C / 4 lanes per (sample, scale) row, float4 each); vanished features get G = 0 (pass B then adds exactly nothing for the
// channel) and, where the gradient is not zero, an entry in the fix list.
template <int C>
__global__ __launch_bounds__(256) void quotient_prepare_kernel(int64_t rows, const float* __restrict__ gfeat, const float* __restrict__ feat,
                                                              float* __restrict__ G, int32_t* __restrict__ list, int capacity, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ count_next) {
  // two counters, used alternately: this launch resets the OTHER one (its last reader, the previous step's fix-up, is behind us in stream
  // order), so no memset launch sits between the MLP backward and this kernel
  if (blockIdx.x == 0 && threadIdx.x == 0 && count_next) *count_next = 0;
  constexpr int LPR = C / 4;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = gid / LPR;
  if (row >= rows) return;
  const float4 g = *reinterpret_cast<const float4*>(gfeat + gid * 4);
  const float4 f = *reinterpret_cast<const float4*>(feat + gid * 4);
  const bool zx = fabsf(f.x) < QUOT_TINY, zy = fabsf(f.y) < QUOT_TINY, zz = fabsf(f.z) < QUOT_TINY, zw = fabsf(f.w) < QUOT_TINY;
  float4 Gv = f4_mul(g, f);
  Gv.x = zx ? 0.f : Gv.x; Gv.y = zy ? 0.f : Gv.y; Gv.z = zz ? 0.f : Gv.z; Gv.w = zw ? 0.f : Gv.w;
  *reinterpret_cast<float4*>(G + gid * 4) = Gv;
  if (zx && g.x != 0.f) fix_append(list, capacity, count, (int32_t)(gid * 4), g.x);
  if (zy && g.y != 0.f) fix_append(list, capacity, count, (int32_t)(gid * 4 + 1), g.y);
  if (zz && g.z != 0.f) fix_append(list, capacity, count, (int32_t)(gid * 4 + 2), g.z);
  if (zw && g.w != 0.f) fix_append(list, capacity, count, (int32_t)(gid * 4 + 3), g.w);
}

// Exact gradient of the listed elements, one lane per element (sample n, scale s, channel ch; g = the feature gradient).  With v_p the six
// planes' values at the sample (the forward's own numbers: bilerp4):
//   exactly ONE |v_z| below QUOT_TINY -> plane z receives g * prod_{p != z} v_p (the others' terms contain v_z: zero);
//   none (the product of six normal values underflowed)  -> EVERY plane q receives g * prod_{p != q} v_p;
//   two or more -> every term contains a vanished factor: nothing to add.
// Rare by construction (a trained texel that is exactly 0.0f, or an underflowing product), so no run-length combining.
template <int NP>
__global__ __launch_bounds__(256) void quotient_fixup_kernel(snerf_kplanes_desc d, const float* __restrict__ planes, snerf_coords c,
                                                            const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                            int capacity, float* __restrict__ gplanes, int n_scales_total, int scale_begin, int scale_end,
                                                            int32_t* __restrict__ overflow_peak) {
  constexpr int C = 32;
  int n_list = *count;
  // more entries were appended than the list holds: the ones beyond the capacity are lost.  Record it where the host can see it (sticky
  // maximum of the demanded entry count) instead of dropping gradients silently.
  if (overflow_peak && n_list > capacity && blockIdx.x == 0 && threadIdx.x == 0) atomicMax(overflow_peak, n_list);
  n_list = n_list < capacity ? n_list : capacity;
  const int F = n_scales_total * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_list; i += gridDim.x * blockDim.x) {
    const int elem = list[2 * i];
    const float g = __int_as_float(list[2 * i + 1]);
    const int64_t n = elem / F;
    const int col = elem - (int)n * F;
    const int s = col / C, ch = col - s * C;
    if (s < scale_begin || s >= scale_end) continue;
    float p[4];
    load_coords<NP>(c, n, p);
    AxisTap tap[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tap[k] = axis_tap(p[k], d.res[s][k] > 0 ? d.res[s][k] : 1);
    float v[NP];
    int zeros = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const AxisTap& tx = tap[pair_a<NP>(q)];
      const AxisTap& ty = tap[pair_b<NP>(q)];
      const int W = d.res[s][pair_a<NP>(q)];
      const float* base = planes + d.off[s][q] + ch;
      const float4 w = tap_weights(tx, ty);
      v[q] = bilerp4(base[((int64_t)ty.i0 * W + tx.i0) * C], base[((int64_t)ty.i0 * W + tx.i1) * C], base[((int64_t)ty.i1 * W + tx.i0) * C],
                     base[((int64_t)ty.i1 * W + tx.i1) * C], w.x, w.y, w.z, w.w);
      zeros += fabsf(v[q]) < QUOT_TINY;
    }
    if (zeros >= 2) continue;
    float term[NP];  // g * prod_{p != q} v_p
    leave_one_out<NP>(g, v, term);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      if (zeros == 1 && fabsf(v[q]) >= QUOT_TINY) continue;  // one vanished plane: only IT has a non-zero gradient
      const AxisTap& tx = tap[pair_a<NP>(q)];
      const AxisTap& ty = tap[pair_b<NP>(q)];
      const int W = d.res[s][pair_a<NP>(q)];
      float* gb = gplanes + d.off[s][q] + ch;
      const float a00 = term[q] * tx.w0 * ty.w0, a01 = term[q] * tx.w0 * ty.w1, a10 = term[q] * tx.w1 * ty.w0, a11 = term[q] * tx.w1 * ty.w1;
      if (a00 != 0.f) atomicAdd(gb + ((int64_t)ty.i0 * W + tx.i0) * C, a00);
      if (a01 != 0.f) atomicAdd(gb + ((int64_t)ty.i1 * W + tx.i0) * C, a01);
      if (a10 != 0.f) atomicAdd(gb + ((int64_t)ty.i0 * W + tx.i1) * C, a10);
      if (a11 != 0.f) atomicAdd(gb + ((int64_t)ty.i1 * W + tx.i1) * C, a11);
    }
  }
}

// Measured and dropped (profiles/r01_kernels.md): a per-wave LDS texel cache behind the register stage (64 direct-mapped texel
// rows, tags in lanes) halves the atomic requests (8.4 M -> 4.5 M) but is no faster: with ds_add_f32 each LDS instruction costs
// ~146 cycles (6x slower end to end), with read-add-write the LDS round trip per flush sits on the wave's critical path
// (0.88-0.93 ms vs 0.80-0.86 ms); deferring the add/write to the next flush so that the read has time to land: 1.09 ms.
// Ablation of this kernel: 0.28 ms without gvec loads and atomics, 0.36 ms without atomics, 0.81-0.86 ms complete -- the in-loop
// atomics are what it waits for, and the time follows neither the request count nor the prefetch depth nor the VALU count.

static int check_desc(const snerf_kplanes_desc* d, const snerf_coords* c, int64_t N) {
  SNERF_REQUIRE(d && c, "kplanes_sorted: null descriptor");
  SNERF_REQUIRE(d->n_scales >= 1 && d->n_scales <= SNERF_MAX_SCALES, "kplanes_sorted: n_scales=%d", d->n_scales);
  SNERF_REQUIRE(d->C == 8 || d->C == 16 || d->C == 32, "kplanes_sorted: C=%d unsupported", d->C);
  SNERF_REQUIRE(d->n_coords == 3 || d->n_coords == 4, "kplanes_sorted: n_coords=%d", d->n_coords);
  SNERF_REQUIRE(N >= 0 && N < (1LL << 31), "kplanes_sorted: N=%lld", (long long)N);
  SNERF_REQUIRE(c->mode == 0 || c->mode == 1, "kplanes_sorted: coords.mode=%d", c->mode);
  SNERF_REQUIRE_CONTRACT(c, "kplanes_sorted");
  if (c->mode == 1 && N > 0)
    SNERF_REQUIRE(ray_coords_complete(c, d->n_coords), "kplanes_sorted: null ray buffers (times may be null only with three coordinates)");
  return 0;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_kplanes_sort_workspace(const snerf_kplanes_desc* desc, int64_t N, int64_t* hist_cells, int64_t* index_elems) {
  SNERF_REQUIRE(desc && hist_cells && index_elems, "kplanes_sort_workspace: null argument");
  SegTable st;
  int rc = build_segs(desc, st);
  if (rc) return rc;
  SortPlan sp;
  rc = sort_plan_make(st, N, sp);
  if (rc) return rc;
  *hist_cells = sp.total;  // intermediate records + count matrix + bin bases
  *index_elems = (int64_t)st.n_planes * N;
  return 0;
}

template <int NP>
static int launch_sort(const snerf_coords& c, const SegTable& st, const SortPlan& sp, int64_t N, int32_t* ws, float4* sorted_n, hipStream_t s) {
  float4* tmp = reinterpret_cast<float4*>(ws + sp.tmp_off);
  int32_t* counts = ws + sp.counts_off;
  int32_t* totals = ws + sp.totals_off;
  int32_t* bin_base = ws + sp.base_off;
  const int n_bins = sp.bin0[NP];
  const dim3 grid((unsigned)sp.n_chunks, (unsigned)NP);
  hipLaunchKernelGGL((sort_bin_kernel<NP, false>), grid, dim3(SORT_NT), (size_t)sp.lds1, s, c, st, sp, N, counts, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(sort_scan_chunks_kernel, dim3((unsigned)ceil_div(n_bins, 64)), dim3(256), 0, s, counts, sp.n_chunks, n_bins, totals);
  hipLaunchKernelGGL((sort_bin_kernel<NP, true>), grid, dim3(SORT_NT), (size_t)sp.lds1, s, c, st, sp, N, counts, totals, bin_base, tmp);
  hipLaunchKernelGGL(sort_place_kernel, dim3((unsigned)n_bins), dim3(SORT_NT), (size_t)sp.lds2, s, sp, bin_base, tmp, sorted_n);
  SNERF_LAUNCH_CHECK("kplanes_sort_samples");
  return 0;
}

extern "C" int snerf_kplanes_sort_samples(const snerf_kplanes_desc* desc, const snerf_coords* coords, int64_t N, int32_t* hist, int32_t* rank,
                                          float* sorted_rec, snerf_stream_t stream) {
  int rc = check_desc(desc, coords, N);
  if (rc) return rc;
  if (N == 0) return 0;
  SNERF_REQUIRE(hist && rank && sorted_rec, "kplanes_sort_samples: null workspace");
  float4* sorted_n = reinterpret_cast<float4*>(sorted_rec);
  SegTable st;
  rc = build_segs(desc, st);
  if (rc) return rc;
  SortPlan sp;
  rc = sort_plan_make(st, N, sp);
  if (rc) return rc;
  SNERF_REQUIRE((reinterpret_cast<uintptr_t>(hist) & 15) == 0, "kplanes_sort_samples: the workspace must be 16-byte aligned");
  (void)rank;  // the second workspace: sized by the contract (index_elems), not needed by this sort
  if (desc->n_coords == 4) return launch_sort<6>(*coords, st, sp, N, hist, sorted_n, (hipStream_t)stream);
  return launch_sort<3>(*coords, st, sp, N, hist, sorted_n, (hipStream_t)stream);
}

template <int C, int NP>
static int launch_gradvec(const snerf_kplanes_desc* d, const float* planes, const snerf_coords* c, int64_t N, const float* gout, void* gvec, int gvec_bf16,
                          hipStream_t st) {
  const dim3 grid((unsigned)ceil_div(N * (C / 4), 256));
  if (gvec_bf16) hipLaunchKernelGGL((gradvec_kernel<C, NP, __bf16>), grid, dim3(256), 0, st, *d, planes, *c, N, gout, (__bf16*)gvec);
  else hipLaunchKernelGGL((gradvec_kernel<C, NP, float>), grid, dim3(256), 0, st, *d, planes, *c, N, gout, (float*)gvec);
  SNERF_LAUNCH_CHECK("kplanes_gradvec");
  return 0;
}
// What a pass-B launch over scales [scale_begin, scale_end) needs, for both forms.  row_stride: floats between two samples' gradient rows (C for
// the product form's per-segment vectors, C * n_scales for the quotient form's G).
struct PassBLaunch {
  snerf_kplanes_desc dd;  // the descriptor cut off at scale_end: the kernels stop at segment dd.n_scales * NP
  SegTable st;
  int64_t gps;      // lane groups per segment: one per 256 sorted entries
  dim3 grid;        // of the two chunk kernels: 4 waves = 4 lane groups per workgroup
  int64_t max_res;  // the largest resolution of the scales in the range
  bool halfwave;    // scatter_halfwave_kernel may run: its 32-bit BYTE offsets reach every gradient row and every texel, x0 | y0 << 16 holds the cell
};
static int passb_launch_make(const snerf_kplanes_desc* d, int64_t N, int scale_begin, int scale_end, int64_t row_stride, PassBLaunch& L) {
  L.dd = *d;
  L.dd.n_scales = scale_end;
  int rc = build_segs(d, L.st);
  if (rc) return rc;
  L.gps = (N + 255) / 256;
  L.grid = dim3((unsigned)ceil_div(L.gps * (scale_end - scale_begin) * L.st.n_planes, 4));
  L.max_res = 1;
  for (int s = scale_begin; s < scale_end; ++s)
    for (int k = 0; k < d->n_coords; ++k) L.max_res = L.max_res > d->res[s][k] ? L.max_res : d->res[s][k];
  const char* env = getenv("SNERF_PASSB_GROUPED");  // 1 (dev A-B) keeps scatter_grouped_kernel; read per call: tools/bench_passb.py flips it inside one process
  L.halfwave = !(env && atoi(env) != 0) && d->C == 32 && N * row_stride * 4 < (1LL << 32) && L.max_res * L.max_res * d->C * 4 < (1LL << 32) &&
               L.max_res < 65536;
  return 0;
}

template <int C, int NP>
static int launch_scatter_sorted(const snerf_kplanes_desc* d, int64_t N, const void* gvec, int gvec_bf16, const float4* sorted_n, float* gp, int scale_begin,
                                 int scale_end, hipStream_t st) {
  PassBLaunch L;
  int rc = passb_launch_make(d, N, scale_begin, scale_end, C, L);
  if (rc) return rc;
  const int seg0 = scale_begin * NP;
  if (C == 32 && N * C < (1LL << 31)) {  // 32-bit gvec row offsets inside the kernel
    if (!gvec_bf16 && L.halfwave) {
      hipLaunchKernelGGL((scatter_halfwave_kernel<NP, false>), L.grid, dim3(256), 0, st, L.dd, N, (const float*)gvec, sorted_n, gp, L.gps, seg0, L.st.per_scale,
                         nullptr, 0);
      SNERF_LAUNCH_CHECK("kplanes_scatter_halfwave");
      return 0;
    }
    if (gvec_bf16) hipLaunchKernelGGL((scatter_grouped_kernel<NP, __bf16>), L.grid, dim3(256), 0, st, L.dd, N, (const __bf16*)gvec, sorted_n, gp, L.gps, seg0,
                                      L.st.per_scale);
    else hipLaunchKernelGGL((scatter_grouped_kernel<NP, float>), L.grid, dim3(256), 0, st, L.dd, N, (const float*)gvec, sorted_n, gp, L.gps, seg0, L.st.per_scale);
    SNERF_LAUNCH_CHECK("kplanes_scatter_grouped");
    return 0;
  }
  constexpr int run = 256;  // entries per lane group, as the chunk kernels: L.gps groups per segment
  const dim3 grid((unsigned)ceil_div(L.gps * (scale_end - scale_begin) * NP * (2 * C), 256));
  if (gvec_bf16) hipLaunchKernelGGL((scatter_sorted_kernel<C, NP, __bf16>), grid, dim3(256), 0, st, L.dd, N, (const __bf16*)gvec, sorted_n, gp, run, L.gps, seg0,
                                    L.st.per_scale);
  else hipLaunchKernelGGL((scatter_sorted_kernel<C, NP, float>), grid, dim3(256), 0, st, L.dd, N, (const float*)gvec, sorted_n, gp, run, L.gps, seg0, L.st.per_scale);
  SNERF_LAUNCH_CHECK("kplanes_scatter_sorted");
  return 0;
}

extern "C" int snerf_kplanes_gradvec(const snerf_kplanes_desc* desc, const float* planes, const snerf_coords* coords, int64_t N, const float* grad_out,
                                     void* gvec, int32_t gvec_bf16, snerf_stream_t stream) {
  int rc = check_desc(desc, coords, N);
  if (rc) return rc;
  if (N == 0) return 0;
  SNERF_REQUIRE(planes && grad_out && gvec, "kplanes_gradvec: null buffer");
  DISPATCH_C_NP(launch_gradvec, desc, planes, coords, N, grad_out, gvec, gvec_bf16, (hipStream_t)stream);
}

extern "C" int snerf_kplanes_scatter_sorted_scales(const snerf_kplanes_desc* desc, int64_t N, const void* gvec, int32_t gvec_bf16, const float* sorted_rec,
                                                   float* grad_planes, int32_t scale_begin, int32_t scale_end, snerf_stream_t stream) {
  snerf_coords dummy = {};
  int rc = check_desc(desc, &dummy, N);
  if (rc) return rc;
  SNERF_REQUIRE(scale_begin >= 0 && scale_begin <= scale_end && scale_end <= desc->n_scales, "kplanes_scatter_sorted: scales [%d, %d) of %d",
                scale_begin, scale_end, desc->n_scales);
  if (N == 0 || scale_begin == scale_end) return 0;
  SNERF_REQUIRE(gvec && sorted_rec && grad_planes, "kplanes_scatter_sorted: null buffer");
  DISPATCH_C_NP(launch_scatter_sorted, desc, N, gvec, gvec_bf16, reinterpret_cast<const float4*>(sorted_rec), grad_planes, scale_begin, scale_end,
            (hipStream_t)stream);
}

extern "C" int snerf_kplanes_scatter_sorted(const snerf_kplanes_desc* desc, int64_t N, const void* gvec, int32_t gvec_bf16, const float* sorted_rec,
                                            float* grad_planes, snerf_stream_t stream) {
  SNERF_REQUIRE(desc, "kplanes_scatter_sorted: null descriptor");
  return snerf_kplanes_scatter_sorted_scales(desc, N, gvec, gvec_bf16, sorted_rec, grad_planes, 0, desc->n_scales, stream);
}

// ---- quotient form of the sorted scatter (snerf.h) ----
static int quotient_ok(const snerf_kplanes_desc* d, int64_t N) {
  SNERF_REQUIRE(d, "kplanes_quotient: null descriptor");
  SNERF_REQUIRE(d->C == 32 && d->concat == 1 && d->n_scales >= 1 && (int64_t)N * d->C * d->n_scales < (1LL << 31),
                "kplanes_quotient: built for C = 32, concatenated scales and N * 32 * n_scales < 2^31 (C=%d concat=%d N=%lld)", d->C, d->concat, (long long)N);
  return 0;
}

extern "C" int snerf_kplanes_quotient_supported(const snerf_kplanes_desc* desc, int64_t N) {
  return desc && desc->C == 32 && desc->concat == 1 && desc->n_scales >= 1 && N >= 0 && (int64_t)N * desc->C * desc->n_scales < (1LL << 31) &&
         (desc->n_coords == 3 || desc->n_coords == 4);
}

extern "C" int snerf_kplanes_quotient_prepare(const snerf_kplanes_desc* desc, int64_t N, const float* grad_feat, const float* feat, float* G,
                                              int32_t* fix_list, int32_t fix_capacity, int32_t* fix_count, int32_t* fix_count_next, snerf_stream_t stream) {
  int rc = quotient_ok(desc, N);
  if (rc) return rc;
  SNERF_REQUIRE(N >= 0 && fix_capacity >= 0, "kplanes_quotient_prepare: N=%lld capacity=%d", (long long)N, fix_capacity);
  SNERF_REQUIRE(fix_count, "kplanes_quotient_prepare: null counter");
  hipStream_t st = (hipStream_t)stream;
  if (!fix_count_next) {  // single counter: reset it here
    rc = check_hip(hipMemsetAsync(fix_count, 0, sizeof(int32_t), st), "kplanes_quotient_prepare memset");
    if (rc) return rc;
  }
  if (N == 0) {
    if (fix_count_next) return check_hip(hipMemsetAsync(fix_count_next, 0, sizeof(int32_t), st), "kplanes_quotient_prepare memset");
    return 0;
  }
  SNERF_REQUIRE(grad_feat && feat && G && (fix_list || fix_capacity == 0), "kplanes_quotient_prepare: null buffer");
  const int64_t rows = N * desc->n_scales;
  hipLaunchKernelGGL((quotient_prepare_kernel<32>), dim3((unsigned)ceil_div(rows * 8, 256)), dim3(256), 0, st, rows, grad_feat, feat, G, fix_list,
                     fix_capacity, fix_count, fix_count_next);
  SNERF_LAUNCH_CHECK("kplanes_quotient_prepare");
  return 0;
}

extern "C" int snerf_kplanes_scatter_quotient_scales(const snerf_kplanes_desc* desc, const float* planes, int64_t N, const float* G, const float* sorted_rec,
                                                     float* grad_planes, int32_t scale_begin, int32_t scale_end, snerf_stream_t stream) {
  int rc = quotient_ok(desc, N);
  if (rc) return rc;
  SNERF_REQUIRE(scale_begin >= 0 && scale_begin <= scale_end && scale_end <= desc->n_scales, "kplanes_scatter_quotient: scales [%d, %d) of %d",
                scale_begin, scale_end, desc->n_scales);
  if (N == 0 || scale_begin == scale_end) return 0;
  SNERF_REQUIRE(planes && G && sorted_rec && grad_planes, "kplanes_scatter_quotient: null buffer");
  const int stride = desc->C * desc->n_scales;
  PassBLaunch L;
  rc = passb_launch_make(desc, N, scale_begin, scale_end, stride, L);
  if (rc) return rc;
  // scatter_grouped_kernel addresses a plane's texels with 32-bit element offsets
  SNERF_REQUIRE(L.max_res * L.max_res * desc->C < (1LL << 31), "kplanes_scatter_quotient: plane of %lld^2 texels too large for 32-bit offsets",
                (long long)L.max_res);
  const int NP = L.st.n_planes, seg0 = scale_begin * NP;
  const float4* rec = reinterpret_cast<const float4*>(sorted_rec);
  hipStream_t st = (hipStream_t)stream;
  if (L.halfwave) {
    if (NP == 6) hipLaunchKernelGGL((scatter_halfwave_kernel<6, true>), L.grid, dim3(256), 0, st, L.dd, N, G, rec, grad_planes, L.gps, seg0, L.st.per_scale, planes, stride);
    else hipLaunchKernelGGL((scatter_halfwave_kernel<3, true>), L.grid, dim3(256), 0, st, L.dd, N, G, rec, grad_planes, L.gps, seg0, L.st.per_scale, planes, stride);
  } else {
    if (NP == 6) hipLaunchKernelGGL((scatter_grouped_kernel<6, float, true>), L.grid, dim3(256), 0, st, L.dd, N, G, rec, grad_planes, L.gps, seg0, L.st.per_scale, planes, stride);
    else hipLaunchKernelGGL((scatter_grouped_kernel<3, float, true>), L.grid, dim3(256), 0, st, L.dd, N, G, rec, grad_planes, L.gps, seg0, L.st.per_scale, planes, stride);
  }
  SNERF_LAUNCH_CHECK("kplanes_scatter_quotient");
  return 0;
}

extern "C" int snerf_kplanes_quotient_fixup(const snerf_kplanes_desc* desc, const float* planes, const snerf_coords* coords, int64_t N,
                                            const int32_t* fix_list, const int32_t* fix_count, int32_t fix_capacity, float* grad_planes,
                                            int32_t scale_begin, int32_t scale_end, int32_t* overflow_peak, snerf_stream_t stream) {
  int rc = check_desc(desc, coords, N);
  if (rc) return rc;
  rc = quotient_ok(desc, N);
  if (rc) return rc;
  SNERF_REQUIRE(scale_begin >= 0 && scale_begin <= scale_end && scale_end <= desc->n_scales, "kplanes_quotient_fixup: scales [%d, %d) of %d", scale_begin,
                scale_end, desc->n_scales);
  if (N == 0 || fix_capacity == 0 || scale_begin == scale_end) return 0;
  SNERF_REQUIRE(planes && fix_list && fix_count && grad_planes, "kplanes_quotient_fixup: null buffer");
  // a fixed small grid that strides over the (device-side) count: an empty list costs one launch
  hipStream_t st = (hipStream_t)stream;
  if (desc->n_coords == 4) hipLaunchKernelGGL((quotient_fixup_kernel<6>), dim3(64), dim3(256), 0, st, *desc, planes, *coords, fix_list, fix_count,
                                              fix_capacity, grad_planes, desc->n_scales, scale_begin, scale_end, overflow_peak);
  else hipLaunchKernelGGL((quotient_fixup_kernel<3>), dim3(64), dim3(256), 0, st, *desc, planes, *coords, fix_list, fix_count, fix_capacity,
                          grad_planes, desc->n_scales, scale_begin, scale_end, overflow_peak);
  SNERF_LAUNCH_CHECK("kplanes_quotient_fixup");
  return 0;
}
