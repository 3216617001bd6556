// Pixel draws inside image masks: a packed rank-select index of the mask and the per-step masked draw.
//
// Reference: PixelSampler.sample_method with a mask (NS/data/pixel_samplers.py:69-72) -- torch.nonzero(mask[..., 0]) over the whole image
// cache on EVERY step (an index list of 24 bytes per valid pixel: 31 GB at the K-Planes preset's 2500 x 540 x 960 cache), then a host-side
// random.sample and an index by a Python list (a host sync).  Here the mask is packed ONCE per image-cache refresh into one bit per pixel
// plus one count per block of 1024 pixels (snerf_mask_pack; the exclusive prefix of the counts is a cumsum at prepare time), and the
// per-step draw is one kernel with one lane per ray that maps two uniforms to a rank in [0, total) in exact integer arithmetic and selects
// the rank-th valid pixel: the row torch.nonzero(mask[..., 0])[rank] by construction, with no list, no host loop and no sync.
#include "common.hpp"

namespace snerf {

constexpr int MASK_BLOCK = 1024;                  // pixels per counted block: what one wavefront packs from one 16-byte load per lane
constexpr int MASK_BLOCK_WORDS = MASK_BLOCK / 32;

// bit k of the result = (byte k of x != 0).  Bit 7 of every byte of t is set iff the byte is non-zero (the low seven bits carry into it, or it
// is set already); the multiply gathers the four bits, moved to bit 0 of their bytes, into bits 24..27 (the sixteen partial products land on
// sixteen different bit positions, so nothing carries).
__device__ __forceinline__ uint32_t nonzero_bytes4(uint32_t x) {
  const uint32_t t = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;
  return ((((t >> 7) & 0x01010101u) * 0x01020408u) >> 24) & 0xfu;
}

// The 16 mask bytes at p as four little-endian dwords; only the first `left` bytes exist (left >= 1), the others read as zero.  ALIGN is what
// the chunk's base address allows: one 16-byte load, four 4-byte loads, or bytes.  A lane whose 16 bytes straddle the end takes byte loads.
template <int ALIGN>
__device__ __forceinline__ void load_mask16(const uint8_t* __restrict__ p, int64_t left, uint32_t (&w)[4]) {
  if (left >= 16) {
    if (ALIGN == 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      return;
    }
    if (ALIGN == 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = reinterpret_cast<const uint32_t*>(p)[j];
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = 0u;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < left) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
}

// One wavefront per block of 1024 pixels: lane l owns the 16 contiguous pixels [16 l, 16 l + 16) of the block, so the wave's load is one
// contiguous KiB and the lane's 16 compares are 16 CONTIGUOUS bits of the index -- half a word, joined with the neighbour lane's half by one
// shuffle.  (A wave ballot of "my byte is non-zero" would put pixel 16 l + k at bit l of ballot k: bits strided by 16 that would have to be
// transposed before they could be stored.)  chunk = the bytes of pixels [first_pixel, first_pixel + count); words and counts are written at
// their place in the whole index.
template <int ALIGN>
__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* __restrict__ chunk, int64_t count, uint32_t* __restrict__ bits,
                                                        int32_t* __restrict__ block_counts) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // wave-uniform
  const int64_t p0 = blk * MASK_BLOCK;
  if (p0 >= count) return;
  const int64_t p = p0 + lane * 16;
  uint32_t half = 0u;
  if (p < count) {
    uint32_t w[4];
    load_mask16<ALIGN>(chunk + p, count - p, w);
    half = nonzero_bytes4(w[0]) | (nonzero_bytes4(w[1]) << 4) | (nonzero_bytes4(w[2]) << 8) | (nonzero_bytes4(w[3]) << 12);
  }
  const uint32_t upper = __shfl_down(half, 1, 64);
  // word w of the block = lanes 2 w and 2 w + 1; it exists if its first pixel does (bits past the end are zero by the load above)
  if ((lane & 1) == 0 && p < count) bits[(p0 >> 5) + (lane >> 1)] = half | (upper << 16);
  int n = __popc(half);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if (lane == 0) block_counts[blk] = n;
}

// 24 bits of a uniform: floor(u * 2^24) clamped to [0, 2^24 - 1], NaN -> 0.  Exact for every torch.rand value (a multiple of 2^-24 below 1).
__device__ __forceinline__ uint64_t uniform_bits24(float u) {
  const float f = u * 16777216.0f;
  if (!(f >= 0.f)) return 0ull;
  return f < 16777215.0f ? (uint64_t)f : 16777215ull;
}

// One lane per ray, as sample_pixels_kernel (raygen.hip), with its fused gather.
__global__ void sample_pixels_masked_kernel(const float* __restrict__ u, int R, int64_t HW, int W, int64_t n_pixels,
                                            const uint32_t* __restrict__ bits, const int64_t* __restrict__ block_prefix, int64_t n_blocks,
                                            const uint8_t* __restrict__ images, int64_t* __restrict__ indices, float* __restrict__ target) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t total = block_prefix[n_blocks];  // on the device: the draw never syncs
  int64_t p = 0;                                 // an empty mask (refused when the index is built) draws pixel 0
  if (total > 0) {
    // rank = floor(v * total / 2^48) for v = hi * 2^24 + lo in [0, 2^48): below total, exact, monotone in v
    const uint64_t v = (uniform_bits24(u[(int64_t)r * 2]) << 24) | uniform_bits24(u[(int64_t)r * 2 + 1]);
    const int64_t rank = (int64_t)__umul64hi(v << 16, (uint64_t)total);
    // the last block b with block_prefix[b] <= rank = (first index in [1, n_blocks] whose prefix exceeds rank) - 1: an upper bound, so a run of
    // empty blocks (equal prefixes) is skipped.  block_prefix[n_blocks] = total > rank ends the search inside the array.
    int64_t lo = 1, hi = n_blocks;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (block_prefix[mid] > rank) hi = mid; else lo = mid + 1;
    }
    const int64_t b = lo - 1;
    int rem = (int)(rank - block_prefix[b]);  // < 1024
    // walk the block's words by popcount; the last block may hold fewer than 32 (bits has ceil(n_pixels / 32) words)
    const int64_t w0 = b * MASK_BLOCK_WORDS, n_words = (n_pixels + 31) >> 5;
    uint32_t word = 0u;
    int wsel = 0;
    bool found = false;
#pragma unroll 8
    for (int w = 0; w < MASK_BLOCK_WORDS; ++w) {
      const uint32_t x = (w0 + w < n_words) ? bits[w0 + w] : 0u;
      const int c = __popc(x);
      if (!found) {
        if (rem < c) { word = x; wsel = w; found = true; }
        else rem -= c;
      }
    }
    // the rem-th set bit of word: halve the window five times
    int bit = 0;
    uint32_t x = word;
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
      const int c = __popc(x & ((1u << s) - 1u));
      if (rem >= c) { rem -= c; bit += s; x >>= s; }
    }
    p = b * MASK_BLOCK + wsel * 32 + bit;
    p = p < n_pixels ? p : n_pixels - 1;  // unreachable with an index snerf_mask_pack wrote; keeps the gather inside the cache with any other
  }
  const int64_t c = p / HW, q = p % HW, y = q / W, x = q % W;
  indices[(int64_t)r * 3] = c; indices[(int64_t)r * 3 + 1] = y; indices[(int64_t)r * 3 + 2] = x;
  if (images) {
    const uint8_t* px = images + p * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) target[(int64_t)r * 3 + k] = (float)px[k] / 255.0f;  // as sample_pixels_kernel
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_mask_pack(const uint8_t* mask, int64_t n_pixels, int64_t first_pixel, int64_t count, uint32_t* bits, int32_t* block_counts,
                               snerf_stream_t stream) {
  SNERF_REQUIRE(n_pixels >= 1 && first_pixel >= 0 && count >= 0, "mask_pack: n_pixels=%lld first_pixel=%lld count=%lld", (long long)n_pixels,
                (long long)first_pixel, (long long)count);
  SNERF_REQUIRE(first_pixel % MASK_BLOCK == 0, "mask_pack: first_pixel=%lld is not a multiple of %d", (long long)first_pixel, MASK_BLOCK);
  SNERF_REQUIRE(first_pixel <= n_pixels && count <= n_pixels - first_pixel, "mask_pack: pixel range [%lld, %lld + %lld) outside the %lld pixels",
                (long long)first_pixel, (long long)first_pixel, (long long)count, (long long)n_pixels);
  SNERF_REQUIRE(count % MASK_BLOCK == 0 || first_pixel + count == n_pixels,
                "mask_pack: count=%lld is not a multiple of %d and the range does not end at the last pixel", (long long)count, MASK_BLOCK);
  if (count == 0) return 0;
  SNERF_REQUIRE(mask && bits && block_counts, "mask_pack: null buffer");
  const int64_t blocks = (count + MASK_BLOCK - 1) / MASK_BLOCK;
  SNERF_REQUIRE((blocks + 3) / 4 < (1LL << 31), "mask_pack: %lld blocks in one call: pack in chunks", (long long)blocks);
  uint32_t* words = bits + first_pixel / 32;
  int32_t* counts = block_counts + first_pixel / MASK_BLOCK;
  const dim3 grid((unsigned)((blocks + 3) / 4)), wg(256);  // four wavefronts = four blocks of pixels per workgroup
  const uintptr_t addr = reinterpret_cast<uintptr_t>(mask);
  if (addr % 16 == 0)
    hipLaunchKernelGGL(mask_pack_kernel<16>, grid, wg, 0, (hipStream_t)stream, mask, count, words, counts);
  else if (addr % 4 == 0)
    hipLaunchKernelGGL(mask_pack_kernel<4>, grid, wg, 0, (hipStream_t)stream, mask, count, words, counts);
  else
    hipLaunchKernelGGL(mask_pack_kernel<1>, grid, wg, 0, (hipStream_t)stream, mask, count, words, counts);
  SNERF_LAUNCH_CHECK("mask_pack");
  return 0;
}

extern "C" int snerf_sample_pixels_masked(const float* u, int32_t R, int32_t M, int32_t H, int32_t W, const uint32_t* bits,
                                          const int64_t* block_prefix, int64_t n_blocks, const uint8_t* images, int64_t* indices, float* target,
                                          snerf_stream_t stream) {
  SNERF_REQUIRE(R >= 0 && M >= 1 && H >= 1 && W >= 1, "sample_pixels_masked: R=%d M=%d H=%d W=%d", R, M, H, W);
  const int64_t n_pixels = (int64_t)M * H * W;
  SNERF_REQUIRE(n_blocks == (n_pixels + MASK_BLOCK - 1) / MASK_BLOCK, "sample_pixels_masked: n_blocks=%lld for %lld pixels (one per %d)",
                (long long)n_blocks, (long long)n_pixels, MASK_BLOCK);
  if (R == 0) return 0;
  SNERF_REQUIRE(u && bits && block_prefix && indices && (!images || target), "sample_pixels_masked: null buffer");
  hipLaunchKernelGGL(sample_pixels_masked_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, (hipStream_t)stream, u, R, (int64_t)H * W, W, n_pixels, bits,
                     block_prefix, n_blocks, images, indices, target);
  SNERF_LAUNCH_CHECK("sample_pixels_masked");
  return 0;
}
