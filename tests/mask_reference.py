"""The rank arithmetic of the masked pixel draw (snerf_sample_pixels_masked, include/snerf.h) in Python integers, and the definition the draw is
held to: the rank-th row of torch.nonzero(mask[..., 0]) (NS/data/pixel_samplers.py:70), the valid pixels in row-major order."""
import math

import numpy as np

BITS = 24
ONE = 1 << BITS        # 2^24: what a float32 uniform resolves
SPAN = 1 << (2 * BITS)  # 2^48: the values v takes


def bits24(u) -> int:
    """floor(u * 2^24) clamped to [0, 2^24 - 1], NaN -> 0; u is taken as the float32 it is stored as (the product is exact in a double)."""
    f = float(np.float32(u)) * ONE
    if math.isnan(f) or f < 0:
        return 0
    return ONE - 1 if f >= ONE - 1 else int(math.floor(f))


def v_of(u0, u1) -> int:
    return bits24(u0) * ONE + bits24(u1)


def rank_of_v(v: int, total: int) -> int:
    return (v * total) >> (2 * BITS)


def rank(u0, u1, total: int) -> int:
    """rank = floor(v * total / 2^48), v = floor(u0 * 2^24) * 2^24 + floor(u1 * 2^24)."""
    return rank_of_v(v_of(u0, u1), total)


def v_for_rank(k: int, total: int) -> int:
    """The smallest v that maps to rank k: ceil(k * 2^48 / total)."""
    return -((-k * SPAN) // total)


def uniforms_for_v(v: int):
    """The float32 pair (u0, u1) with v_of(u0, u1) == v: multiples of 2^-24 below 1, exact in float32."""
    assert 0 <= v < SPAN
    return np.float32((v >> BITS) / ONE), np.float32((v & (ONE - 1)) / ONE)


def uniforms_for_rank(k: int, total: int):
    return uniforms_for_v(v_for_rank(k, total))


def uniforms_for_vs(vs) -> np.ndarray:
    """uniforms_for_v for an int64 array of v: float32 [n,2]."""
    vs = np.asarray(vs, dtype=np.int64)
    assert vs.min() >= 0 and vs.max() < SPAN
    return np.stack(((vs >> BITS).astype(np.float64) / ONE, (vs & (ONE - 1)).astype(np.float64) / ONE), axis=1).astype(np.float32)


def vs_for_ranks(ks, total: int) -> np.ndarray:
    """v_for_rank for many ranks: int64 [n] (Python integers inside: k * 2^48 does not fit 64 bits)."""
    return np.array([v_for_rank(int(k), total) for k in np.asarray(ks).reshape(-1)], dtype=np.int64)


def pack(mask_flat: np.ndarray):
    """The index snerf_mask_pack writes for a flat byte mask: (uint32 words [ceil(n / 32)] in numpy.packbits' little bit order, int32 counts of
    every block of 1024 pixels)."""
    valid = np.asarray(mask_flat).reshape(-1) != 0
    n = valid.size
    by = np.packbits(valid, bitorder="little")
    by = np.concatenate([by, np.zeros((-by.size) % 4, dtype=np.uint8)])
    words = by.view("<u4").astype(np.uint32)
    assert words.size == -(-n // 32)
    padded = np.concatenate([valid, np.zeros((-n) % 1024, dtype=bool)])
    return words, padded.reshape(-1, 1024).sum(1).astype(np.int32)
