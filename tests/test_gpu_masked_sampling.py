"""GPU: pixel draws inside image masks (snerf_mask_pack, snerf_sample_pixels_masked, ops.MaskIndex and the samplers above them).

The definition the draw is held to is the reference's own (NS/data/pixel_samplers.py:70): the valid pixels are the rows of
torch.nonzero(mask[..., 0]), in row-major order, and a draw is row `rank` of that list for rank = floor(v * total / 2^48)
(tests/mask_reference.py restates the arithmetic in Python integers).  Everything is integers: every comparison is exact equality.
The packed index is compared with numpy.packbits(bitorder="little") and per-block sums."""
import numpy as np
import pytest
import torch

from tests import mask_reference as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_WORD, SENTINEL_COUNT, GUARD = 0x5A5A5A5A, -7, 4
PACK_SIZES = (1, 31, 32, 33, 1023, 1024, 1025, 2065, 105, 4096)
FILLS = ("zeros", "ones", "half", "sparse", "last")
SHAPES = ((1, 1, 1), (3, 5, 7), (2, 33, 31), (4, 32, 32), (2, 64, 80))


def _fill(kind, n, rng):
    if kind == "zeros":
        return np.zeros(n, dtype=bool)
    if kind == "ones":
        return np.ones(n, dtype=bool)
    if kind == "half":
        return rng.random(n) < 0.5
    if kind == "sparse":
        return rng.random(n) < 1e-3
    m = np.zeros(n, dtype=bool)
    m[-1] = True  # only the last pixel
    return m


def _as_dtype(valid, dtype, rng):
    if dtype == "bool":
        return torch.from_numpy(valid)
    return torch.from_numpy(np.where(valid, rng.choice(np.array([1, 2, 255], dtype=np.uint8), valid.size), 0).astype(np.uint8))  # values {0, 1, 2, 255}


def _pack(mask_dev_bytes, n, first=0, bits=None, counts=None):
    """ops.mask_pack into guarded buffers: GUARD sentinel elements behind bits and block_counts."""
    from soccernerfs_amd import ops

    nw, nb = -(-n // 32), -(-n // 1024)
    if bits is None:
        bits = torch.full((nw + GUARD,), SENTINEL_WORD, dtype=torch.int32, device=DEV)
        counts = torch.full((nb + GUARD,), SENTINEL_COUNT, dtype=torch.int32, device=DEV)
    ops.mask_pack(mask_dev_bytes, n, first, bits, counts)
    return bits, counts


def _check_packed(bits, counts, valid):
    n = valid.size
    words, block_counts = MR.pack(valid)
    got_bits, got_counts = bits.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(got_bits[:words.size].view(np.uint32), words)
    assert np.array_equal(got_counts[:block_counts.size], block_counts)
    assert (got_bits[words.size:] == SENTINEL_WORD).all() and got_bits.size == words.size + GUARD      # nothing behind the last word
    assert (got_counts[block_counts.size:] == SENTINEL_COUNT).all() and got_counts.size == block_counts.size + GUARD
    assert int(block_counts.sum()) == int(valid.sum()) and block_counts.size == -(-n // 1024)


@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack(n):
    from soccernerfs_amd import ops

    rng = np.random.default_rng(n)
    for kind in FILLS:
        valid = _fill(kind, n, rng)
        for dtype in ("bool", "uint8"):
            host = _as_dtype(valid, dtype, rng)
            dev_bytes = ops._mask_bytes(host.to(DEV), "test")
            assert dev_bytes.data_ptr() % 16 == 0
            _check_packed(*_pack(dev_bytes, n), valid)


@pytest.mark.parametrize("offset", (4, 8, 1, 2, 3, 16))
def test_pack_at_every_alignment_of_the_mask(offset):
    """A base address that allows 16-byte loads, only 4-byte loads, or neither (a byte-offset view): the same index, and no byte outside the
    view is read as mask (the bytes around it are non-zero)."""
    rng = np.random.default_rng(offset)
    for n in (1, 15, 16, 17, 33, 1023, 1024, 1025, 2065):
        valid = rng.random(n) < 0.5
        buf = torch.full((offset + n + 64,), 255, dtype=torch.uint8, device=DEV)
        buf[offset:offset + n] = torch.from_numpy(valid.astype(np.uint8) * 3).to(DEV)
        view = buf[offset:offset + n]
        assert view.data_ptr() % 16 == offset % 16
        _check_packed(*_pack(view, n), valid)


def test_pack_in_chunks():
    """Chunks at first_pixel 0, 1024 and 3072 write the index one call writes."""
    n = 4096 + 105
    rng = np.random.default_rng(1)
    valid = rng.random(n) < 0.3
    dev = torch.from_numpy(valid.astype(np.uint8)).to(DEV)
    whole_bits, whole_counts = _pack(dev, n)
    _check_packed(whole_bits, whole_counts, valid)
    bits, counts = None, None
    for first, last in ((3072, n), (0, 1024), (1024, 3072)):  # in any order
        bits, counts = _pack(dev[first:last].clone(), n, first, bits, counts)
    assert torch.equal(bits, whole_bits) and torch.equal(counts, whole_counts)
    # a chunk writes its own range only
    bits2, counts2 = _pack(dev[1024:3072].clone(), n, 1024)
    got = bits2.cpu().numpy()
    assert (got[:32] == SENTINEL_WORD).all() and (got[96:] == SENTINEL_WORD).all() and np.array_equal(got[32:96], whole_bits.cpu().numpy()[32:96])
    assert counts2.cpu().numpy().tolist()[:5] == [SENTINEL_COUNT] + whole_counts.cpu().numpy().tolist()[1:3] + [SENTINEL_COUNT] * 2


def test_mask_index_from_mask_and_from_host():
    from soccernerfs_amd import ops

    gen = torch.Generator().manual_seed(2)
    mask = torch.rand(3, 37, 41, 1, generator=gen) < 0.6  # 4551 pixels: 5 blocks, the last partial
    a = ops.MaskIndex.from_mask(mask.to(DEV))
    words, counts = MR.pack(mask.numpy())
    assert a.shape == (3, 37, 41) and a.n_pixels == 4551 and a.n_blocks == 5 and a.total == int(mask.sum())
    assert np.array_equal(a.bits.cpu().numpy().view(np.uint32), words) and np.array_equal(a.block_counts.cpu().numpy(), counts)
    assert a.block_prefix.dtype == torch.int64 and a.block_prefix.cpu().tolist() == [0] + np.cumsum(counts).tolist()
    for variant in (ops.MaskIndex.from_mask(mask[..., 0].to(DEV)), ops.MaskIndex.from_mask(mask.to(torch.uint8).to(DEV) * 255),
                    ops.MaskIndex.from_host(mask, DEV, chunk_pixels=1024), ops.MaskIndex.from_host(mask[..., 0], DEV, chunk_pixels=2048),
                    ops.MaskIndex.from_host(mask, DEV)):
        assert variant.shape == a.shape and variant.total == a.total
        assert torch.equal(variant.bits, a.bits) and torch.equal(variant.block_counts, a.block_counts) and torch.equal(variant.block_prefix, a.block_prefix)
    with pytest.raises(ValueError, match="no valid pixel"):
        ops.MaskIndex.from_mask(torch.zeros(2, 8, 8, 1, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="no valid pixel"):
        ops.MaskIndex.from_host(torch.zeros(2, 40, 40, dtype=torch.uint8), DEV, chunk_pixels=1024)
    with pytest.raises(RuntimeError):
        ops.MaskIndex.from_mask(torch.ones(2, 8, 8, device=DEV))  # a float mask


def _masks_of(shape, rng):
    n = int(np.prod(shape))
    out = {"random": rng.random(n) < 0.5, "ones": np.ones(n, dtype=bool)}
    if not out["random"].any():
        out["random"][0] = True
    # valid pixels in the first and in the last block only
    ends = np.zeros(n, dtype=bool)
    ends[:1024] = rng.random(min(n, 1024)) < 0.25
    ends[(n - 1) // 1024 * 1024:] = rng.random(n - (n - 1) // 1024 * 1024) < 0.25
    ends[0] = ends[-1] = True
    out["ends"] = ends
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_select_every_rank(shape):
    from soccernerfs_amd import ops

    M, H, W = shape
    rng = np.random.default_rng(M * H * W)
    for name, valid in _masks_of(shape, rng).items():
        if name == "ends" and shape == (2, 64, 80):
            blocks = valid.reshape(-1, 1024).any(1)
            assert blocks[0] and blocks[-1] and not blocks[1:-1].any() and blocks.size - 2 >= 3  # at least three empty blocks between them
        mask = torch.from_numpy(valid.reshape(M, H, W, 1))
        index = ops.MaskIndex.from_mask(mask.to(DEV))
        rows = torch.nonzero(mask[..., 0])  # the definition, on the host
        total = rows.shape[0]
        assert index.total == total
        ks = np.arange(total)
        first_v = MR.vs_for_ranks(ks, total)           # the smallest v of every rank ...
        for vs, want in ((first_v, rows), (first_v[1:] - 1, rows[:-1]),  # ... and the v just below it: the previous rank
                         (np.array([MR.SPAN - 1]), rows[-1:])):      # the largest v: the last valid pixel
            if vs.size == 0:
                continue
            u = torch.from_numpy(MR.uniforms_for_vs(vs)).to(DEV)
            idx, target = ops.sample_pixels_masked(u, index, M, H, W)
            assert target is None and idx.dtype == torch.int64 and tuple(idx.shape) == (vs.size, 3)
            assert torch.equal(idx.cpu(), want), (name, shape)


@pytest.mark.parametrize("R", (1, 63, 64, 65, 257))
def test_select_ragged_batches(R):
    """Ragged last wavefronts and workgroups; rows behind the R-th stay untouched; non-rand uniforms (NaN, negative, >= 1) are clamped."""
    from soccernerfs_amd import _lib, ops

    M, H, W = 2, 33, 31
    gen = torch.Generator().manual_seed(R)
    mask = torch.rand(M, H, W, 1, generator=gen) < 0.4
    index = ops.MaskIndex.from_mask(mask.to(DEV))
    rows = torch.nonzero(mask[..., 0])
    u = torch.rand(R, 2, generator=gen)
    u[0] = torch.tensor([float("nan"), -1.0])
    if R > 2:
        u[1], u[2] = torch.tensor([1.0, 5.0]), torch.tensor([float("inf"), float("nan")])
    want = rows[[MR.rank(a, b, index.total) for a, b in u.numpy()]]
    ud = u.to(DEV)
    idx = torch.full((R + GUARD, 3), -5, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().snerf_sample_pixels_masked(ops._ptr(ud), R, M, H, W, ops._ptr(index.bits), ops._ptr(index.block_prefix), index.n_blocks, None,
                                                     ops._ptr(idx), None, ops._stream()), "sample_pixels_masked")
    assert torch.equal(idx[:R].cpu(), want) and bool((idx[R:] == -5).all())
    assert torch.equal(want[0], rows[0]) and (R <= 2 or torch.equal(want[1], rows[-1]))


@pytest.fixture(scope="module")
def big():
    """(5, 2048, 2048): 20 971 520 pixels, more than the 2^24 a single float32 uniform tells apart."""
    M, H, W = 5, 2048, 2048
    n = M * H * W
    rng = np.random.default_rng(24)
    ks = np.unique(np.concatenate([rng.integers(0, n, 4000), [0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, n - 2, n - 1]]))
    return M, H, W, n, ks


def _decode(p, H, W):
    return torch.stack((p // (H * W), (p % (H * W)) // W, p % W), dim=1)


def test_more_pixels_than_one_float_resolves(big):
    from soccernerfs_amd import ops

    M, H, W, n, ks = big
    assert n > 2 ** 24
    index = ops.MaskIndex.from_mask(torch.ones(M, H, W, dtype=torch.bool, device=DEV))
    assert index.total == n and index.n_blocks == n // 1024
    # rank == flat index
    u = torch.from_numpy(MR.uniforms_for_vs(MR.vs_for_ranks(ks, n))).to(DEV)
    idx, _ = ops.sample_pixels_masked(u, index, M, H, W)
    assert torch.equal(idx.cpu(), _decode(torch.from_numpy(ks), H, W))
    # draws that differ ONLY in u1 land on different pixels: 2^24 values of u0 cannot reach 20 971 520 pixels (n / 2^24 = 1.25 ranks per step of
    # u0, so the low uniform decides between neighbours)
    hi = torch.arange(0, 2 ** 24, 4099, dtype=torch.int64)
    u0 = (hi.double() / 2 ** 24).float()
    pair = lambda u1: torch.stack((u0, torch.full_like(u0, u1)), 1)
    lo_idx, _ = ops.sample_pixels_masked(pair(0.0).to(DEV), index, M, H, W)
    hi_idx, _ = ops.sample_pixels_masked(pair(1 - 2 ** -24).to(DEV), index, M, H, W)
    flat = lambda t: (t[:, 0] * H + t[:, 1]) * W + t[:, 2]
    want_lo = torch.tensor([MR.rank_of_v(int(h) << 24, n) for h in hi])
    want_hi = torch.tensor([MR.rank_of_v((int(h) << 24) + 2 ** 24 - 1, n) for h in hi])
    assert torch.equal(flat(lo_idx).cpu(), want_lo) and torch.equal(flat(hi_idx).cpu(), want_hi)
    assert bool((want_hi > want_lo).all()) and bool((want_hi - want_lo <= 2).all())
    # every pixel between two neighbouring values of u0 is reached by some u1
    h = 12345
    lo_steps = torch.arange(0, 2 ** 24, 2 ** 16, dtype=torch.int64)
    u = torch.stack((torch.full((lo_steps.numel(),), h / 2 ** 24, dtype=torch.float64), lo_steps.double() / 2 ** 24), 1).float()
    idx, _ = ops.sample_pixels_masked(u.to(DEV), index, M, H, W)
    assert sorted(set(flat(idx).cpu().tolist())) == list(range(MR.rank_of_v(h << 24, n), MR.rank_of_v(((h + 1) << 24) - 1, n) + 1))


def test_large_mask_with_holes_against_nonzero(big):
    """The same cache with every third pixel cleared: the draw is row `rank` of torch.nonzero."""
    from soccernerfs_amd import ops

    M, H, W, n, ks = big
    mask = (torch.arange(n, device=DEV) % 3 != 0).view(M, H, W, 1)
    index = ops.MaskIndex.from_mask(mask)
    rows = torch.nonzero(mask[..., 0])
    total = rows.shape[0]
    assert index.total == total == n - (n + 2) // 3 and total < 2 ** 24  # the draw still takes both uniforms: ranks are exact
    ks = np.unique(np.concatenate([ks[ks < total], [total - 1]]))
    first_v = MR.vs_for_ranks(ks, total)
    idx, _ = ops.sample_pixels_masked(torch.from_numpy(MR.uniforms_for_vs(first_v)).to(DEV), index, M, H, W)
    assert torch.equal(idx, rows[torch.from_numpy(ks).to(DEV)])
    idx, _ = ops.sample_pixels_masked(torch.from_numpy(MR.uniforms_for_vs(first_v[1:] - 1)).to(DEV), index, M, H, W)
    assert torch.equal(idx, rows[torch.from_numpy(ks[1:] - 1).to(DEV)])
    # torch.rand draws: every one lands inside the mask, and on the row its rank names
    u = torch.rand(4096, 2, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    idx, _ = ops.sample_pixels_masked(u, index, M, H, W)
    assert bool(mask[idx[:, 0], idx[:, 1], idx[:, 2], 0].all())
    want = [MR.rank(a, b, total) for a, b in u.cpu().numpy()]
    assert torch.equal(idx, rows[torch.tensor(want, device=DEV)])


@pytest.fixture(scope="module")
def scene():
    """A small image cache with its mask: (4, 33, 47), 6204 pixels = 7 blocks; one image fully masked out."""
    M, H, W = 4, 33, 47
    gen = torch.Generator().manual_seed(8)
    images = torch.randint(0, 256, (M, H, W, 3), dtype=torch.uint8, generator=gen).to(DEV)
    mask = torch.rand(M, H, W, 1, generator=gen) < 0.5
    mask[:, :6, :20] = False  # a banner
    mask[2] = False
    return M, H, W, images, mask.to(DEV)


def test_fused_gather(scene):
    from soccernerfs_amd import ops

    M, H, W, images, mask = scene
    index = ops.MaskIndex.from_mask(mask)
    u = torch.rand(777, 2, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    idx, target = ops.sample_pixels_masked(u, index, M, H, W, images)
    idx_only, none = ops.sample_pixels_masked(u, index, M, H, W)
    assert none is None and torch.equal(idx, idx_only)
    # uint8 -> float32 / 255 evaluated on the HOST (a correctly rounded division, what the kernel restates): the device library divides a tensor
    # by a scalar as a product with its reciprocal, which is one ulp off on some values
    want = images.cpu()[idx[:, 0].cpu(), idx[:, 1].cpu(), idx[:, 2].cpu()].float() / 255.0
    assert target.dtype == torch.float32 and torch.equal(target.cpu(), want)
    assert bool(mask[idx[:, 0], idx[:, 1], idx[:, 2], 0].all()) and 2 not in idx[:, 0].tolist()
    with pytest.raises(ValueError):
        ops.sample_pixels_masked(u, index, M, H, W + 1)
    with pytest.raises(RuntimeError):
        ops.sample_pixels_masked(u, index, M, H, W, images.float())
    with pytest.raises(RuntimeError):
        ops.sample_pixels_masked(torch.rand(8, 3, device=DEV), index, M, H, W)


def _batch(scene, **extra):
    M, H, W, images, mask = scene
    return {"image": images, "image_idx": torch.arange(M, device=DEV) + 10, "mask": mask, **extra}


def test_pixel_sampler_draws_inside_the_mask(scene):
    from soccernerfs_amd import ops
    from soccernerfs_amd.pixel_samplers import PixelSampler

    M, H, W, images, mask = scene
    R = 300
    batch = _batch(scene)
    torch.manual_seed(31)
    out = PixelSampler(R).sample(batch)
    assert isinstance(batch["mask_index"], ops.MaskIndex)  # built at the first draw and kept, as "ist_cdf" is
    torch.manual_seed(31)
    want, _ = ops.sample_pixels_masked(torch.rand((R, 2), device=DEV), ops.MaskIndex.from_mask(mask), M, H, W)
    c, y, x = want[:, 0], want[:, 1], want[:, 2]
    assert torch.equal(out["indices"][:, 1:], want[:, 1:]) and torch.equal(out["indices"][:, 0], c + 10)
    assert bool(mask[c, y, x, 0].all())
    assert out["mask"].dtype == torch.bool and tuple(out["mask"].shape) == (R, 1) and bool(out["mask"].all())
    assert torch.equal(out["image"], images[c, y, x].float() / 255.0)
    assert set(out) == {"image", "mask", "indices"}
    # the second draw reuses the index
    kept = batch["mask_index"]
    PixelSampler(R).sample(batch)
    assert batch["mask_index"] is kept
    # prepared up front, and a batch that holds ONLY the packed index: the same draws
    prepared = PixelSampler.prepare_mask(_batch(scene))
    assert torch.equal(prepared["mask_index"].bits, kept.bits)
    only_index = {"image": images, "image_idx": batch["image_idx"], "mask_index": kept}
    torch.manual_seed(31)
    out2 = PixelSampler(R).sample(only_index)
    assert set(out2) == set(out) and all(torch.equal(out2[k], out[k]) for k in out)
    # an all-zero mask is refused when its index is built
    with pytest.raises(ValueError, match="no valid pixel"):
        PixelSampler(R).sample({"image": images, "image_idx": batch["image_idx"], "mask": torch.zeros_like(mask)})


def test_samplers_without_a_mask_draw_what_they_drew(scene):
    """No mask: the launches and the bits of the unmasked draw (torch.rand((R, 3)) through snerf_sample_pixels_uniform), and no "mask" key."""
    from soccernerfs_amd import ops
    from soccernerfs_amd.pixel_samplers import DynamicBasedPixelSampler, PixelSampler

    M, H, W, images, _ = scene
    R = 256
    plain = {"image": images, "image_idx": torch.arange(M, device=DEV)}
    torch.manual_seed(41)
    out = PixelSampler(R).sample(plain)
    torch.manual_seed(41)
    want, _ = ops.sample_pixels_uniform(torch.rand((R, 3), device=DEV), M, H, W)
    assert torch.equal(out["indices"], want) and set(out) == {"image", "indices"} and "mask_index" not in plain
    # the IST sampler past its start: the random stream up to the uniform tail is the one of today's code (randperm, rand(n), rand((R - n, 3)))
    w = torch.rand(M, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(42)).half()
    batch = dict(plain, ist_weights=w, iter_steps=10)
    sampler = DynamicBasedPixelSampler(R, is_pixel_ratio=0.5, iters_to_start_ist=5)
    torch.manual_seed(43)
    idx = sampler.sample_method(R, M, H, W, batch=batch, device=DEV)
    n = 128  # floor(0.5 * 256) importance draws, all from one image (10 * ceil(128 / 4) = 320 per image)
    torch.manual_seed(43)
    torch.randperm(M, device=DEV)
    torch.rand(n, device=DEV)
    tail, _ = ops.sample_pixels_uniform(torch.rand((R - n, 3), device=DEV), M, H, W)
    assert tuple(idx.shape) == (R, 3) and torch.equal(idx[n:], tail) and len(set(idx[:n, 0].tolist())) == 1


def test_dynamic_sampler_with_a_mask(scene):
    from soccernerfs_amd import ops
    from soccernerfs_amd.pixel_samplers import DynamicBasedPixelSampler

    M, H, W, images, mask = scene
    R, n = 256, 128
    w = torch.rand(M, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(52)).half() + 0.01  # every pixel has weight
    inside = lambda idx: mask[idx[:, 0], idx[:, 1], idx[:, 2], 0]
    # before the start: the masked uniform draw
    batch = _batch(scene, ist_weights=w, iter_steps=0)
    sampler = DynamicBasedPixelSampler(R, is_pixel_ratio=0.5, iters_to_start_ist=5)
    torch.manual_seed(53)
    idx = sampler.sample_method(R, M, H, W, mask=mask, batch=batch, device=DEV)
    torch.manual_seed(53)
    want, _ = ops.sample_pixels_masked(torch.rand((R, 2), device=DEV), batch["mask_index"], M, H, W)
    assert torch.equal(idx, want) and bool(inside(idx).all())
    # past the start: the uniform tail is inside the mask; the importance part ignores the mask, as the reference's does (about half of every
    # image is masked out and every pixel has weight: 128 importance draws that all miss the masked-out half have probability ~2^-128)
    batch["iter_steps"] = 10
    out = sampler.sample(batch)
    idx = out["indices"].clone()
    idx[:, 0] -= 10
    assert bool(inside(idx[n:]).all()) and not bool(inside(idx[:n]).all())
    assert torch.equal(out["image"], images[idx[:, 0], idx[:, 1], idx[:, 2]].float() / 255.0) and tuple(out["mask"].shape) == (R, 1)
    # mask_ist_weights: the maps are zeroed outside the mask when they are prepared, so every draw is inside -- image 2 (all masked out) is never drawn
    batch2 = _batch(scene, ist_weights=w, iter_steps=10)
    strict = DynamicBasedPixelSampler(R, is_pixel_ratio=0.5, iters_to_start_ist=5, mask_ist_weights=True)
    for _ in range(3):
        idx = strict.sample_method(R, M, H, W, mask=mask, batch=batch2, device=DEV)
        assert tuple(idx.shape) == (R, 3) and bool(inside(idx).all())
    assert batch2["ist_nonempty"].tolist() == [0, 1, 3] and torch.equal(batch2["ist_cdf"], torch.cumsum((w * mask[..., 0]).reshape(M, -1).float(), 1))


def test_equirectangular_sampler_with_a_mask(scene):
    from soccernerfs_amd import ops
    from soccernerfs_amd.pixel_samplers import EquirectangularPixelSampler

    M, H, W, images, mask = scene
    R = 200
    batch = _batch(scene)
    torch.manual_seed(61)
    out = EquirectangularPixelSampler(R).sample(batch)
    torch.manual_seed(61)
    want, _ = ops.sample_pixels_masked(torch.rand((R, 2), device=DEV), ops.MaskIndex.from_mask(mask), M, H, W)
    assert torch.equal(out["indices"][:, 1:], want[:, 1:]) and torch.equal(out["indices"][:, 0], want[:, 0] + 10) and bool(out["mask"].all())
    # without a mask it still draws on the sphere
    torch.manual_seed(62)
    plain = EquirectangularPixelSampler(R).sample_method(R, M, H, W, device=DEV)
    torch.manual_seed(62)
    assert torch.equal(plain, ops.sample_pixels_sphere(torch.rand((R, 3), device=DEV), M, H, W)[0])
