"""Host side of the masked pixel draw: the ABI surface of snerf_mask_pack / snerf_sample_pixels_masked, the rank arithmetic restated in Python
integers (tests/mask_reference.py), dataparsers.load_mask_cache, synthetic.add_broadcast_overlay and what the samplers refuse without a device.
Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mask_reference as MR
from tests.conftest import ROOT

NEW = ("snerf_mask_pack", "snerf_sample_pixels_masked")
TOTALS = (1, 2, 3, 1000, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 40)


def test_new_entries_declared_exported_and_bound():
    from soccernerfs_amd import _lib

    raw = open(os.path.join(ROOT, "include", "snerf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    l = _lib.lib()
    for s in NEW:
        assert re.search(r"\bint\s+" + s + r"\s*\(", txt), s
        assert s in _lib.EXPORTS and hasattr(l, s), s
    P, I, L = C.c_void_p, C.c_int32, C.c_int64
    assert l.snerf_mask_pack.argtypes == [P, L, L, L, P, P, P]
    assert l.snerf_sample_pixels_masked.argtypes == [P, I, I, I, I, P, P, L, P, P, P, P]
    # the header's argument lists, type by type
    args = lambda name: [re.sub(r"\s*\w+$", "", a.strip()) for a in re.search(name + r"\s*\(([^)]*)\)", txt).group(1).split(",")]
    assert args("snerf_mask_pack") == ["const uint8_t*", "int64_t", "int64_t", "int64_t", "uint32_t*", "int32_t*", "snerf_stream_t"]
    assert args("snerf_sample_pixels_masked") == ["const float*", "int32_t", "int32_t", "int32_t", "int32_t", "const uint32_t*", "const int64_t*", "int64_t",
                                                  "const uint8_t*", "int64_t*", "float*", "snerf_stream_t"]
    # each entry cites the reference lines it replaces
    for s in NEW:
        comment = re.findall(r"/\*.*?\*/", raw[:raw.index("int " + s + "(")], flags=re.S)[-1]
        assert "pixel_samplers.py:69-72" in comment, s
    # no new revision: the entries are part of revision 2's surface
    assert int(re.search(r"#define\s+SNERF_ABI_REVISION\s+(\d+)", raw).group(1)) == _lib.ABI_REVISION == l.snerf_abi_revision() == 2
    assert int(re.search(r"#define\s+SNERF_ABI_VERSION\s+(\d+)", raw).group(1)) == _lib.ABI_VERSION == l.snerf_abi_version() == 16
    # an older library must fail at load: both are in the signature table, every name of which the loader requires
    # (tests/test_binding_cpu.py::test_stale_library_fails_at_load loads a library without them)
    assert _lib.SIGNATURES["snerf_mask_pack"] == "s:PLLLPPP" and _lib.SIGNATURES["snerf_sample_pixels_masked"] == "s:PIIIIPPLPPPP"


def test_new_entries_validate_their_arguments():
    """Null buffers, a first_pixel off the 1024 grid, a range outside the mask and bad sizes are refused on the host, before anything is launched."""
    from soccernerfs_amd import _lib

    l = _lib.lib()
    err = l.snerf_last_error
    assert l.snerf_mask_pack(None, 4096, 0, 4096, None, None, None) < 0 and b"null" in err()
    assert l.snerf_mask_pack(None, 4096, 1000, 1024, None, None, None) < 0 and b"first_pixel=1000" in err() and b"1024" in err()
    assert l.snerf_mask_pack(None, 4096, 32, 1024, None, None, None) < 0 and b"first_pixel=32" in err()
    assert l.snerf_mask_pack(None, 4096, 3072, 1025, None, None, None) < 0 and b"outside" in err()
    assert l.snerf_mask_pack(None, 4096, 5120, 0, None, None, None) < 0 and b"outside" in err()
    assert l.snerf_mask_pack(None, 4096, 0, -1, None, None, None) < 0
    assert l.snerf_mask_pack(None, 0, 0, 0, None, None, None) < 0
    assert l.snerf_mask_pack(None, 4096, 1024, 100, None, None, None) < 0 and b"count=100" in err()  # a chunk that ends inside the mask, off the grid
    assert l.snerf_mask_pack(None, 4096, 1024, 0, None, None, None) == 0  # nothing to do
    assert l.snerf_sample_pixels_masked(None, 4, 1, 1, 1, None, None, 1, None, None, None, None) < 0 and b"null" in err()
    assert l.snerf_sample_pixels_masked(None, 4, 0, 1, 1, None, None, 1, None, None, None, None) < 0 and b"M=0" in err()
    assert l.snerf_sample_pixels_masked(None, -1, 1, 1, 1, None, None, 1, None, None, None, None) < 0 and b"R=-1" in err()
    assert l.snerf_sample_pixels_masked(None, 4, 2, 32, 32, None, None, 1, None, None, None, None) < 0 and b"n_blocks=1" in err()
    assert l.snerf_sample_pixels_masked(None, 0, 2, 32, 32, None, None, 2, None, None, None, None) == 0  # nothing to do


@pytest.mark.parametrize("total", TOTALS)
def test_rank_arithmetic(total):
    top = MR.SPAN - 1
    assert MR.rank_of_v(0, total) == 0 and MR.rank_of_v(top, total) == total - 1  # the largest v maps to the last rank
    rng = np.random.default_rng(total % 9973)
    ks = sorted(k for k in {0, 1, 2, total // 3, total // 2, total - 3, total - 2, total - 1, *rng.integers(0, total, 200).tolist()} if 0 <= k < total)
    for k in ks:
        v = MR.v_for_rank(k, total)
        assert 0 <= v <= top and v * total >= k * MR.SPAN > (v - 1) * total  # v = ceil(k 2^48 / total)
        assert MR.rank_of_v(v, total) == k
        if k > 0:
            assert MR.rank_of_v(v - 1, total) == k - 1
        u0, u1 = MR.uniforms_for_rank(k, total)
        assert u0.dtype == u1.dtype == np.float32 and 0 <= u0 < 1 and 0 <= u1 < 1
        assert MR.v_of(u0, u1) == v and MR.rank(u0, u1, total) == k  # round trip through float32
    # monotone in v: over random sorted v, and over every v next to a rank boundary
    vs = np.sort(rng.integers(0, MR.SPAN, 2000)).tolist() + [top]
    rs = [MR.rank_of_v(v, total) for v in vs]
    assert all(a <= b for a, b in zip(rs, rs[1:])) and 0 <= rs[0] and rs[-1] == total - 1
    # the kernel's form: __umul64hi(v << 16, total)
    for v in vs[::50] + [MR.v_for_rank(k, total) for k in ks[:20]]:
        assert MR.rank_of_v(v, total) == ((v << 16) * total) >> 64 and (v << 16) < 2 ** 64


def test_uniform_bits():
    assert MR.bits24(0.0) == 0 and MR.bits24(np.float32(1 - 2 ** -24)) == MR.ONE - 1
    assert MR.bits24(1.0) == MR.ONE - 1 and MR.bits24(7.5) == MR.ONE - 1 and MR.bits24(-0.25) == 0 and MR.bits24(float("nan")) == 0
    assert MR.bits24(float("inf")) == MR.ONE - 1 and MR.bits24(float("-inf")) == 0
    # torch.rand values are multiples of 2^-24 below 1: the 24 bits are the value
    u = torch.rand(4096, generator=torch.Generator().manual_seed(3))
    assert all(MR.bits24(x) / MR.ONE == float(x) for x in u.tolist())
    vs = np.array([0, 1, MR.ONE - 1, MR.ONE, MR.SPAN - 1, 123456789012345], dtype=np.int64)
    pairs = MR.uniforms_for_vs(vs)
    assert pairs.dtype == np.float32 and [MR.v_of(a, b) for a, b in pairs] == vs.tolist()
    assert MR.vs_for_ranks([0, 5, 999], 1000).tolist() == [MR.v_for_rank(k, 1000) for k in (0, 5, 999)]


def test_pack_reference():
    m = np.zeros(1025 + 40, dtype=np.uint8)
    m[[0, 31, 32, 1023, 1024, 1064]] = [1, 2, 255, 1, 7, 1]
    words, counts = MR.pack(m)
    assert words.dtype == np.uint32 and words.size == 34 and counts.tolist() == [4, 2]
    assert words[0] == (1 | 1 << 31) and words[1] == 1 and words[31] == 1 << 31 and words[32] == 1 and words[33] == 1 << 8


def _write_masks(tmp_path, arrays, mode):
    from PIL import Image

    files = []
    for i, a in enumerate(arrays):
        f = tmp_path / f"mask_{mode}_{i}.png"
        Image.fromarray(a).convert(mode).save(f)
        files.append(f)
    return files


def test_load_mask_cache(tmp_path):
    from PIL import Image

    from soccernerfs_amd.dataparsers import load_mask_cache

    rng = np.random.default_rng(7)
    H, W = 18, 26
    grey = [(rng.integers(0, 4, (H, W)) * 85).astype(np.uint8) for _ in range(3)]  # values 0, 85, 170, 255
    for mode in ("L", "1"):
        files = _write_masks(tmp_path, grey, mode)
        got = load_mask_cache(files)
        assert got.dtype == torch.bool and tuple(got.shape) == (3, H, W, 1) and not got.is_cuda
        for i, f in enumerate(files):
            want = torch.from_numpy(np.array(Image.open(f))).bool()  # .bool() of the file
            assert torch.equal(got[i, :, :, 0], want)
            # mode L keeps every non-zero grey level valid; mode 1 thresholds when the file is written
            assert mode != "L" or torch.equal(want, torch.from_numpy(grey[i] != 0))
        assert 0 < int(got.sum()) < got.numel()
        half = load_mask_cache(files, scale_factor=0.5)
        assert tuple(half.shape) == (3, int(H * 0.5), int(W * 0.5), 1)
        for i, f in enumerate(files):
            want = np.array(Image.open(f).resize((int(W * 0.5), int(H * 0.5)), resample=Image.NEAREST))
            assert torch.equal(half[i, :, :, 0], torch.from_numpy(want).bool())
    odd = load_mask_cache(_write_masks(tmp_path, [np.ascontiguousarray(g[:, :25]) for g in grey], "L"), scale_factor=0.3)
    assert tuple(odd.shape) == (3, int(H * 0.3), int(25 * 0.3), 1)
    rgb = _write_masks(tmp_path, [np.stack([grey[0]] * 3, -1)], "RGB")
    with pytest.raises(ValueError, match="1 channel"):
        load_mask_cache(rgb)


def test_mask_and_image_shapes_are_checked_by_the_sampler():
    from soccernerfs_amd.pixel_samplers import DynamicBasedPixelSampler, EquirectangularPixelSampler, PixelSampler

    for cls in (PixelSampler, EquirectangularPixelSampler):
        for bad in (torch.ones(2, 4, 5, 1, dtype=torch.bool), torch.ones(3, 4, 4, 1, dtype=torch.bool), torch.ones(2, 4, 4, 3, dtype=torch.bool)):
            with pytest.raises(ValueError, match="different shapes"):
                cls(8).sample_method(8, 2, 4, 4, mask=bad, device="cpu")
    batch = {"image": torch.zeros(2, 4, 4, 3, dtype=torch.uint8), "image_idx": torch.arange(2), "mask": torch.ones(2, 4, 6, 1, dtype=torch.bool)}
    with pytest.raises(ValueError, match="different shapes"):
        PixelSampler(8).sample(batch)
    with pytest.raises(ValueError, match="different shapes"):
        PixelSampler.prepare_mask(batch)
    with pytest.raises(ValueError, match="different shapes"):
        DynamicBasedPixelSampler(8).sample(dict(batch, ist_weights=None))


def test_a_host_mask_is_still_refused():
    """The library has no host draw: a mask that is not on the HIP device raises NotImplementedError, in every sampler and through sample()."""
    from soccernerfs_amd import ops
    from soccernerfs_amd.pixel_samplers import DynamicBasedPixelSampler, EquirectangularPixelSampler, PixelSampler

    mask = torch.ones(2, 4, 4, 1, dtype=torch.bool)
    batch = {"image": torch.zeros(2, 4, 4, 3, dtype=torch.uint8), "image_idx": torch.arange(2), "mask": mask}
    for cls in (PixelSampler, EquirectangularPixelSampler, DynamicBasedPixelSampler):
        with pytest.raises(NotImplementedError, match="HIP device"):
            cls(8).sample_method(8, 2, 4, 4, mask=mask, batch=dict(batch, ist_weights=None), device="cpu")
        with pytest.raises(NotImplementedError, match="HIP device"):
            cls(8).sample(dict(batch, ist_weights=None))
    with pytest.raises(NotImplementedError):
        PixelSampler.prepare_mask(dict(batch))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.MaskIndex.from_mask(mask)
    with pytest.raises(ValueError, match="chunk_pixels"):
        ops.MaskIndex.from_host(mask, "cpu", chunk_pixels=1000)
    assert DynamicBasedPixelSampler(8).mask_ist_weights is False and DynamicBasedPixelSampler(8, mask_ist_weights=True).mask_ist_weights is True


def test_mask_ist_weights_zero_the_maps_outside_the_mask():
    """DynamicBasedPixelSampler.prepare(batch, mask_ist_weights=True): the prefix sums of the maps with the masked-out weights at zero; the
    default leaves today's tables as they are (plain torch: runs on the host)."""
    from soccernerfs_amd.pixel_samplers import DynamicBasedPixelSampler

    gen = torch.Generator().manual_seed(11)
    w = torch.rand(3, 6, 7, generator=gen).half()
    mask = torch.rand(3, 6, 7, 1, generator=gen) > 0.4
    mask[1] = False
    plain = DynamicBasedPixelSampler.prepare({"ist_weights": w})
    same = DynamicBasedPixelSampler.prepare({"ist_weights": w, "mask": mask})
    for k in ("ist_cdf", "ist_nonempty", "ist_nnz"):
        assert torch.equal(plain[k], same[k]), k
    got = DynamicBasedPixelSampler.prepare({"ist_weights": w, "mask": mask}, mask_ist_weights=True)
    wm = (w * mask[..., 0]).reshape(3, -1)
    assert torch.equal(got["ist_cdf"], torch.cumsum(wm.float(), 1)) and got["ist_nonempty"].tolist() == [0, 2]
    assert torch.equal(got["ist_nnz"], (wm > 0).sum(1).to(torch.int32)) and got["ist_nnz"][1] == 0
    with pytest.raises(ValueError, match="byte mask"):
        DynamicBasedPixelSampler.prepare({"ist_weights": w}, mask_ist_weights=True)
    with pytest.raises(ValueError, match="different shapes"):
        DynamicBasedPixelSampler.prepare({"ist_weights": w, "mask": mask[:2]}, mask_ist_weights=True)


def test_broadcast_overlay():
    from soccernerfs_amd import synthetic

    M, H, W = 5, 20, 40
    gen = torch.Generator().manual_seed(5)
    clean = torch.randint(0, 256, (M, H, W, 3), dtype=torch.uint8, generator=gen)
    data = {"images": clean.clone(), "times": torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])}
    box = (2, 6, 10, 30)
    mask = synthetic.add_broadcast_overlay(data, box, colour=(1, 2, 3), stripe_colour=(250, 251, 252))
    assert mask.dtype == torch.bool and tuple(mask.shape) == (M, H, W, 1)
    inside = torch.zeros(M, H, W, dtype=torch.bool)
    inside[:, 2:6, 10:30] = True
    assert torch.equal(mask[..., 0], ~inside)
    assert torch.equal(data["images"][~inside], clean[~inside])  # nothing outside the box changes
    banner = data["images"][:, 2:6, 10:30]
    is_bg, is_stripe = (banner == torch.tensor([1, 2, 3], dtype=torch.uint8)).all(-1), (banner == torch.tensor([250, 251, 252], dtype=torch.uint8)).all(-1)
    assert bool((is_bg | is_stripe).all())
    starts = []
    for m in range(M):
        cols = is_stripe[m].all(0).nonzero()[:, 0].tolist()  # whole columns of the box
        assert cols == list(range(cols[0], cols[0] + 2)) and int(is_stripe[m].sum()) == 4 * 2  # a tenth of 20 columns
        starts.append(cols[0])
    assert starts == [0, 4, 9, 13, 18]  # floor(t * (20 - 2)): the clock moves with the frame time
    with pytest.raises(ValueError):
        synthetic.add_broadcast_overlay(data, (2, 6, 30, 41))
