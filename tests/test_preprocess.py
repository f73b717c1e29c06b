import numpy as np
import pytest
import torch

from mi355x_scale.ops.preprocess import (IMAGENET_MEAN, IMAGENET_STD,
                                         normalize_images)


def _reference_fp32(u8_nhwc: torch.Tensor) -> torch.Tensor:
    x = u8_nhwc.to(torch.float32) / 255.0
    mean = torch.tensor(IMAGENET_MEAN)
    std = torch.tensor(IMAGENET_STD)
    return ((x - mean) / std).permute(0, 3, 1, 2)


def test_normalize_cpu_matches_reference():
    torch.manual_seed(0)
    x = torch.randint(0, 256, (2, 8, 8, 3), dtype=torch.uint8)
    out = normalize_images(x)
    ref = _reference_fp32(x)
    assert out.shape == (2, 3, 8, 8)
    assert torch.allclose(out.float(), ref, atol=1e-2)  # bf16 rounding


@pytest.mark.gpu
def test_normalize_gpu_kernel_vs_cpu_fp32():
    """HIP kernel vs plain fp32 torch reference (SURVEY §4 numerics rule)."""
    torch.manual_seed(0)
    x = torch.randint(0, 256, (4, 224, 224, 3), dtype=torch.uint8)
    ref = _reference_fp32(x)
    out = normalize_images(x.cuda()).float().cpu()
    # bf16 has ~3 decimal digits; normalized range ~[-2.2, 2.7]
    assert (out - ref).abs().max() < 2e-2
    # channel order must not be swapped: check per-channel means
    for c in range(3):
        assert abs(out[:, c].mean() - ref[:, c].mean()) < 1e-2


@pytest.mark.gpu
def test_normalize_gpu_is_channels_last_bf16():
    x = torch.randint(0, 256, (2, 32, 32, 3), dtype=torch.uint8).cuda()
    out = normalize_images(x)
    assert out.dtype == torch.bfloat16
    assert out.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.gpu
def test_normalize_gpu_odd_sizes():
    """Tail path: n not a multiple of 16 lanes*16B."""
    x = torch.randint(0, 256, (1, 7, 9, 3), dtype=torch.uint8)
    ref = _reference_fp32(x)
    out = normalize_images(x.cuda()).float().cpu()
    assert (out - ref).abs().max() < 2e-2


# ------------------------------------------------ half-ulp bound, every byte
# The reference is ((x / 255 - mean) / std) in float64. Per element
#     |out - ref| <= 2^(floor(log2 |ref|) - 8)
#                    + 2^-22 (|mean / std| + 1 / std)
# The first term is half a bf16 ulp of ref: the kernel must round to
# nearest, a truncating cast errs by up to a whole ulp. The second is the
# slack for the float32 scale and shift constants and the fma, each within
# 2^-24 of |mean / std| + 1 / std; about 1.6e-6 for the ImageNet constants.
OTHER_MEAN = (0.5, 0.25, 0.1)
OTHER_STD = (0.5, 0.3, 1.7)


def _ref64_and_bound(values, channels, mean, std):
    """float64 reference and bound for byte values at given channels."""
    mean = np.asarray(mean, dtype=np.float64)[channels]
    std = np.asarray(std, dtype=np.float64)[channels]
    ref = (np.asarray(values, dtype=np.float64) / 255.0 - mean) / std
    assert (ref != 0).all()
    half_ulp = 2.0 ** (np.floor(np.log2(np.abs(ref))) - 8)
    slack = 2.0 ** -22 * (np.abs(mean / std) + 1.0 / std)
    return ref, half_ulp + slack


def _pattern_u8(shape):
    """Pixel k is (k % 256, (k + 85) % 256, (k + 170) % 256): from 256
    pixels on, all 768 (value, channel) pairs occur."""
    n, h, w, c = shape
    k = np.arange(n * h * w, dtype=np.int64)[:, None]
    x = (k + np.array([0, 85, 170])) % 256
    return torch.from_numpy(x.astype(np.uint8).reshape(shape))


def _emulate_kernel(values, channels, mean, std, truncate=False):
    """The kernel's arithmetic on the CPU: float32 scale and shift as
    ops/preprocess.py builds them, one fma, then bf16 round-to-nearest-
    even (or, to show what the bound rejects, truncation)."""
    scale = np.array([1.0 / (255.0 * s) for s in std], dtype=np.float32)
    shift = np.array([-m / s for m, s in zip(mean, std)], dtype=np.float32)
    v = np.asarray(values, dtype=np.float64)    # the product is exact
    r = (v * scale[channels].astype(np.float64)
         + shift[channels].astype(np.float64)).astype(np.float32)
    if truncate:
        bits = r.view(np.uint32) & np.uint32(0xFFFF0000)
        return bits.view(np.float32).astype(np.float64)
    return torch.from_numpy(r).bfloat16().double().numpy()


@pytest.mark.parametrize("mean,std", [(IMAGENET_MEAN, IMAGENET_STD),
                                      (OTHER_MEAN, OTHER_STD)])
def test_normalize_bound_table_rne_passes_truncation_fails(mean, std):
    """All 256 x 3 (value, channel) pairs: fma then round-to-nearest-even
    stays inside the bound; truncation to bf16 leaves it, in every
    channel."""
    values = np.repeat(np.arange(256), 3)
    channels = np.tile(np.arange(3), 256)
    ref, bound = _ref64_and_bound(values, channels, mean, std)
    rne = np.abs(_emulate_kernel(values, channels, mean, std) - ref) / bound
    cut = np.abs(_emulate_kernel(values, channels, mean, std, truncate=True)
                 - ref) / bound
    per_channel = [int((cut[channels == c] > 1).sum()) for c in range(3)]
    print(f"normalize table std={std}: rne worst={rne.max():.4g} of the "
          f"bound, truncation worst={cut.max():.4g}, outside per channel "
          f"{per_channel}")
    assert rne.max() <= 1.0
    assert all(k > 0 for k in per_channel)


def _check_normalized(out, x_u8, mean, std, tag):
    n, h, w, _ = x_u8.shape
    assert out.dtype == torch.bfloat16
    assert out.shape == (n, 3, h, w)
    assert out.is_contiguous(memory_format=torch.channels_last)
    got = out.permute(0, 2, 3, 1).cpu().contiguous().double().numpy()
    # reference and bound depend on (value, channel) alone: one table
    ref, bound = _ref64_and_bound(np.repeat(np.arange(256), 3),
                                  np.tile(np.arange(3), 256), mean, std)
    pair = x_u8.numpy().reshape(-1, 3).astype(np.int64) * 3 + np.arange(3)
    pair = pair.reshape(-1)
    ratio = np.abs(got.reshape(-1) - ref[pair]) / bound[pair]
    worst = float(ratio.max())
    print(f"normalize {tag} {tuple(x_u8.shape)}: worst={worst:.4g} of the "
          "bound")
    assert np.isfinite(ratio).all() and worst <= 1.0, \
        f"{tag}: element {int(ratio.argmax())} at {worst:.4g} of the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [
    (2, 13, 11, 3),       # 858 bytes: 53 vectors + tail of 10, all pairs
    (1, 17, 17, 3),       # tail of 3
    (1, 1, 5, 3),         # 15 bytes: tail only
    (1, 2365, 2365, 3),   # 16,779,675 bytes: 2,459 past the first sweep,
                          # vectors and the 11-byte tail in the second
])
def test_normalize_gpu_half_ulp_bound(shape):
    x = _pattern_u8(shape)
    if shape[1] * shape[2] >= 256:
        flat = x.reshape(-1, 3).long()
        pairs = torch.unique(flat * 3 + torch.arange(3))
        assert pairs.numel() == 768
    out = normalize_images(x.cuda())
    _check_normalized(out, x, IMAGENET_MEAN, IMAGENET_STD, "imagenet")


@pytest.mark.gpu
def test_normalize_gpu_other_constants():
    x = _pattern_u8((2, 13, 11, 3))
    out = normalize_images(x.cuda(), mean=OTHER_MEAN, std=OTHER_STD)
    _check_normalized(out, x, OTHER_MEAN, OTHER_STD, "other constants")


@pytest.mark.gpu
def test_normalize_gpu_writes_caller_supplied_out():
    x = _pattern_u8((2, 13, 11, 3))
    out = torch.full((2, 3, 13, 11), -7.25, dtype=torch.bfloat16,
                     device="cuda").contiguous(
                         memory_format=torch.channels_last)
    got = normalize_images(x.cuda(), out=out)
    assert got is out
    _check_normalized(out, x, IMAGENET_MEAN, IMAGENET_STD, "out=")
