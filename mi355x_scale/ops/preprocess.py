"""Device-side image preprocessing (fused uint8→bf16 normalize, and fused
resize + center crop + normalize of variable-size images).

GPU path: one HIP kernel (``csrc/preprocess.hip``) converts a uint8 NHWC
batch to a normalized bf16 channels-last tensor in a single HBM pass;
another (``csrc/resize_crop.hip``) does the same from decoded images of any
size, resampling on the way. CPU path (and the numerics reference in
tests): plain torch ops in fp32.

Replaces the reference's per-row CPU transform
(``deep_learning/2.distributed-data-loading-petastorm.py:282-296``).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

_consts_cache = {}


def _consts(device: torch.device, mean: Sequence[float],
            std: Sequence[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (device, tuple(mean), tuple(std))
    got = _consts_cache.get(key)
    if got is None:
        scale = torch.tensor([1.0 / (255.0 * s) for s in std],
                             dtype=torch.float32, device=device)
        shift = torch.tensor([-m / s for m, s in zip(mean, std)],
                             dtype=torch.float32, device=device)
        got = _consts_cache[key] = (scale, shift)
    return got


def normalize_images(images_u8: torch.Tensor,
                     mean: Sequence[float] = IMAGENET_MEAN,
                     std: Sequence[float] = IMAGENET_STD,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [N,H,W,3] → bf16 channels-last [N,3,H,W], (x/255 - mean)/std.

    On GPU this is the fused HIP kernel (mandatory — raises if the
    extension is missing). On CPU it is the torch reference path.
    """
    if images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"expected [N,H,W,3] uint8, got {tuple(images_u8.shape)}")
    n, h, w, _ = images_u8.shape
    if images_u8.is_cuda:
        from . import _C, require_ext, HAVE_EXT
        require_ext()
        images_u8 = images_u8.contiguous()
        if out is None:
            out = torch.empty((n, 3, h, w), dtype=torch.bfloat16,
                              device=images_u8.device,
                              memory_format=torch.channels_last)
        scale, shift = _consts(images_u8.device, mean, std)
        _C.normalize_u8_to_bf16(images_u8, out, scale, shift)
        return out
    # CPU / reference path (fp32 math, then cast) — also the test oracle.
    x = images_u8.to(torch.float32) / 255.0
    mean_t = torch.tensor(mean, dtype=torch.float32)
    std_t = torch.tensor(std, dtype=torch.float32)
    x = (x - mean_t) / std_t                      # [N,H,W,3]
    x = x.permute(0, 3, 1, 2)                     # [N,3,H,W] (view)
    return x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def resize_crop_geometry(h: int, w: int, resize: int = 256,
                         crop: int = 224) -> Tuple[int, int, int, int]:
    """``(nh, nw, top, left)`` of torchvision's ``Resize(resize)`` followed
    by ``CenterCrop(crop)`` on an ``h x w`` image: the short side becomes
    ``resize`` (``h`` on a tie), the long side ``int(resize * long / short)``,
    and the window starts at ``int(round((n - crop) / 2.0))`` per axis."""
    h, w, resize, crop = int(h), int(w), int(resize), int(crop)
    if h < 1 or w < 1:
        raise ValueError(f"image size must be positive, got {h}x{w}")
    if crop < 1 or crop > resize:
        raise ValueError(f"need 1 <= crop <= resize, got crop={crop}, "
                         f"resize={resize}")
    if h <= w:
        nh, nw = resize, resize * w // h
    else:
        nh, nw = resize * h // w, resize
    return (nh, nw, int(round((nh - crop) / 2.0)),
            int(round((nw - crop) / 2.0)))


def _resize_crop_descriptors(hw, offsets, pitches, nbytes: int, resize: int,
                             crop: int) -> np.ndarray:
    """int32 [N,8] kernel descriptors (offset, h, w, pitch, nh, nw, top,
    left), checked: every image inside the ``nbytes`` buffer, and the
    kernel's integer tap arithmetic inside int32."""
    desc = np.empty((len(hw), 8), dtype=np.int64)
    for i, ((h, w), off, pitch) in enumerate(zip(hw, offsets, pitches)):
        nh, nw, top, left = resize_crop_geometry(h, w, resize, crop)
        if 2 * max(h, w) * max(nh, nw) >= 2 ** 31:
            raise ValueError(
                f"image {i} ({h}x{w} -> {nh}x{nw}): 2 * n_in * n_out must "
                "stay below 2^31")
        if pitch < 3 * w or off < 0 or \
                off + (h - 1) * pitch + 3 * w > nbytes:
            raise ValueError(
                f"image {i} (offset {off}, {h}x{w}, pitch {pitch}) leaves "
                f"the {nbytes}-byte buffer")
        desc[i] = (off, h, w, pitch, nh, nw, top, left)
    if nbytes >= 2 ** 31:
        raise ValueError("image buffer must hold fewer than 2^31 bytes")
    return desc.astype(np.int32)


def _canvas_on_device(canvas: torch.Tensor, image_hw: torch.Tensor,
                      resize: int, crop: int, mean, std,
                      out: Optional[torch.Tensor]) -> torch.Tensor:
    """GPU canvas batch with ``image_hw`` on the device: the kernel derives
    the geometry itself (sizes clamped into the canvas), nothing is read
    back, and the call may be captured into a graph. Only the worst case
    the canvas admits can be checked: a 1-pixel short side."""
    from . import _C, require_ext
    require_ext()
    n, hc, wc, _ = canvas.shape
    if crop < 1 or crop > resize:
        raise ValueError(f"need 1 <= crop <= resize, got crop={crop}, "
                         f"resize={resize}")
    if tuple(image_hw.shape) != (n, 2):
        raise ValueError(f"image_hw must be [{n},2]")
    if 2 * resize * max(hc, wc) ** 2 >= 2 ** 31 or canvas.numel() >= 2 ** 31:
        raise ValueError(
            f"a {hc}x{wc} canvas admits images for which 2 * n_in * n_out "
            "reaches 2^31; pass image_hw on the host to check each image")
    if out is None:
        out = torch.empty((n, 3, crop, crop), dtype=torch.bfloat16,
                          device=canvas.device,
                          memory_format=torch.channels_last)
    scale, shift = _consts(canvas.device, mean, std)
    _C.resize_crop_normalize_canvas(
        canvas.contiguous(), image_hw.to(torch.int32).contiguous(), out,
        scale, shift, resize, crop)
    return out


def resize_crop_normalize(
        images: Union[torch.Tensor, Sequence[torch.Tensor]],
        image_hw=None, resize: int = 256, crop: int = 224,
        mean: Sequence[float] = IMAGENET_MEAN,
        std: Sequence[float] = IMAGENET_STD,
        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Variable-size uint8 images → bf16 channels-last [N,3,crop,crop]:
    ``Resize(resize)`` (antialiased bilinear) → ``CenterCrop(crop)`` →
    ``(x/255 - mean)/std``, without rounding to uint8 in between.

    ``images`` is a sequence of uint8 [h,w,3] tensors (packed into one flat
    buffer with a single ``torch.cat``), or a padded canvas [N,Hc,Wc,3] whose
    image ``i`` occupies the top-left ``image_hw[i] = (h, w)`` corner.

    On GPU this is one launch of the fused HIP kernel (mandatory — raises
    if the extension is missing). A GPU canvas with ``image_hw`` already on
    the device (what the loader delivers) is never read back: the kernel
    works out the geometry, clamping sizes into the canvas instead of
    raising, and the call can sit inside a captured graph. Sizes given on
    the host are checked one by one. On CPU it is the torch reference path:
    ``F.interpolate(antialias=True)`` in fp32 per image. An empty sequence
    yields an empty result on ``out``'s device, or on the CPU.
    """
    if out is not None and out.dtype != torch.bfloat16:
        raise ValueError("out must be bf16")
    if isinstance(images, torch.Tensor):
        if images.dim() != 4 or images.shape[-1] != 3 or \
                images.dtype != torch.uint8:
            raise ValueError("canvas must be uint8 [N,Hc,Wc,3], got "
                             f"{images.dtype} {tuple(images.shape)}")
        if image_hw is None:
            raise ValueError("a canvas batch needs image_hw [N,2]")
        n, hc, wc, _ = images.shape
        if out is not None and tuple(out.shape) != (n, 3, crop, crop):
            raise ValueError(f"out must be bf16 [{n},3,{crop},{crop}]")
        if images.is_cuda and isinstance(image_hw, torch.Tensor) \
                and image_hw.is_cuda:
            return _canvas_on_device(images, image_hw, resize, crop, mean,
                                     std, out)
        hw = np.asarray(image_hw.cpu() if isinstance(image_hw, torch.Tensor)
                        else image_hw, dtype=np.int64).reshape(-1, 2)
        if len(hw) != n:
            raise ValueError(f"image_hw must be [{n},2]")
        hw = [(int(h), int(w)) for h, w in hw]
        for i, (h, w) in enumerate(hw):
            if h > hc or w > wc:
                raise ValueError(f"image {i} ({h}x{w}) is larger than the "
                                 f"{hc}x{wc} canvas")
        offsets = [i * hc * wc * 3 for i in range(n)]
        pitches = [3 * wc] * n
        flat = images.contiguous().reshape(-1)
    else:
        images = list(images)
        if image_hw is not None:
            raise ValueError("image_hw goes with a canvas batch only")
        for t in images:
            if t.dim() != 3 or t.shape[-1] != 3 or t.dtype != torch.uint8:
                raise ValueError("expected uint8 [h,w,3] images, got "
                                 f"{t.dtype} {tuple(t.shape)}")
        hw = [(int(t.shape[0]), int(t.shape[1])) for t in images]
        sizes = [3 * h * w for h, w in hw]
        offsets = [0] + list(np.cumsum(sizes[:-1], dtype=np.int64))
        pitches = [3 * w for _, w in hw]
        flat = torch.cat([t.reshape(-1) for t in images]) if images else \
            torch.empty(0, dtype=torch.uint8,
                        device=out.device if out is not None else "cpu")
    n = len(hw)
    desc = _resize_crop_descriptors(hw, offsets, pitches, flat.numel(),
                                    resize, crop)
    if out is not None and tuple(out.shape) != (n, 3, crop, crop):
        raise ValueError(f"out must be bf16 [{n},3,{crop},{crop}]")
    if flat.is_cuda:
        from . import _C, require_ext
        require_ext()
        if out is None:
            out = torch.empty((n, 3, crop, crop), dtype=torch.bfloat16,
                              device=flat.device,
                              memory_format=torch.channels_last)
        scale, shift = _consts(flat.device, mean, std)
        desc_cpu = torch.from_numpy(desc)
        _C.resize_crop_normalize(flat, desc_cpu.to(flat.device), desc_cpu,
                                 out, scale, shift, crop)
        return out
    # CPU / reference path: torch's own antialiased bilinear, fp32.
    mean_t = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    std_t = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    res = torch.empty((n, 3, crop, crop), dtype=torch.bfloat16).contiguous(
        memory_format=torch.channels_last) if out is None else out
    for i, (off, h, w, pitch, nh, nw, top, left) in enumerate(desc.tolist()):
        img = flat[off:off + h * pitch].reshape(h, pitch // 3, 3)[:, :w]
        x = img.permute(2, 0, 1).unsqueeze(0).to(torch.float32)
        x = F.interpolate(x, size=(nh, nw), mode="bilinear",
                          antialias=True, align_corners=False)
        x = x[:, :, top:top + crop, left:left + crop]
        res[i] = ((x / 255.0 - mean_t) / std_t)[0].to(torch.bfloat16)
    return res
