"""Fused resize + center crop + normalize (ops.resize_crop_normalize).

Reference: fp64 numpy, dense per-axis weight matrices of the antialiased
triangle filter in exact integers, ``Wy @ img @ Wx^T`` per channel, crop,
normalize. Bound for the kernel: ``|out - ref| <= 2^-8 |ref| + 2e-5`` —
half a bf16 ulp plus the fp32 arithmetic of two passes of at most 9 taps
with exact weights (below about 7e-6 each in normalized units). A pass of
T > 9 taps sums T non-negative fp32 terms, each step within 2^-24 of the
running sum, so each tap past the ninth adds 2^-24 / min(std) per pass.
"""
import functools
import io

import numpy as np
import pandas as pd
import pytest
import torch

from mi355x_scale.ops import (resize_crop_geometry, resize_crop_normalize)
from mi355x_scale.ops.preprocess import IMAGENET_MEAN, IMAGENET_STD

# h x w -> (nh, nw, top, left) at 256/224, worked out by hand
SHAPES = {
    (256, 256): (256, 256, 16, 16),      # one tap, pure crop
    (37, 53): (256, 366, 16, 71),        # upscale, support 1
    (300, 257): (298, 256, 37, 16),      # nw exact
    (500, 375): (341, 256, 58, 16),      # 3 taps, 58.5 rounds to even
    (225, 900): (256, 1024, 16, 400),    # staging must skip the wings
    (1031, 777): (339, 256, 58, 16),     # 7-9 taps, 57.5 rounds to even
    (8, 300): (256, 9600, 16, 4688),     # extreme upscale
}


# (h, w, resize, crop): the kernel's column chunks and buffer ends
CHUNKED = [
    (37, 53, 300, 260),    # crop > 256 columns: chunks of 256 + 4
    (2750, 2750, 4, 4),    # a row of 8250 bytes does not fit the row buffer:
                           # the chunk halves to 2 columns; crop == resize on
                           # a square image whose last row ends 12 bytes past
                           # a 16-byte boundary, so the last vector of the
                           # buffer is loaded bytewise
]


@functools.lru_cache(maxsize=None)
def _image(h, w):
    if h * w > 1 << 20:   # averaged over ~700 taps noise would go flat: ramps
        y, x = np.mgrid[0:h, 0:w]
        img = np.stack([x * 255 // (w - 1), y * 255 // (h - 1),
                        (x + 2 * y) % 256], axis=-1).astype(np.uint8)
        return torch.from_numpy(img)
    rng = np.random.default_rng(1000 * h + w)
    return torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))


def _weights(n_in, n_out):
    o = np.arange(n_out, dtype=np.int64)[:, None]
    j = np.arange(n_in, dtype=np.int64)[None, :]
    d = 2 * max(n_in, n_out)
    wt = np.maximum(0, d - np.abs((2 * j + 1) * n_out - (2 * o + 1) * n_in))
    return wt / wt.sum(axis=1, keepdims=True, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _reference(h, w, resize=256, crop=224):
    """fp64 [3, crop, crop] for _image(h, w)."""
    nh, nw, top, left = resize_crop_geometry(h, w, resize, crop)
    wy = _weights(h, nh)[top:top + crop]
    wx = _weights(w, nw)[left:left + crop]
    rows = np.tensordot(wy, _image(h, w).double().numpy(), axes=(1, 0))
    x = np.tensordot(rows, wx, axes=(1, 1)).transpose(1, 0, 2)  # [c, y, x]
    mean = np.asarray(IMAGENET_MEAN)[:, None, None]
    std = np.asarray(IMAGENET_STD)[:, None, None]
    return (x / 255.0 - mean) / std


def _check(out, shapes, resize=256, crop=224, rel=2.0 ** -8, abs_=2e-5):
    assert out.dtype == torch.bfloat16
    assert out.shape == (len(shapes), 3, crop, crop)
    assert out.is_contiguous(memory_format=torch.channels_last)
    got = out.double().cpu().numpy()
    for i, (h, w) in enumerate(shapes):
        ref = _reference(h, w, resize, crop)
        taps = 2 * -(-min(h, w) // resize) + 1
        slack = abs_ + 2 * max(0, taps - 9) * 2.0 ** -24 / min(IMAGENET_STD)
        excess = np.abs(got[i] - ref) - (rel * np.abs(ref) + slack)
        print(f"resize_crop {h}x{w} -> {crop}: worst excess over the bound "
              f"{excess.max():.3g}, max |err| {np.abs(got[i] - ref).max():.3g}")
        assert np.isfinite(got[i]).all() and excess.max() <= 0, \
            f"{h}x{w}: {np.unravel_index(excess.argmax(), ref.shape)}"


# ------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("hw", list(SHAPES))
def test_gpu_single_image(hw):
    _check(resize_crop_normalize([_image(*hw).cuda()]), [hw])


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,resize,crop", CHUNKED)
def test_gpu_column_chunks(h, w, resize, crop):
    out = resize_crop_normalize([_image(h, w).cuda()], resize=resize,
                                crop=crop)
    _check(out, [(h, w)], resize=resize, crop=crop)


@pytest.mark.gpu
def test_gpu_packed_batch_and_canvas_bit_identical():
    """All shapes in one launch (odd byte offsets, blocks of different
    images), then from a 1040x912 canvas, with the sizes on the host
    (descriptors) and on the device (geometry in the kernel): same bits."""
    shapes = list(SHAPES)
    packed = resize_crop_normalize([_image(*s).cuda() for s in shapes])
    _check(packed, shapes)
    canvas = torch.zeros((len(shapes), 1040, 912, 3), dtype=torch.uint8)
    for i, (h, w) in enumerate(shapes):
        canvas[i, :h, :w] = _image(h, w)
    hw = torch.tensor(shapes, dtype=torch.int32)
    for sizes in (hw, hw.cuda()):
        got = resize_crop_normalize(canvas.cuda(), sizes)
        assert torch.equal(got.view(torch.int16), packed.view(torch.int16))


def _canvas_batch(shapes, hc=320, wc=272):
    canvas = torch.zeros((len(shapes), hc, wc, 3), dtype=torch.uint8)
    for i, (h, w) in enumerate(shapes):
        canvas[i, :h, :w] = _image(h, w)
    return {"image": canvas, "image_hw": torch.tensor(shapes, dtype=torch.int32),
            "label": torch.arange(len(shapes))}


@pytest.mark.gpu
def test_gpu_unpack_captured_in_graph_follows_new_sizes():
    """ImageClassifier._unpack on a loader batch with image_hw, captured
    into a graph on one batch and replayed on another of other sizes: no
    host read during capture, and the geometry is the replayed batch's."""
    from mi355x_scale.train import ImageClassifier
    model = ImageClassifier("resnet18", num_classes=10)
    first, second = [(256, 256), (300, 257)], [(37, 53), (225, 260)]
    static = {k: v.cuda() for k, v in _canvas_batch(first).items()}
    model._unpack(static)               # constants land before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x, _ = model._unpack(static)
    for k, v in _canvas_batch(second).items():
        static[k].copy_(v)
    for _ in range(2):
        graph.replay()
        _check(x, second)


@pytest.mark.gpu
def test_gpu_binding_rejects_descriptor_outside_buffer():
    from mi355x_scale.ops import _C
    from mi355x_scale.ops.preprocess import _consts
    flat = torch.zeros(3 * 300 * 257, dtype=torch.uint8, device="cuda")
    out = torch.empty((1, 3, 224, 224), dtype=torch.bfloat16,
                      device="cuda").contiguous(
                          memory_format=torch.channels_last)
    scale, shift = _consts(flat.device, IMAGENET_MEAN, IMAGENET_STD)
    # 300 x 257 from byte 1 of a buffer that holds exactly one such image
    desc = torch.tensor([[1, 300, 257, 771, 298, 256, 37, 16]],
                        dtype=torch.int32)
    with pytest.raises(RuntimeError, match="leaves"):
        _C.resize_crop_normalize(flat, desc.cuda(), desc, out, scale, shift,
                                 224)


@pytest.mark.gpu
def test_gpu_crop_33_store_tail_into_out():
    """Rows of 99 elements: no multiple of 8, so every row starts at
    another 16-byte phase; the result lands in the caller's ``out``."""
    shapes = [(37, 53), (300, 257)]
    out = torch.full((2, 3, 33, 33), -7.25, dtype=torch.bfloat16,
                     device="cuda").contiguous(
                         memory_format=torch.channels_last)
    got = resize_crop_normalize([_image(*s).cuda() for s in shapes],
                                resize=48, crop=33, out=out)
    assert got is out
    _check(out, shapes, resize=48, crop=33)


# ------------------------------------------------------------------- CPU
def test_geometry_hand_computed():
    for (h, w), want in SHAPES.items():
        assert resize_crop_geometry(h, w, 256, 224) == want
    assert resize_crop_geometry(37, 53, 48, 33) == (48, 68, 8, 18)


def test_cpu_path_against_reference():
    """torch's fp32 antialiased bilinear builds its weights from a float
    centre, so it is not held to the kernel's bound: measured against the
    fp64 reference on these shapes, the worst error beyond the half-ulp
    term is 5.2e-5 (at 300x257); 2e-4 leaves a margin of about 4 and is
    still far below what a wrong tap or offset gives (>= 1e-2)."""
    shapes = list(SHAPES)
    out = resize_crop_normalize([_image(*s) for s in shapes])
    _check(out, shapes, abs_=2e-4)
    hw = torch.tensor(shapes[:2])
    canvas = torch.zeros((2, 256, 256, 3), dtype=torch.uint8)
    for i, (h, w) in enumerate(shapes[:2]):
        canvas[i, :h, :w] = _image(h, w)
    assert torch.equal(resize_crop_normalize(canvas, hw), out[:2])


def test_rejects_bad_requests():
    img = _image(37, 53)
    with pytest.raises(ValueError, match="crop"):
        resize_crop_normalize([img], resize=224, crop=256)
    with pytest.raises(ValueError, match="2\\^31"):
        resize_crop_normalize([torch.zeros((8, 40000, 3),
                                           dtype=torch.uint8)])
    canvas = torch.zeros((1, 64, 64, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="larger than"):
        resize_crop_normalize(canvas, torch.tensor([[64, 65]]))
    from mi355x_scale.ops.preprocess import _resize_crop_descriptors
    for off, pitch in ((1, 159), (0, 158), (-1, 159)):  # 37x53 in 5883 bytes
        with pytest.raises(ValueError, match="leaves"):
            _resize_crop_descriptors([(37, 53)], [off], [pitch], 5883,
                                     256, 224)


def test_unpack_uses_image_hw_on_cpu():
    from mi355x_scale.train import ImageClassifier
    shapes = [(37, 53), (300, 257)]
    batch = _canvas_batch(shapes)
    x, y = ImageClassifier("resnet18", num_classes=10)._unpack(batch)
    assert x.dtype == torch.float32 and y.tolist() == [0, 1]
    want = resize_crop_normalize([_image(*s) for s in shapes])
    assert torch.equal(x, want.float())


def _jpeg(h, w):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(_image(h, w).numpy()).save(buf, "JPEG")
    return buf.getvalue()


def test_decode_jpeg_canvas():
    from mi355x_scale.data.generator import decode_jpeg_canvas
    pdf = pd.DataFrame({"image": [_jpeg(37, 53), _jpeg(300, 257)],
                        "label": [3, 4]})
    got = decode_jpeg_canvas(pdf, canvas_hw=(128, 160))
    assert got["image"].shape == (2, 128, 160, 3)
    assert got["image"].dtype == np.uint8
    assert got["image_hw"].dtype == np.int32
    # 300x257 does not fit 128x160: reduced by k = 3 to 100x86
    assert got["image_hw"].tolist() == [[37, 53], [100, 86]]
    assert not got["image"][0, 37:].any() and not got["image"][1, :, 86:].any()
    assert got["image"][1, :100, :86].any()
    assert got["label"].tolist() == [3, 4]


def test_classify_resize():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from mi355x_scale.serve import create_app
    app = create_app(model_name="resnet18", num_classes=10, device="cpu")
    img = _image(300, 257).tolist()
    with TestClient(app) as c:
        r = c.post("/classify", json={"image": img, "resize": 256})
        assert r.status_code == 200 and len(r.json()["classes"]) == 5
        r = c.post("/classify", json={"image": img, "resize": 200})
        assert r.status_code == 400
