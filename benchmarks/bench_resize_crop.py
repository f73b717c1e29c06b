"""Fused resize + center crop + normalize kernel (ops/csrc/resize_crop.hip)
and the loader with and without device-side resampling. Needs an MI355X.

  1. kernel time for 256 canvas images decoded from the write_jpeg_parquet
     size distribution (device events, warm, window >= 0.5 s), against the
     byte floor: source bytes the kernel has to stage + output bytes, at
     6.9 TB/s, the best streaming rate this project has recorded for one of
     its own kernels (the one-gradient BN backward reduce, NOTES_NEXT.md);
  2. loader rows/s, ImageStreamDataModule(image_format="jpeg") with
     device_resize off and on, same workers, alternating, three runs each.
     Both deliver the normalized bf16 batch on the device.

    python benchmarks/bench_resize_crop.py --rows 2048
"""
import argparse
import json
import os
import sys
import tempfile
import time

import pyarrow.parquet as pq
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from mi355x_scale.data.generator import (decode_jpeg_canvas,  # noqa: E402
                                         write_jpeg_parquet)
from mi355x_scale.ops import (_C, normalize_images,  # noqa: E402
                              resize_crop_geometry, resize_crop_normalize)
from mi355x_scale.ops.preprocess import (IMAGENET_MEAN,  # noqa: E402
                                         IMAGENET_STD, _consts,
                                         _resize_crop_descriptors)

FLOOR_BYTES_PER_S = 6.9e12


def _taps(o, n_in, n_out):
    m = max(n_in, n_out)
    a = (2 * o + 1) * n_in + n_out
    return max(0, (a - 2 * m) // (2 * n_out)), \
        min(n_in, (a + 2 * m) // (2 * n_out))


def floor_bytes(hw, crop=224, resize=256):
    """Source bytes inside the crop's tap reach, once each, + bf16 output."""
    total = 0
    for h, w in hw:
        nh, nw, top, left = resize_crop_geometry(h, w, resize, crop)
        r_lo, r_hi = _taps(top, h, nh)[0], _taps(top + crop - 1, h, nh)[1]
        x_lo, x_hi = _taps(left, w, nw)[0], _taps(left + crop - 1, w, nw)[1]
        total += (r_hi - r_lo) * 3 * (x_hi - x_lo) + 3 * crop * crop * 2
    return total


def kernel_time(data_dir, n=256):
    pdf = pq.read_table(os.path.join(data_dir, "part-00000.parquet")
                        ).to_pandas().iloc[:n]
    b = decode_jpeg_canvas(pdf)
    canvas = torch.from_numpy(b["image"]).cuda()
    hw = torch.from_numpy(b["image_hw"])
    out = resize_crop_normalize(canvas, hw)
    # descriptor form of the launch, descriptors built once; the public call
    # below has image_hw on the device, as the loader delivers it, and the
    # kernel works out the geometry
    hc, wc = canvas.shape[1:3]
    desc_cpu = torch.from_numpy(_resize_crop_descriptors(
        hw.tolist(), [i * hc * wc * 3 for i in range(n)], [3 * wc] * n,
        canvas.numel(), 256, 224))
    desc = desc_cpu.cuda()
    scale, shift = _consts(canvas.device, IMAGENET_MEAN, IMAGENET_STD)
    flat = canvas.reshape(-1)

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        calls, ms = 0, 0.0
        while ms < 500.0:
            e0.record()
            for _ in range(100):
                fn()
            e1.record()
            e1.synchronize()
            ms += e0.elapsed_time(e1)
            calls += 100
        return 1e3 * ms / calls, ms

    us, ms = timed(lambda: _C.resize_crop_normalize(
        flat, desc, desc_cpu, out, scale, shift, 224))
    hw_dev = hw.cuda()
    api_us, _ = timed(lambda: resize_crop_normalize(canvas, hw_dev, out=out))
    assert torch.equal(out.view(torch.int16),
                       resize_crop_normalize(canvas, hw).view(torch.int16))
    torch.cuda.synchronize()
    fb = floor_bytes(b["image_hw"].tolist())
    return {"images": n, "kernel_us": round(us, 2),
            "window_ms": round(ms, 1), "public_call_us": round(api_us, 2),
            "floor_bytes": fb,
            "floor_us": round(1e6 * fb / FLOOR_BYTES_PER_S, 2),
            "bytes_per_s": round(fb / (us * 1e-6), 0)}


def loader_rows_per_s(data_dir, device_resize, workers, batch_size, rows):
    from mi355x_scale.train import ImageStreamDataModule
    dm = ImageStreamDataModule(data_dir, batch_size=batch_size,
                               workers_count=workers,
                               reader_pool_type="process",
                               image_format="jpeg",
                               device_resize=device_resize,
                               results_queue_size=20, prefetch_depth=3,
                               stagers=3)
    it = iter(dm.train_dataloader())

    def consume():
        b = next(it)
        if device_resize:
            resize_crop_normalize(b["image"], b["image_hw"])
        else:
            normalize_images(b["image"])
        return len(b["label"])

    consume()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = 0
    while got < rows:
        got += consume()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dm.teardown()
    return got / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--timed-rows", type=int, default=6000)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=212)
    ap.add_argument("--data-dir", type=str, default=None)
    ap.add_argument("--skip-loader", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU path"
    d = args.data_dir or os.path.join(tempfile.gettempdir(),
                                      f"jpegds_{args.rows}")
    if not os.path.exists(os.path.join(d, "part-00000.parquet")):
        write_jpeg_parquet(d, num_rows=args.rows, rows_per_group=64)
    out = {"metric": "resize_crop_normalize", "kernel": kernel_time(d)}
    print(f"# kernel: {out['kernel']}", file=sys.stderr, flush=True)
    if not args.skip_loader:
        runs = {"host_resize": [], "device_resize": []}
        for _ in range(3):
            for key, flag in (("host_resize", False), ("device_resize", True)):
                r = loader_rows_per_s(d, flag, args.workers, args.batch_size,
                                      args.timed_rows)
                runs[key].append(round(r, 1))
                print(f"# {key}: {r:,.0f} rows/s", file=sys.stderr,
                      flush=True)
        out["loader_rows_per_s"] = runs
        out["workers"] = args.workers
    print(json.dumps(out))


if __name__ == "__main__":
    main()
