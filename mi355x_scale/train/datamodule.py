"""ImageStreamDataModule — the ImageNetDataModule equivalent.

Mirrors the reference's Petastorm datamodule
(``deep_learning/2.distributed-data-loading-petastorm.py:224-318``) with
the same knob names (``workers_count``, ``reader_pool_type``,
``results_queue_size``, ``cur_shard``, ``shard_count``) over the native
streaming stack: pyarrow row-group decode threads → bounded queue →
fixed-size batches → pinned ring → side-stream H2D.

The per-row JPEG/resize/crop CPU transform of the reference is replaced
by storing images at training shape and doing normalize+dtype on device
(the fused HIP kernel) — the decode pool only reshapes bytes.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..data import (BatchReader, DataLoader, DatasetManifest, DeviceLoader,
                    TransformSpec)  # noqa: F401 (re-export)
from .module import DataModule


def _bytes_to_nhwc(h: int, w: int):
    def _f(pdf):
        imgs = np.stack([
            np.frombuffer(b, dtype=np.uint8).reshape(h, w, 3)
            for b in pdf["image"]
        ])
        return {"image": imgs, "label": pdf["label"].to_numpy()}
    return _f


def _arrow_images(h: int, w: int):
    """Zero-copy arrow decode: the fixed_size_binary image column's data
    buffer is viewed directly as uint8 [n,h,w,3] — no per-row python loop,
    no np.stack memcpy. This is where the streaming path's host-side
    headroom comes from (vs Petastorm's pandas round trip)."""
    rb = h * w * 3

    def _f(table):
        col = table.column("image")
        chunks = col.chunks if hasattr(col, "chunks") else [col]
        views = []
        for ch in chunks:
            buf = ch.buffers()[1]
            a = np.frombuffer(buf, dtype=np.uint8)
            a = a[ch.offset * rb:(ch.offset + len(ch)) * rb]
            views.append(a.reshape(len(ch), h, w, 3))
        imgs = views[0] if len(views) == 1 else np.concatenate(views)
        labels = table.column("label").to_numpy()
        return {"image": imgs, "label": labels}
    return _f


class ImageStreamDataModule(DataModule):
    def __init__(
        self,
        data_dir: str,
        batch_size: int = 212,            # reference BATCH_SIZE (deep_learning/2...py:342)
        workers_count: int = 2,           # reference :346
        reader_pool_type: str = "thread",  # reference :347
        results_queue_size: int = 20,     # reference :348
        cur_shard: Optional[int] = None,
        shard_count: Optional[int] = None,
        image_hw=(224, 224),
        device: Optional[torch.device] = None,
        prefetch_depth: int = 2,
        stagers: int = 2,
        val_fraction_shards: bool = True,
        image_format: str = "raw",
        device_resize: bool = False,
        canvas_hw=(512, 512),
    ):
        if image_format not in ("raw", "jpeg"):
            raise ValueError("image_format must be 'raw' or 'jpeg'")
        if device_resize and image_format != "jpeg":
            raise ValueError("device_resize goes with image_format='jpeg'")
        self.image_format = image_format
        self.device_resize = device_resize
        self.canvas_hw = tuple(canvas_hw)
        self.data_dir = data_dir
        self.batch_size = batch_size
        self.workers_count = workers_count
        self.reader_pool_type = reader_pool_type
        self.results_queue_size = results_queue_size
        self.cur_shard = cur_shard
        self.shard_count = shard_count
        self.image_hw = tuple(image_hw)
        self.device = device if device is not None else (
            torch.device("cuda", torch.cuda.current_device())
            if torch.cuda.is_available() else torch.device("cpu"))
        self.prefetch_depth = prefetch_depth
        self.stagers = stagers
        self._manifest: Optional[DatasetManifest] = None
        self._open_loaders = []

    def setup(self, stage: Optional[str] = None) -> None:
        if self._manifest is None:
            self._manifest = DatasetManifest.discover(self.data_dir)

    @property
    def num_rows(self) -> int:
        self.setup()
        return self._manifest.num_rows

    def _make_loader(self, num_epochs: Optional[int]):
        self.setup()
        h, w = self.image_hw
        if self.image_format == "jpeg" and self.device_resize:
            # decode only: images land on a fixed canvas with their size
            # alongside, and resize + crop + normalize run on the device
            # (ops.resize_crop_normalize, picked by ImageClassifier._unpack
            # when the batch carries image_hw)
            from functools import partial

            from ..data.generator import decode_jpeg_canvas
            hc, wc = self.canvas_hw
            kwargs = dict(transform_spec=TransformSpec(
                partial(decode_jpeg_canvas, canvas_hw=(hc, wc)),
                edit_fields=[("image", np.uint8, (hc, wc, 3), False),
                             ("image_hw", np.int32, (2,), False),
                             ("label", np.int64, (), False)],
                selected_fields=["image", "image_hw", "label"]))
        elif self.image_format == "jpeg":
            # encoded-JPEG datasets: the reference's real per-row CPU
            # transform (decode + resize + crop) runs in the reader pool
            # (deep_learning/2...py:282-296); normalize stays on device
            from functools import partial

            from ..data.generator import decode_jpeg_batch
            kwargs = dict(transform_spec=TransformSpec(
                partial(decode_jpeg_batch, image_hw=(h, w)),
                edit_fields=[("image", np.uint8, (h, w, 3), False),
                             ("label", np.int64, (), False)],
                selected_fields=["image", "label"]))
        else:
            kwargs = dict(arrow_transform=_arrow_images(h, w))
        reader = BatchReader(
            self._manifest,
            cur_shard=self.cur_shard,
            shard_count=self.shard_count,
            workers_count=self.workers_count,
            reader_pool_type=self.reader_pool_type,
            results_queue_size=self.results_queue_size,
            num_epochs=num_epochs,
            **kwargs,
        )
        loader = DeviceLoader(DataLoader(reader, self.batch_size),
                              self.device, depth=self.prefetch_depth,
                              stagers=self.stagers)
        self._open_loaders.append(loader)
        return loader

    def train_dataloader(self):
        # Infinite reader (num_epochs=None): epoch length is imposed by the
        # Trainer's limit_train_batches — the reference's exact contract
        # (deep_learning/2...py:218-220,254).
        return self._make_loader(num_epochs=None)

    def val_dataloader(self):
        return self._make_loader(num_epochs=1)

    def teardown(self, stage: Optional[str] = None) -> None:
        for ld in self._open_loaders:
            ld.close()
        self._open_loaders = []
