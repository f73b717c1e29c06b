"""MFMA stem convolution (7x7 stride-2 pad-3, 3->64, NHWC bf16).

The ResNet stem is the one conv MIOpen leaves on a generic igemm tile
(Cin=3 starves the GEMM K: K = 7*7*3 = 147) — MIOpen measured ~298 us
forward + ~294 us weight-grad per step at bs 212 on the flagship bench,
~7% of the whole step. ``ops/csrc/stemconv.hip`` computes it as the
GEMM it is on ``v_mfma_f32_16x16x32_bf16`` with a pixel-padded LDS
input band per output row: forward 210 us (1.73x MIOpen, padded
weights read from L1-resident global), weight-grad 133 us per step
(2.1x MIOpen in ``benchmarks/bench_stemconv.py``; ring-band staging,
the next row's dy slice and band rows prefetched into registers under
the MFMA phase, and both MFMA operands read from LDS with the
transposing ``ds_read_b64_tr_b16``). ``MI355X_STEM_WRW_TR=0``, read by
the extension on every call, selects the earlier weight-grad kernel
that gathers its operands element by element (260 us; A/B runs, tests).

The default forward kernel (``MI355X_STEM_FUSED_STATS``, ``0`` = the
one-row-per-block kernel above) gives a block eight output rows: the
input band is staged once, the weights stay in registers across the
rows, the output leaves as 16-byte stores, and the epilogue sums the
BN batch statistics of the values it stores into one partial slot per
block (``forward_with_stats`` hands them to
``FusedBNReLU2d.forward_pooled``, which then skips its reduce pass).
The bf16 output is bit-identical to the one-row kernel's.

``StemConv2d`` subclasses ``nn.Conv2d`` (state-dict compatible, same
init); the HIP path engages on CUDA bf16 channels-last inputs with the
exact stem geometry, everything else falls back to ``F.conv2d`` (the
CPU numerics baseline). The stem input needs no data-grad (it is the
normalized image batch), so backward produces only the weight grad.
Replaces the reference's torchvision conv1 (``deep_learning/
2.distributed-data-loading-petastorm.py:150``'s resnet50 stem).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F


def fused_stats_enabled() -> bool:
    """``MI355X_STEM_FUSED_STATS=0`` selects the one-row-per-block forward
    kernel and the separate BN reduce over its output (A/B runs, tests)."""
    return os.environ.get("MI355X_STEM_FUSED_STATS", "1") != "0"


def _stem_forward(x: torch.Tensor, weight: torch.Tensor, fused: bool):
    """Launch the forward conv. ``fused``: the multi-row kernel, which also
    fills the BN partial sums of its output (fp32 ``[2*64][nblocks]``, the
    layout ``bn_fwd_finalize`` reads); otherwise ``partial`` is None."""
    from . import _C
    N, C, H, W = x.shape
    HO = (H + 2 * 3 - 7) // 2 + 1
    WO = (W + 2 * 3 - 7) // 2 + 1
    out = torch.empty((N, 64, HO, WO), dtype=torch.bfloat16,
                      device=x.device,
                      memory_format=torch.channels_last)
    # kernels address raw NHWC storage: hand the physical views over
    wp = torch.empty(64 * 160, dtype=torch.bfloat16, device=x.device)
    partial = None
    if fused:
        partial = torch.empty(2 * 64 * _C.stem_fwd_blocks(N, HO),
                              dtype=torch.float32, device=x.device)
    _C.stem_conv_fwd(x.permute(0, 2, 3, 1), weight.permute(0, 2, 3, 1),
                     out.permute(0, 2, 3, 1), wp, 7, partial)
    return out, partial


def _stem_backward(ctx, dy: torch.Tensor):
    from . import _C
    x, weight = ctx.saved_tensors
    if dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    dw = torch.empty_like(weight)
    # which wrw kernel runs is the extension's choice per call
    # (MI355X_STEM_WRW_TR, "0" = the element-gather kernel)
    scratch = torch.empty(_C.stem_wrw_scratch(), dtype=torch.float32,
                          device=x.device)
    _C.stem_conv_wrw(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1),
                     scratch, dw.permute(0, 2, 3, 1))
    return None, dw


class _StemConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor):
        out, _ = _stem_forward(x, weight, fused_stats_enabled())
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        return _stem_backward(ctx, dy)


class _StemConvStatsFn(torch.autograd.Function):
    """Forward conv that also returns the BN partial sums of its output
    (non-differentiable); backward is ``_StemConvFn``'s."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor):
        out, partial = _stem_forward(x, weight, True)
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(partial)
        # otherwise autograd hands backward a zero-filled tensor of
        # partial's size every step (a 1.5 MB fill kernel at bs 212)
        ctx.set_materialize_grads(False)
        return out, partial

    @staticmethod
    def backward(ctx, dy, _dpartial):
        if dy is None:
            return None, None
        return _stem_backward(ctx, dy)


class StemConv2d(nn.Conv2d):
    """7x7/s2/p3 3->64 conv with the MFMA HIP fast path."""

    def __init__(self):
        super().__init__(3, 64, 7, stride=2, padding=3, bias=False)

    def _hip_ok(self, x: torch.Tensor) -> bool:
        from . import HAVE_EXT
        return (HAVE_EXT and x.is_cuda
                and os.environ.get("MI355X_STEM_CONV", "1") == "1"
                # the kernels' cap is 128 OUTPUT pixels per row
                and (x.shape[-1] - 1) // 2 + 1 <= 128
                and x.dtype == torch.bfloat16
                and self.weight.dtype == torch.bfloat16
                and x.is_contiguous(memory_format=torch.channels_last)
                and self.weight.is_contiguous(
                    memory_format=torch.channels_last)
                and not x.requires_grad)  # stem input never needs dx

    def stats_ok(self, x: torch.Tensor) -> bool:
        """True when ``forward_with_stats`` will run the fused kernel."""
        return fused_stats_enabled() and self._hip_ok(x)

    def forward_with_stats(self, x: torch.Tensor):
        """``(conv(x), partial)``: ``partial`` holds the per-block BN sums
        of the output for ``FusedBNReLU2d.forward_pooled``, or is None
        when the HIP path does not engage or the switch is off."""
        if self.stats_ok(x):
            return _StemConvStatsFn.apply(x, self.weight)
        return self.forward(x), None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._hip_ok(x):
            return _StemConvFn.apply(x, self.weight)
        if x.is_cuda and torch.cuda.is_available():
            from . import HAVE_EXT, require_ext
            if HAVE_EXT is False and x.dtype == torch.bfloat16:
                require_ext()  # no silent eager fallback on a GPU box
        return F.conv2d(x, self.weight, None, self.stride, self.padding)
