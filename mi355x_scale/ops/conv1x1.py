"""MFMA pointwise (1x1, stride 1 and 2) convolution, NHWC bf16.

Two thirds of a Bottleneck network's convs are 1x1 (the reference trains
torchvision resnet50, ``deep_learning/
2.distributed-data-loading-petastorm.py:150``). In channels-last storage
a stride-1 1x1 conv is the plain GEMM ``Y[M, Cout] = X[M, Cin] . W^T``
(``M = N*H*W``) with both operands contiguous along the reduction axis.
``ops/csrc/conv1x1.hip`` computes it on ``v_mfma_f32_16x16x32_bf16``
(128 x 64 output tile per block, K-step 64, double-buffered swizzled LDS
tiles), and its statistics variant sums the BN batch statistics of the
bf16 values it stores into one partial slot per M-block:
``forward_with_stats`` hands them to ``FusedBNReLU2d.forward(...,
partial=...)``, which then skips ``bn_fwd_reduce`` and with it the second
read of the conv's output map. The data-grad ``dX = dY . W`` runs on the
same GEMM body; it reads the weight as it lies and transposes it on the
way out of LDS (``ds_read_b64_tr_b16``), so there is no scratch copy of
``W^T``.

The weight-grad ``dW = dY^T . X`` contracts over M, the strided index of
both maps, into a tiny output. ``conv1x1_wrw_kernel`` splits M into chunks
(about two blocks per CU), stages 32-row tiles as they lie, feeds both
MFMA operands with transposed LDS reads and writes one fp32 partial per
chunk; ``conv1x1_wrw_reduce_kernel`` sums them in a fixed order and
rounds once to bf16. It is a second opt-in, ``MI355X_CONV1X1_WRW=1``
(default ``0``, read on every call, effective only where
``MI355X_CONV1X1=1`` engages the HIP path); with it off the weight-grad is
MIOpen's. While a graph is being captured and ``weight.grad`` is a bf16
tensor of the weight's shape, dense like the weight (the FlatAdam views), the
reduce kernel ADDS into that view, bit for bit what ``AccumulateGrad``'s
bf16 add of a returned ``dw`` produces, and backward returns ``None`` for
the weight: the per-weight add launch is gone. Like the fused BN's
in-place channel grads this assumes the capture is of a ``.backward()``
into ``.grad``: tensor hooks on the weight do not see that gradient, and
``torch.autograd.grad(...)`` called INSIDE a capture with such a
``.grad`` present would get None for the weight and find ``.grad``
added to (keep the second switch off for that). Everywhere else
backward returns a fresh ``dw``.

STATUS (first reading, one benchmark run on MI355X at batch 212 —
benchmarks/bench_conv1x1.py, table in BASELINE.md): numerics are pinned
to fp64 references (tests/test_conv1x1.py). Forward + statistics beats
MIOpen + ``bn_fwd_reduce`` on eight of the twelve ResNet-50 shapes and
LOSES on four (512->128, 512->256, 1024->256, 1024->512, 6-23% slower);
the plain forward loses to MIOpen on ten of twelve; the data-grad is
ahead on ten and behind on 256->1024. The load phase is the bound at
Cin >= 512 (NOTES_NEXT.md lead 9). ResNet-50 step with the switch on:
9,231 vs 8,891 samples/s (two alternating runs each). Default-OFF:
``MI355X_CONV1X1=1``, read on every call, opts in; a per-shape default
needs three alternating runs per shape and re-baselines outputs.
Weight-grad: pinned to fp64 (tests/test_conv1x1_wrw.py); the twelve-shape
table against MIOpen + the grad add and the ResNet-50 step with the
second switch on are in BASELINE.md. At batch 212
(three runs) it is faster than MIOpen + the grad add on eight of the
twelve shapes and level on 64->256, 256->64, 256->128 and 512->256; the
ResNet-50 step goes 22.89 -> 22.80 ms with the second switch on (three
alternating runs each, slowest new above fastest old). The H = 56
shapes are HBM-bound (operands at 4.9-5.7 TB/s of 8); from H = 28 down
the bound is the tiles' re-reads through L2 and/or load latency
(BASELINE.md has the byte counts). Default-OFF as well.

Stride 2 (``Conv1x1(cin, cout, stride=2)``, the downsample projections
of every ResNet here): the same GEMMs over the ``M' = N*Ho*Wo`` rows of
the small map (``Ho = (H+1)//2``, ``Wo = (W+1)//2``) with the rows of the
large map gathered, ``(n, ho, wo) <-> (n, 2ho, 2wo)``; each is still Cin
contiguous values. The forward gathers its A rows (statistics epilogue
and partial layout unchanged, so ``forward_with_stats`` serves both
strides), the weight-grad gathers its X panel rows, and the data-grad
scatters: it writes the product row to the even pixel and zeros to the
other pixels of its 2x2 cell, so one launch writes all of ``dx`` and
there is no memset. The row map is two mul-hi divisions with host-computed
reciprocals. Same two switches, same gate. Measured at batch 212 on the
six downsample shapes (benchmarks/bench_conv1x1_s2.py, three alternating
rounds, table in BASELINE.md): every kernel is faster than MIOpen on the
three ResNet-18/34 shapes (fwd + stats 12-19 us against 23-28, dgrad 1.9x,
wrw + add 1.4-1.5x); on ResNet-50's the plain forward LOSES on 256->512@56
and 512->1024@28, fwd + stats is level on 256->512@56 and faster on the
other two, dgrad is faster on two and level on 512->1024@28, wrw faster on
two and level on 256->512@56. Steps with both switches on: ResNet-50
22.84 -> 22.63 ms (faster by the rule), ResNet-18 7.59 -> 7.53 ms by the
medians but LEVEL by the rule. Default-OFF like stride 1.

``Conv1x1`` subclasses ``nn.Conv2d`` (state-dict compatible, same init).
When enabled, the HIP path takes CUDA bf16 channels-last inputs and a
bf16 weight with Cin, Cout in {64, 128, ..., 2048}; everything else
falls through to ``F.conv2d``.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F


def _fwd(x: torch.Tensor, weight: torch.Tensor, stats: bool, stride: int):
    """Launch the forward GEMM. ``stats``: also fill the BN partial sums of
    the output (fp32 ``[2*Cout][nblocks]``, the layout ``bn_fwd_finalize``
    reads); otherwise ``partial`` is None."""
    from . import _C
    N, _, H, W = x.shape
    if stride == 2:
        H, W = (H + 1) // 2, (W + 1) // 2
    cout = weight.shape[0]
    out = torch.empty((N, cout, H, W), dtype=torch.bfloat16, device=x.device,
                      memory_format=torch.channels_last)
    partial = None
    if stats:
        partial = torch.empty(2 * cout * _C.conv1x1_fwd_blocks(N * H * W),
                              dtype=torch.float32, device=x.device)
    # the kernel addresses raw NHWC storage: hand the physical views over
    fwd = _C.conv1x1_s2_fwd if stride == 2 else _C.conv1x1_fwd
    fwd(x.permute(0, 2, 3, 1), weight, out.permute(0, 2, 3, 1), partial)
    return out, partial


def _bwd(ctx, dy: torch.Tensor):
    from . import _C
    x, weight = ctx.saved_tensors
    stride = ctx.stride
    if dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    dx = dw = None
    if ctx.needs_input_grad[0]:
        # the stride-2 kernel writes the skipped pixels' zeros itself
        dx = torch.empty_like(x)
        dgrad = _C.conv1x1_s2_dgrad if stride == 2 else _C.conv1x1_dgrad
        dgrad(dy.permute(0, 2, 3, 1), weight, dx.permute(0, 2, 3, 1))
    if ctx.needs_input_grad[1]:
        if os.environ.get("MI355X_CONV1X1_WRW", "0") == "1":
            dw = _wrw(x, dy, weight, stride)
        else:
            dw = torch.ops.aten.convolution_backward(
                dy, x, weight, None, [stride, stride], [0, 0], [1, 1], False,
                [0, 0], 1, [False, True, False])[1]
    return dx, dw, None


def _wrw(x: torch.Tensor, dy: torch.Tensor, weight: torch.Tensor,
         stride: int):
    """Weight-grad on the HIP kernels. Returns a fresh ``dw``, or None after
    adding it into ``weight.grad`` in place (under graph capture, when the
    grad is a dense bf16 tensor of the weight's shape; the weight is dense
    wherever the HIP path engages, so the two share one layout)."""
    from . import _C
    cin, cout = x.shape[1], weight.shape[0]
    rows = dy.shape[0] * dy.shape[2] * dy.shape[3]  # the reduction length
    wrw = _C.conv1x1_s2_wrw if stride == 2 else _C.conv1x1_wrw
    with torch.cuda.device(x.device):  # the chunk rule asks this device
        nch = _C.conv1x1_wrw_nchunks(rows, cin, cout)
    part = torch.empty(nch * cout * cin, dtype=torch.float32, device=x.device)
    xn, dyn = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    g = weight.grad
    if (torch.cuda.is_current_stream_capturing() and g is not None
            and g.dtype == torch.bfloat16 and g.device == weight.device
            and g.shape == weight.shape and g.is_contiguous()):
        wrw(xn, dyn, part, g, True)
        return None
    dw = torch.empty_like(weight)
    wrw(xn, dyn, part, dw)
    return dw


class _Conv1x1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int):
        out, _ = _fwd(x, weight, False, stride)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        return out

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        return _bwd(ctx, dy)


class _Conv1x1StatsFn(torch.autograd.Function):
    """Forward conv that also returns the BN partial sums of its output
    (non-differentiable); backward is ``_Conv1x1Fn``'s."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int):
        out, partial = _fwd(x, weight, True, stride)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        ctx.mark_non_differentiable(partial)
        # otherwise autograd hands backward a zero-filled tensor of
        # partial's size every step
        ctx.set_materialize_grads(False)
        return out, partial

    @staticmethod
    def backward(ctx, dy, _dpartial):
        if dy is None:
            return None, None, None
        return _bwd(ctx, dy)


class Conv1x1(nn.Conv2d):
    """1x1 conv, stride 1 or 2 (no bias), with the MFMA HIP fast path."""

    def __init__(self, cin: int, cout: int, stride: int = 1):
        if stride not in (1, 2):
            raise ValueError(f"Conv1x1: stride must be 1 or 2, got {stride!r}")
        super().__init__(cin, cout, 1, stride=stride, bias=False)

    def _hip_ok(self, x: torch.Tensor) -> bool:
        if os.environ.get("MI355X_CONV1X1", "0") != "1" or not x.is_cuda:
            return False
        from . import HAVE_EXT, require_ext
        cin, cout = self.in_channels, self.out_channels
        ok = (x.dim() == 4 and x.shape[1] == cin
              and cin % 64 == 0 and cin <= 2048
              and cout % 64 == 0 and cout <= 2048
              and x.dtype == torch.bfloat16
              and self.weight.dtype == torch.bfloat16
              and x.is_contiguous(memory_format=torch.channels_last)
              and self.weight.is_contiguous())
        if ok and not HAVE_EXT:
            require_ext()  # asked for, and missing: no silent fallback
        return ok

    def stats_ok(self, x: torch.Tensor) -> bool:
        """True when ``forward_with_stats`` will run the fused kernel."""
        return self._hip_ok(x)

    def forward_with_stats(self, x: torch.Tensor):
        """``(conv(x), partial)``: ``partial`` holds the per-block BN sums
        of the output for ``FusedBNReLU2d.forward(..., partial=...)``, or
        is None when the HIP path does not engage."""
        if self.stats_ok(x):
            return _Conv1x1StatsFn.apply(x, self.weight, self.stride[0])
        return self.forward(x), None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._hip_ok(x):
            return _Conv1x1Fn.apply(x, self.weight, self.stride[0])
        return F.conv2d(x, self.weight, None, self.stride[0], 0)
