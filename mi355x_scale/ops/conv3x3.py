"""3x3/s1/p1 conv: MFMA forward (with BN statistics), data-grad, weight-grad.

Three independent legs, each opt-in and default-off; with every switch
unset the conv is ``F.conv2d`` (MIOpen) in both directions.

Forward, ``MI355X_CONV3X3=1`` (``ops/csrc/conv3x3.hip``): an implicit GEMM
in padded-flat coordinates. The input is seen as a zero-bordered map
``[N][H+2][W+2]``; a block owns 128 consecutive virtual pixels and 64
output channels, stages ONE band of ``128 + 2W + 6`` pixel rows per
64-channel chunk of Cin into LDS and feeds all nine taps from it (a tap is
one constant row offset). Border outputs are computed and thrown away
(useful MFMA share ``H*W / ((H+2)*(W+2))``). Its statistics variant sums
the BN batch statistics of the bf16 values it stores into one partial slot
per block: ``forward_with_stats`` hands them to
``FusedBNReLU2d.forward(..., partial=...)``, which then skips
``bn_fwd_reduce`` and the second read of the map.

Data-grad, ``MI355X_CONV3X3_DGRAD=1`` (only where ``MI355X_CONV3X3=1``
engaged the forward): ``dX`` is the same convolution applied to ``dY`` with
the weight rotated and transposed. ``conv3x3_wflip_kernel`` repacks the
weight (at most 4.7 MB) into a scratch tensor and the forward kernel runs
on it; there is no second GEMM body.

Weight-grad, ``MI355X_CONV_WRW=1`` (``ops/csrc/conv3x3wrw.hip``, Cin ==
Cout, 9 <= W <= 64): MIOpen's weakest leg on these shapes, plus its
fp32-workspace zero + bf16-cast launches and the AccumulateGrad add into
the flat grad view. Inside hipGraph capture the cast kernel writes the
weight's flat grad view DIRECTLY (the fused-BN fuse_acc pattern), so the
add disappears from the captured step.

STATUS, weight-grad (round 2, measured on MI355X —
benchmarks/bench_conv3x3_wrw.py):
numerics verified against the fp32 reference on every block-conv shape,
but two blocking iterations both lost to MIOpen igemm wrw (v1 32x32
tiles: 0.56x at C=64; v2 64x64 tiles / 8-wave blocks / non-atomic chunk
partials: 0.35x at C=64 down to 0.10x at C=512). Ablations localize the
cost to the thin per-row phase structure: one staging latency + three
barriers per 56-px output row, at 1 block/CU (211 VGPRs -> 2
waves/SIMD), cannot fill the machine, and the K-padding waste at
W<=14 is fatal for layer3/4. Default-OFF (``MI355X_CONV_WRW=1`` opts
in); the round-3 path is software-pipelined multi-row K-phases (stage
row r+1 into registers during row r's MFMAs) plus a VGPR diet — see
NOTES_NEXT.md.

STATUS, forward and data-grad (one benchmark run on MI355X at batch 212,
three alternating rounds — benchmarks/bench_conv3x3_fwd.py, table in
BASELINE.md): numerics are pinned to fp64 references
(tests/test_conv3x3_fwd.py). By the project's rule (our slowest round
against MIOpen's fastest), medians in us:
forward + statistics against MIOpen + ``bn_fwd_reduce`` is FASTER on
64@56 (84 against 115), 128@28 (73 against 83) and 512@7 (88 against 100)
and LEVEL on 256@14 (72 against 76 by the medians; slowest 74.6 against
fastest 73.9). The plain forward is faster on 64@56 (73 against 100) and
128@28 (63 against 72), and LEVEL on 256@14 (68 against 65: behind by the
medians) and on 512@7 (88 against 92). The data-grad, repack included, is
faster on all four (73 / 66 / 69 / 91 against 125 / 99 / 95 / 113).
ResNet-18 step with both switches on: 6.98 / 6.94 / 7.00 ms against 7.62 /
7.60 / 7.56 with them off (three alternating ``bench.py`` runs each):
faster by the rule. Staging alone is 57-82 % of the call and MFMA alone
50-69 %: the two do not overlap well yet (NOTES_NEXT.md lead 10). Both
switches are default-OFF in this state: they are read on every call, and
turning them on re-baselines the model's outputs.

``Conv3x3`` subclasses ``nn.Conv2d`` (state-dict compatible, same
init). The forward / data-grad path takes CUDA bf16 channels-last inputs
and a bf16 channels-last weight with Cin, Cout in {64, 128, ..., 2048} and
1 <= W <= 64; everything else falls back to the standard conv autograd.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

_S1 = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)  # stride, pad, dilation, ...


def _switch(name: str) -> bool:
    return os.environ.get(name, "0") == "1"


def _fwd_gate(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """True when ``MI355X_CONV3X3=1`` and conv3x3.hip takes this call."""
    if not _switch("MI355X_CONV3X3") or not x.is_cuda:
        return False
    from . import HAVE_EXT, require_ext
    ok = x.dim() == 4 and weight.dim() == 4
    if ok:
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        ok = (tuple(weight.shape[1:]) == (cin, 3, 3)
              and cin % 64 == 0 and 64 <= cin <= 2048
              and cout % 64 == 0 and 64 <= cout <= 2048
              and n >= 1 and h >= 1 and 1 <= w <= 64
              and n * (h + 2) * (w + 2) + 2 * w + 6 < 2 ** 31
              and x.dtype == torch.bfloat16
              and weight.dtype == torch.bfloat16
              and x.is_contiguous(memory_format=torch.channels_last)
              and weight.is_contiguous(memory_format=torch.channels_last))
    if ok and not HAVE_EXT:
        require_ext()  # asked for, and missing: no silent fallback
    return ok


def _fwd(x: torch.Tensor, weight: torch.Tensor, stats: bool):
    """Launch the forward kernel. ``stats``: also fill the BN partial sums
    of the output (fp32 ``[2*Cout][nblocks]``, the layout ``bn_fwd_finalize``
    reads); otherwise ``partial`` is None."""
    from . import _C
    n, _, h, w = x.shape
    cout = weight.shape[0]
    out = torch.empty((n, cout, h, w), dtype=torch.bfloat16, device=x.device,
                      memory_format=torch.channels_last)
    partial = None
    if stats:
        partial = torch.empty(2 * cout * _C.conv3x3_fwd_blocks(n, h, w),
                              dtype=torch.float32, device=x.device)
    # the kernel addresses raw NHWC storage: hand the physical views over
    _C.conv3x3_fwd(x.permute(0, 2, 3, 1), weight.permute(0, 2, 3, 1),
                   out.permute(0, 2, 3, 1), partial)
    return out, partial


def _forward(ctx, x, weight, hip_fwd: bool, stats: bool, hip_wrw: bool):
    if hip_fwd:
        out, partial = _fwd(x, weight, stats)
    else:
        out, partial = torch.ops.aten.convolution(x, weight, None, *_S1), None
    ctx.save_for_backward(x, weight)
    ctx.hip_fwd, ctx.hip_wrw = hip_fwd, hip_wrw
    return out, partial


def _backward(ctx, dy: torch.Tensor):
    """``(dx, dw)``: each leg on its HIP kernel or on aten, independently."""
    from . import _C
    x, weight = ctx.saved_tensors
    if ctx.hip_fwd and dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    hip_dgrad = ctx.hip_fwd and _switch("MI355X_CONV3X3_DGRAD")
    need_dx, need_dw = ctx.needs_input_grad[:2]
    # whatever stays on aten goes in one call
    mask = [need_dx and not hip_dgrad, need_dw and not ctx.hip_wrw, False]
    dx = dw = None
    if mask[0] or mask[1]:
        dx, dw, _ = torch.ops.aten.convolution_backward(
            dy, x, weight, None, *_S1, mask)
    if need_dx and hip_dgrad:
        dx = torch.empty_like(x)
        wflip = torch.empty(weight.numel(), dtype=torch.bfloat16,
                            device=weight.device)
        _C.conv3x3_dgrad(dy.permute(0, 2, 3, 1), weight.permute(0, 2, 3, 1),
                         wflip, dx.permute(0, 2, 3, 1))
    if ctx.hip_wrw:
        C = weight.shape[0]
        nch = _C.conv3x3_wrw_nchunks(x.shape[0], x.shape[2], C, 0)
        scratch = torch.empty(nch * C * 9 * C, dtype=torch.float32,
                              device=x.device)
        g = weight.grad
        fuse = (torch.cuda.is_current_stream_capturing()
                and g is not None and g.dtype == torch.bfloat16
                and g.is_contiguous(memory_format=torch.channels_last))
        dw = g if fuse else torch.empty_like(weight)
        _C.conv3x3_wrw(x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1),
                       scratch, dw.permute(0, 2, 3, 1))
        # fuse: the cast kernel wrote the flat grad view; returning None
        # skips autograd's AccumulateGrad add for this weight
        if fuse:
            dw = None
    return dx, dw


class _Conv3x3Fn(torch.autograd.Function):
    """The node of ``MI355X_CONV_WRW=1``: weight-grad on conv3x3wrw.hip;
    forward and data-grad on conv3x3.hip where their switches engage."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor):
        return _forward(ctx, x, weight, _fwd_gate(x, weight), False, True)[0]

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        return _backward(ctx, dy)


class _Conv3x3HipFn(torch.autograd.Function):
    """Forward on conv3x3.hip, returning ``(out, partial)``: the BN partial
    sums of the output (non-differentiable) when ``stats``, else None.
    ``hip_wrw`` picks the weight-grad leg."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stats: bool,
                hip_wrw: bool):
        out, partial = _forward(ctx, x, weight, True, stats, hip_wrw)
        if partial is not None:
            ctx.mark_non_differentiable(partial)
        # otherwise autograd hands backward a zero-filled tensor of
        # partial's size every step
        ctx.set_materialize_grads(False)
        return out, partial

    @staticmethod
    def backward(ctx, dy, _dpartial):
        if dy is None:
            return None, None, None, None
        return (*_backward(ctx, dy), None, None)


class Conv3x3(nn.Conv2d):
    """3x3/s1/p1 conv (no bias) with the opt-in MFMA HIP paths."""

    def __init__(self, cin: int, cout: int):
        super().__init__(cin, cout, 3, stride=1, padding=1, bias=False)

    def _hip_ok(self, x: torch.Tensor) -> bool:
        """The weight-grad kernel's gate (``MI355X_CONV_WRW=1``)."""
        from . import HAVE_EXT
        C = self.out_channels
        return (HAVE_EXT and x.is_cuda
                and _switch("MI355X_CONV_WRW")
                and self.in_channels == C
                and C % 64 == 0 and C <= 2048
                and 9 <= x.shape[-1] <= 64
                and x.dtype == torch.bfloat16
                and self.weight.dtype == torch.bfloat16
                and x.is_contiguous(memory_format=torch.channels_last)
                and self.weight.is_contiguous(
                    memory_format=torch.channels_last))

    def stats_ok(self, x: torch.Tensor) -> bool:
        """True when ``forward_with_stats`` will run the fused kernel."""
        return _fwd_gate(x, self.weight)

    def forward_with_stats(self, x: torch.Tensor):
        """``(conv(x), partial)``: ``partial`` holds the per-block BN sums
        of the output for ``FusedBNReLU2d.forward(..., partial=...)``, or
        is None when the HIP forward does not engage."""
        if self.stats_ok(x):
            return _Conv3x3HipFn.apply(x, self.weight, True, self._hip_ok(x))
        return self.forward(x), None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.stats_ok(x):
            return _Conv3x3HipFn.apply(x, self.weight, False,
                                       self._hip_ok(x))[0]
        if self._hip_ok(x):
            return _Conv3x3Fn.apply(x, self.weight)
        return F.conv2d(x, self.weight, None, 1, 1)
