"""3x3/s1/p1 conv: MFMA forward (with BN statistics), data-grad, weight-grad.

Three legs, each behind a tri-state switch read on every call: ``1``
engages the leg wherever its gate allows, ``0`` never, and UNSET asks a
small per-shape table in this file (``_FWD_TABLE``, ``_WRW_TABLE``), keyed
on (C, H, W) with a batch floor, which holds only what was measured faster
than MIOpen by the project's win rule. Everything the table does not name
(every small-batch call among them) is ``F.conv2d`` (MIOpen) in both
directions.

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

Weight-grad, ``MI355X_CONV_WRW`` (``ops/csrc/conv3x3wrw.hip``, Cin == Cout,
1 <= W <= 64): a split-K MFMA kernel in the same padded-flat coordinates.
A block owns a 64 x 64 tile of dW for all nine taps and one chunk of
32-pixel K-steps, stages dY panels and an LDS ring of X rows as they lie
in memory, feeds both operands with transposed LDS reads and writes one
fp32 partial per chunk; ``conv1x1_wrw_reduce_kernel`` sums the partials in
a fixed order and rounds once to bf16. It replaces MIOpen's igemm wrw, its
two fp32-workspace zero fills and its bf16 cast. While a graph is being
captured and ``weight.grad`` is a bf16 channels-last tensor of the weight's
shape (the FlatAdam views), the reduce ADDS into that view, bit for bit
what ``AccumulateGrad``'s bf16 add of a returned ``dw`` produces, and
backward returns ``None`` for the weight (the conv1x1 contract,
ops/conv1x1.py, with the same caveats). Everywhere else backward returns a
fresh ``dw``.

STATUS, weight-grad (one benchmark run on MI355X at batch 212, three
alternating rounds, benchmarks/bench_conv3x3_wrw.py, tables in
BASELINE.md): numerics are pinned to fp64 within one bf16 rounding
(tests/test_conv3x3_wrw_flat.py). Kernel + reduce in accumulate mode
against MIOpen wrw + the grad add, medians in us: 85 against 143 on 64@56,
87 against 108 on 128@28, 93 against 105 on 256@14, 109 against 117 on
512@7: FASTER on all four by the rule (slowest of ours 93.6 / 96.2 / 100.5
/ 112.7 under MIOpen's fastest 139.4 / 107.6 / 104.6 / 116.5), so all four
are in ``_WRW_TABLE`` at batch floor 212. Loads alone are 54-67 us, fragment
reads + MFMA alone 55-72 us, epilogue + reduce 35 us (150 MB of fp32
partials written and read back, the same for every shape).

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
50-69 %: the two do not overlap well yet (NOTES_NEXT.md lead 10). Judged
as a pair (``fwd + stats`` plus ``dgrad`` against MIOpen's ``fwd + reduce``
plus ``dgrad``) all four shapes are faster by the rule, 256@14 included,
and all four are in ``_FWD_TABLE`` at batch floor 212; the data-grad
engages only where the forward did. The defaults re-baseline the model's
outputs at batch >= 212 (profiles/r09_conv3x3_wrw_kernstats.md has the
comparison against the parent's run-to-run spread).

Stride 2 (``Conv3x3(cin, cout, stride=2)``, ``ops/csrc/conv3x3s2.hip``),
behind switches of its own, ``MI355X_CONV3X3_S2`` (forward and statistics)
and ``MI355X_CONV3X3_S2_DGRAD`` (only where the forward engaged), with
``_S2_TABLE`` keyed (Cin, Cout, H, W); the three stride-1 switches never
touch a stride-2 module. At stride 2 a tap is no constant offset in input
coordinates, so the kernels work on the OUTPUT grid, seen as a virtual map
``[N][Ho+1][Wo+1]`` with one leading zero row and column: the input splits
into four parity planes ``X[2i+ph][2j+pw]``, and on that grid every tap is
a constant offset into exactly one plane. The forward stages one plane
band (``128 + Wo + 2`` rows) at a time into two alternating LDS buffers and
runs that plane's 4, 2, 2 or 1 taps from it; the data-grad computes each
parity plane of ``dX`` as a 4-, 2-, 2- or 1-tap convolution of one ``dY``
band against the repacked weight and writes every ``dX`` pixel exactly
once. Cin and Cout may differ, 1 <= W <= 128. The weight-grad of these
convs stays on aten/MIOpen.

STATUS, stride 2 (one benchmark run on MI355X at batch 212, three
alternating rounds, benchmarks/bench_conv3x3_s2.py, table in BASELINE.md):
numerics are pinned to fp64 references (tests/test_conv3x3_s2.py). Medians
in us on 64->128@56 / 128->256@28 / 256->512@14 / 128->128@56 /
256->256@28 / 512->512@14: forward + statistics 73 / 61 / 63 / 113 / 96 /
111 against MIOpen + ``bn_fwd_reduce`` 60 / 53 / 62 / 92 / 78 / 101:
SLOWER on all six, as is the plain forward (68 / 57 / 61 / 109 / 93 / 110
against 46 / 40 / 52 / 81 / 70 / 93). The data-grad, repack included, is 87
/ 60 / 59 / 165 / 106 / 105 against 89 / 63 / 62 / 133 / 114 / 111: LEVEL
by the rule on five shapes, slower on 128->128@56. No pair wins, so
``_S2_TABLE`` is empty and an unset switch means ``F.conv2d``, bit for bit
what the module computed before. Loads + staging alone are 80-93 % of the
forward call (NOTES_NEXT.md lead 1(d)).

``Conv3x3`` subclasses ``nn.Conv2d`` (state-dict compatible, same
init). The forward / data-grad path takes CUDA bf16 channels-last inputs
and a bf16 channels-last weight with Cin, Cout in {64, 128, ..., 2048} and
1 <= W <= 64 (128 at stride 2); everything else falls back to the standard
conv autograd.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

_S1 = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)  # stride, pad, dilation, ...
_S2 = ([2, 2], [1, 1], [1, 1], False, [0, 0], 1)


# Per-shape defaults, (C, H, W) -> batch floor: what an UNSET switch engages.
# A line is here only where the leg was measured faster at that batch by the
# project's win rule (our slowest round under MIOpen's fastest); the floor
# is the smallest batch measured. Forward and data-grad are judged as a
# pair, ``fwd + stats`` plus ``dgrad`` against MIOpen's ``fwd + reduce``
# plus ``dgrad``: BASELINE.md, "3x3 stride-1 conv MFMA kernels", slowest of
# ours against MIOpen's fastest, us.
_FWD_TABLE = {
    (64, 56, 56): 212,   # 89.7 + 78.4 against 115.0 + 124.3
    (128, 28, 28): 212,  # 76.2 + 67.4 against 83.0 + 97.5
    (256, 14, 14): 212,  # 74.6 + 75.5 against 73.9 + 93.1 (fwd alone level)
    (512, 7, 7): 212,    # 91.4 + 94.4 against 98.2 + 112.5
}
# Weight-grad + reduce in accumulate mode against MIOpen wrw + the grad add:
# BASELINE.md, "3x3 stride-1 weight-grad".
_WRW_TABLE = {
    (64, 56, 56): 212,   # 93.6 against 139.4
    (128, 28, 28): 212,  # 96.2 against 107.6
    (256, 14, 14): 212,  # 100.5 against 104.6
    (512, 7, 7): 212,    # 112.7 against 116.5
}


# Stride 2, (Cin, Cout, H, W) -> batch floor, judged as a pair in the same
# way: BASELINE.md, "3x3 stride-2 conv MFMA kernels".
_S2_TABLE = {}


def _engaged(name: str, table: dict, c, n: int, h: int, w: int) -> bool:
    """The tri-state rule of the switches: ``1`` engages wherever the gate
    allows, ``0`` never, unset asks ``table``. ``c`` is the channel part of
    the table's key: one number, or ``(Cin, Cout)`` for ``_S2_TABLE``."""
    v = os.environ.get(name)
    if v is not None:
        return v == "1"
    floor = table.get((*c, h, w) if isinstance(c, tuple) else (c, h, w))
    return floor is not None and n >= floor


def _fwd_gate(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """True when conv3x3.hip takes this call: ``MI355X_CONV3X3`` (or, unset,
    the table) engages and the shape is inside the kernel's gate."""
    if not x.is_cuda or x.dim() != 4 or weight.dim() != 4:
        return False
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    # the table knows Cin == Cout shapes only
    if not _engaged("MI355X_CONV3X3", _FWD_TABLE,
                    cin if cin == cout else None, n, h, w):
        return False
    from . import HAVE_EXT, require_ext
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
    if (ctx.hip_fwd or ctx.hip_wrw) and dy.dtype != torch.bfloat16:
        dy = dy.to(torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    n, c, h, w = x.shape
    hip_dgrad = ctx.hip_fwd and _engaged("MI355X_CONV3X3_DGRAD", _FWD_TABLE,
                                         c, n, h, w)
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
    if need_dw and ctx.hip_wrw:
        dw = _wrw(x, dy, weight)
    return dx, dw


def _wrw(x: torch.Tensor, dy: torch.Tensor, weight: torch.Tensor):
    """Weight-grad on conv3x3wrw.hip. Returns a fresh ``dw``, or None after
    adding it into ``weight.grad`` in place (under graph capture, when the
    grad is a bf16 channels-last tensor of the weight's shape: the conv1x1
    contract, ops/conv1x1.py)."""
    from . import _C
    n, c, h, w = x.shape
    with torch.cuda.device(x.device):  # the chunk rule asks this device
        nch = _C.conv3x3_wrw_nchunks(n, h, w, c)
    part = torch.empty(nch * 9 * c * c, dtype=torch.float32, device=x.device)
    xn, dyn = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    g = weight.grad
    if (torch.cuda.is_current_stream_capturing() and g is not None
            and g.dtype == torch.bfloat16 and g.device == weight.device
            and g.shape == weight.shape
            and g.is_contiguous(memory_format=torch.channels_last)):
        _C.conv3x3_wrw(xn, dyn, part, g.permute(0, 2, 3, 1), True)
        return None
    dw = torch.empty_like(weight)
    _C.conv3x3_wrw(xn, dyn, part, dw.permute(0, 2, 3, 1))
    return dw


def _s2_gate(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """True when conv3x3s2.hip takes this stride-2 call: ``MI355X_CONV3X3_S2``
    (or, unset, ``_S2_TABLE``) engages and the shape is inside the gate."""
    if not x.is_cuda or x.dim() != 4 or weight.dim() != 4:
        return False
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    if not _engaged("MI355X_CONV3X3_S2", _S2_TABLE, (cin, cout), n, h, w):
        return False
    from . import HAVE_EXT, require_ext
    ok = (tuple(weight.shape[1:]) == (cin, 3, 3)
          and cin % 64 == 0 and 64 <= cin <= 2048
          and cout % 64 == 0 and 64 <= cout <= 2048
          and n >= 1 and h >= 1 and 1 <= w <= 128
          and n * ((h + 1) // 2 + 1) * ((w + 1) // 2 + 1)
          + (w + 1) // 2 + 2 < 2 ** 31
          and n * h * w < 2 ** 31
          and x.dtype == torch.bfloat16
          and weight.dtype == torch.bfloat16
          and x.is_contiguous(memory_format=torch.channels_last)
          and weight.is_contiguous(memory_format=torch.channels_last))
    if ok and not HAVE_EXT:
        require_ext()  # asked for, and missing: no silent fallback
    return ok


class _Conv3x3S2Fn(torch.autograd.Function):
    """Stride-2 forward on conv3x3s2.hip, returning ``(out, partial)`` as
    ``_Conv3x3HipFn`` does; data-grad on its kernel where
    ``MI355X_CONV3X3_S2_DGRAD`` engages; weight-grad on aten."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stats: bool):
        from . import _C
        n, _, h, w = x.shape
        cout = weight.shape[0]
        out = torch.empty((n, cout, (h + 1) // 2, (w + 1) // 2),
                          dtype=torch.bfloat16, device=x.device,
                          memory_format=torch.channels_last)
        partial = None
        if stats:
            partial = torch.empty(
                2 * cout * _C.conv3x3_s2_fwd_blocks(n, h, w),
                dtype=torch.float32, device=x.device)
            ctx.mark_non_differentiable(partial)
        _C.conv3x3_s2_fwd(x.permute(0, 2, 3, 1), weight.permute(0, 2, 3, 1),
                          out.permute(0, 2, 3, 1), partial)
        ctx.save_for_backward(x, weight)
        ctx.set_materialize_grads(False)
        return out, partial

    @staticmethod
    def backward(ctx, dy, _dpartial):
        if dy is None:
            return None, None, None
        from . import _C
        x, weight = ctx.saved_tensors
        if dy.dtype != torch.bfloat16:
            dy = dy.to(torch.bfloat16)
        dy = dy.contiguous(memory_format=torch.channels_last)
        n, cin, h, w = x.shape
        hip_dgrad = _engaged("MI355X_CONV3X3_S2_DGRAD", _S2_TABLE,
                             (cin, weight.shape[0]), n, h, w)
        need_dx, need_dw = ctx.needs_input_grad[:2]
        # whatever stays on aten (the weight-grad always) goes in one call
        mask = [need_dx and not hip_dgrad, need_dw, False]
        dx = dw = None
        if mask[0] or mask[1]:
            dx, dw, _ = torch.ops.aten.convolution_backward(
                dy, x, weight, None, *_S2, mask)
        if need_dx and hip_dgrad:
            dx = torch.empty_like(x)
            wflip = torch.empty(weight.numel(), dtype=torch.bfloat16,
                                device=weight.device)
            _C.conv3x3_s2_dgrad(dy.permute(0, 2, 3, 1),
                                weight.permute(0, 2, 3, 1), wflip,
                                dx.permute(0, 2, 3, 1))
        return dx, dw, None


class _Conv3x3Fn(torch.autograd.Function):
    """The node of an engaged ``MI355X_CONV_WRW``: weight-grad on
    conv3x3wrw.hip; forward and data-grad on conv3x3.hip where their
    switches engage."""

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
    """3x3/p1 conv (no bias), stride 1 or 2, with the per-shape MFMA HIP
    paths. A stride-2 module answers to ``MI355X_CONV3X3_S2`` and
    ``MI355X_CONV3X3_S2_DGRAD`` only."""

    def __init__(self, cin: int, cout: int, stride: int = 1):
        if stride not in (1, 2):
            raise ValueError(f"Conv3x3: stride must be 1 or 2, not {stride}")
        super().__init__(cin, cout, 3, stride=stride, padding=1, bias=False)

    @property
    def _s2(self) -> bool:
        return self.stride[0] == 2

    def _hip_ok(self, x: torch.Tensor) -> bool:
        """The weight-grad kernel's gate (``MI355X_CONV_WRW`` or the table)."""
        if self._s2 or not x.is_cuda or x.dim() != 4:
            return False
        from . import HAVE_EXT, require_ext
        C = self.out_channels
        n, _, h, w = x.shape
        ok = (_engaged("MI355X_CONV_WRW", _WRW_TABLE, C, n, h, w)
              and self.in_channels == C and x.shape[1] == C
              and C % 64 == 0 and C <= 2048
              and n >= 1 and h >= 1 and 1 <= w <= 64
              and n * (h + 2) * (w + 2) + 2 * w + 6 < 2 ** 31
              and x.dtype == torch.bfloat16
              and self.weight.dtype == torch.bfloat16
              and x.is_contiguous(memory_format=torch.channels_last)
              and self.weight.is_contiguous(
                  memory_format=torch.channels_last))
        if ok and not HAVE_EXT:
            require_ext()  # asked for, and missing: no silent fallback
        return ok

    def stats_ok(self, x: torch.Tensor) -> bool:
        """True when ``forward_with_stats`` will run the fused kernel."""
        if self._s2:
            return _s2_gate(x, self.weight)
        return _fwd_gate(x, self.weight)

    def forward_with_stats(self, x: torch.Tensor):
        """``(conv(x), partial)``: ``partial`` holds the per-block BN sums
        of the output for ``FusedBNReLU2d.forward(..., partial=...)``, or
        is None when the HIP forward does not engage."""
        if self._s2 and self.stats_ok(x):
            return _Conv3x3S2Fn.apply(x, self.weight, True)
        if self.stats_ok(x):
            return _Conv3x3HipFn.apply(x, self.weight, True, self._hip_ok(x))
        return self.forward(x), None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._s2:
            if self.stats_ok(x):
                return _Conv3x3S2Fn.apply(x, self.weight, False)[0]
            return F.conv2d(x, self.weight, None, 2, 1)
        if self.stats_ok(x):
            return _Conv3x3HipFn.apply(x, self.weight, False,
                                       self._hip_ok(x))[0]
        if self._hip_ok(x):
            return _Conv3x3Fn.apply(x, self.weight)
        return F.conv2d(x, self.weight, None, 1, 1)
