"""Fused BatchNorm(+residual)(+ReLU) — Python surface over fused_bn.hip.

``FusedBNReLU2d`` is a drop-in replacement for the
``nn.BatchNorm2d (+ residual add) + nn.ReLU`` groups in the ResNet family
(the reference runs torchvision resnet50's BN/ReLU through cuDNN,
``deep_learning/2.distributed-data-loading-petastorm.py:150``; PyTorch-ROCm
routes them to MIOpen as four fp32 kernels per BN plus standalone
elementwise passes). The HIP path runs when the input is bf16 on GPU —
the flagship autocast training config — and is mandatory there (no
silent eager fallback if the extension is missing). On CPU, or for
dtypes/channel counts the kernel doesn't cover, the plain PyTorch
composition below doubles as the numerics reference used by the tests.

State-dict layout matches ``nn.BatchNorm2d`` (weight, bias, running_mean,
running_var, num_batches_tracked) so checkpoints interoperate.

Passes and kernels the HIP path leaves out:

* Non-residual relu layers recompute the relu mask in backward as
  ``(w*xhat + b) > 0`` from the saved x (``bn_bwd_*_rm``): the stored y is
  read by neither backward pass and is not saved.
* Residual layers' outputs are block outputs with two consumers (the next
  block's conv1, and its identity path or downsample conv). In training
  ``_FusedBNFn`` returns that output twice over one storage; ``BasicBlock``
  / ``Bottleneck`` feed one path from each, so backward receives the two
  gradients unsummed and the joined ``bn_bwd_reduce`` adds them while it
  streams (bf16-rounded, bit-identical to autograd's add): the stand-alone
  add of two activation-size maps per block does not run.
  ``MI355X_BN_JOIN=0`` selects the single-output path for A/B runs and
  tests; ``FusedBNReLU2d.join_calls`` counts joined backwards.
* The stem (``forward_pooled``) folds affine+relu into the max-pool window
  reads, so the normalized stem map is never materialized; it accepts the
  per-block channel sums the stem conv's epilogue already produced
  (``StemConv2d.forward_with_stats``) and then skips ``bn_fwd_reduce``, so
  the 340 MB stem map is not read back for its statistics. Its backward
  rebuilds the un-pooled gradient in registers from the pooled gradient
  and the u8 window codes (``bn_pool_bwd_*``);
  ``MI355X_BN_POOL_FUSED_BWD=0`` selects the three-kernel path for A/B.
* ``bn_fwd_finalize`` bumps ``num_batches_tracked`` on the device, so no
  per-BN ``+= 1`` kernel runs; inside hipGraph capture ``bn_bwd_finalize``
  accumulates straight into the flat grad views (``MI355X_BN_FUSED_ACC``).

All device work is stream-ordered with no host sync, so the op captures
into hipGraphs (train/graphstep.py).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C, require_ext


def _hip_supported(x: torch.Tensor) -> bool:
    # C = 8*2^k up to 2048: one 256-thread block must tile whole rows
    # (256 % lanes == 0) and a row must fit one block (lanes <= 256).
    # Covers every BN in the ResNet family (64..2048).
    c = x.shape[1]
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
            and c % 8 == 0 and c <= 2048 and (256 % (c // 8)) == 0)


def _channel_grads(weight, bias, C, dev):
    """Where ``bn_bwd_finalize`` puts dweight/dbias: ``(dweight, dbias,
    fuse_acc)``.

    Inside hipGraph capture (the flagship graphed step) the kernel
    accumulates straight into the existing flat grad views and backward
    returns None for weight/bias — autograd's per-param AccumulateGrad adds
    (~40 launch-bound kernels/step across the model's BNs) vanish from the
    captured graph. Outside capture (eager, DDP hooks, tests with fresh
    .grad) fresh buffers keep the standard return-grads contract.
    """
    def _grad_view(p):
        g = p.grad
        if (g is not None and g.is_cuda and g.is_contiguous()
                and g.dtype == torch.float32 and g.numel() == C):
            return g
        return None

    wg, bg = _grad_view(weight), _grad_view(bias)
    fuse_acc = (torch.cuda.is_current_stream_capturing()
                and wg is not None and bg is not None
                and os.environ.get("MI355X_BN_FUSED_ACC", "1") == "1")
    if fuse_acc:
        return wg, bg, True
    return (torch.empty(C, dtype=torch.float32, device=dev),
            torch.empty(C, dtype=torch.float32, device=dev), False)


class _FusedBNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var,
                momentum, eps, relu, num_batches_tracked, join=False):
        C = x.shape[1]
        rows = x.numel() // C
        dev = x.device
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty(C, dtype=torch.float32, device=dev)
        partial = _C.bn_fwd_reduce(x, C)
        # the finalize kernel also bumps the step counter when given one
        _C.bn_fwd_finalize(partial, mean, invstd, running_mean, running_var,
                           momentum, eps, rows, C, True, num_batches_tracked)
        y = torch.empty_like(x)
        res = residual if residual is not None else x.new_empty(0)
        _C.bn_fwd_apply(x, res, y, mean, invstd, weight, bias, C, relu)
        # Non-residual backward recomputes the relu mask from
        # (w*xhat + b) > 0, so y need not be kept alive; the saved slot
        # holds x again (free — same tensor).
        ctx.save_for_backward(x, y if residual is not None else x,
                              mean, invstd, weight, bias)
        ctx.relu = relu
        ctx.has_res = residual is not None
        if not join:
            return y
        # Two outputs over one storage: a consumer of y and a consumer of
        # the alias each send their own gradient to backward, UNSUMMED, so
        # the reduce kernel can add them itself. An unused output's grad
        # arrives as None instead of a zero-filled map.
        ctx.set_materialize_grads(False)
        return y, y.view_as(y)

    @staticmethod
    def backward(ctx, dz, dz2=None):
        x, y, mean, invstd, weight, bias = ctx.saved_tensors
        C = x.shape[1]
        rows = x.numel() // C
        if dz is None:
            dz, dz2 = dz2, None
        if dz is None:  # joined forward, neither output used
            return (None,) * 11
        if not dz.is_contiguous(memory_format=torch.channels_last):
            dz = dz.contiguous(memory_format=torch.channels_last)
        if (dz2 is not None and
                not dz2.is_contiguous(memory_format=torch.channels_last)):
            dz2 = dz2.contiguous(memory_format=torch.channels_last)
        k = torch.empty(3 * C, dtype=torch.float32, device=x.device)
        dweight, dbias, fuse_acc = _channel_grads(weight, bias, C, x.device)
        dx = torch.empty_like(x)
        dym = None
        # reduce
        if ctx.has_res:
            # residual layer: the reduce pass materializes the masked
            # upstream grad (dym) which IS the residual gradient; the
            # apply pass then reads (dym, x) — one read+write less than
            # re-deriving dy from (dz, y).
            dym = torch.empty_like(x)
            if dz2 is not None:
                # both consumers sent a gradient: the reduce sums them
                # (bf16-rounded like autograd's add) while it streams
                partial = _C.bn_bwd_reduce_join(dz, dz2, y, x, mean, invstd,
                                                dym, C, ctx.relu)
                FusedBNReLU2d.join_calls += 1
            else:
                partial = _C.bn_bwd_reduce(dz, y, x, mean, invstd, dym, C,
                                           ctx.relu)
        else:
            # only residual layers are joined in forward
            assert dz2 is None
            if ctx.relu:
                # recompute-mask path: one full activation-map read (the
                # stored y) drops out of BOTH backward passes
                partial = _C.bn_bwd_reduce_rm(dz, x, mean, invstd, weight,
                                              bias, x.new_empty(0), C)
            else:
                partial = _C.bn_bwd_reduce(dz, y, x, mean, invstd,
                                           x.new_empty(0), C, False)
        _C.bn_bwd_finalize(partial, invstd, weight, dweight, dbias, k, rows,
                           C, fuse_acc)
        # apply
        if ctx.has_res:
            _C.bn_bwd_apply_dym(dym, x, mean, invstd, k, dx, C)
        elif ctx.relu:
            _C.bn_bwd_apply_rm(dz, x, mean, invstd, bias, k, dx, C)
        else:
            _C.bn_bwd_apply(dz, y, x, mean, invstd, k, dx, x.new_empty(0),
                            C, False)
        if fuse_acc:  # the kernel already accumulated the channel grads
            dweight = dbias = None
        return (dx, dym, dweight, dbias, None, None, None, None, None, None,
                None)


class _FusedBNPoolFn(torch.autograd.Function):
    """Stem fusion: relu(bn(x)) + maxpool 3x3/s2/p1 with the normalized
    map never materialized (the recompute-mask backward only needs x).
    Saves a full 340 MB write + read per flagship step."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps, training, num_batches_tracked, partial=None):
        C = x.shape[1]
        dev = x.device
        if training:
            rows = x.numel() // C
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            invstd = torch.empty(C, dtype=torch.float32, device=dev)
            # a ready-made partial (the stem conv's epilogue sums, same
            # [2C][nblocks] layout) replaces the full read of x
            if partial is None:
                partial = _C.bn_fwd_reduce(x, C)
            # the finalize kernel also bumps the step counter
            _C.bn_fwd_finalize(partial, mean, invstd, running_mean,
                               running_var, momentum, eps, rows, C, True,
                               num_batches_tracked)
        else:
            mean = running_mean.to(torch.float32)
            invstd = torch.rsqrt(running_var.to(torch.float32) + eps)
        n, _, h, w = x.shape
        ho, wo = (h + 1) // 2, (w + 1) // 2
        y = torch.empty((n, C, ho, wo), dtype=x.dtype, device=dev,
                        memory_format=torch.channels_last)
        code = torch.empty(n * ho * wo * C, dtype=torch.uint8, device=dev)
        _C.bn_maxpool3x3s2_fwd(x, mean, invstd, weight, bias, y, code)
        ctx.save_for_backward(x, mean, invstd, weight, bias, code)
        return y

    @staticmethod
    def backward(ctx, dp):
        x, mean, invstd, weight, bias, code = ctx.saved_tensors
        C = x.shape[1]
        rows = x.numel() // C
        if not dp.is_contiguous(memory_format=torch.channels_last):
            dp = dp.contiguous(memory_format=torch.channels_last)
        # Default: the un-pooled map dz is rebuilt in registers inside
        # both BN passes (bn_pool_bwd_* kernels) and never allocated.
        # MI355X_BN_POOL_FUSED_BWD=0 selects the three-kernel path
        # (un-pool to dz, then the rm kernels) for A/B runs and tests.
        # Deliberately no hasattr() probe for the new pair: the extension
        # is built from this tree, and an extension without them must
        # raise rather than quietly run the slower path.
        fused_unpool = os.environ.get("MI355X_BN_POOL_FUSED_BWD", "1") != "0"
        k = torch.empty(3 * C, dtype=torch.float32, device=x.device)
        dweight, dbias, fuse_acc = _channel_grads(weight, bias, C, x.device)
        dx = torch.empty_like(x)
        if fused_unpool:
            partial = _C.bn_pool_bwd_reduce(dp, code, x, mean, invstd,
                                            weight, bias)
        else:
            # un-pool: scatter the pooled grad to the argmax positions,
            # then the recompute-mask BN backward (fused_bn.hip rm kernels)
            dz = torch.empty_like(x)
            _C.maxpool3x3s2_bwd(dp, code, dz)
            partial = _C.bn_bwd_reduce_rm(dz, x, mean, invstd, weight, bias,
                                          x.new_empty(0), C)
        _C.bn_bwd_finalize(partial, invstd, weight, dweight, dbias, k, rows,
                           C, fuse_acc)
        if fused_unpool:
            _C.bn_pool_bwd_apply(dp, code, x, mean, invstd, bias, k, dx)
        else:
            _C.bn_bwd_apply_rm(dz, x, mean, invstd, bias, k, dx, C)
        if fuse_acc:  # the kernel already accumulated the channel grads
            dweight = dbias = None
        return (dx, dweight, dbias, None, None, None, None, None, None, None)


class FusedBNReLU2d(nn.Module):
    """BatchNorm2d fused with an optional residual add and ReLU.

    ``forward(x, residual=None)`` computes
    ``relu?(bn(x) + residual?)`` in one HIP pass set on GPU/bf16.
    """

    # GPU-side dispatches that took the torch fallback (shape, dtype,
    # training) — should stay empty on the flagship bf16 path; the GPU
    # test asserts it (no silent MIOpen fallback).
    gpu_fallbacks: list = []

    # Backward calls that took the joined reduce (two gradients summed in
    # the kernel, see forward); tests assert the path was taken.
    join_calls: int = 0

    # Name of the attribute by which a joined output carries its twin.
    JOIN_ATTR = "_bn_join_twin"

    def __init__(self, num_features: int, eps: float = 1e-5,
                 momentum: float = 0.1, relu: bool = True):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.relu = relu
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked",
                             torch.tensor(0, dtype=torch.long))

    def extra_repr(self) -> str:
        return (f"{self.num_features}, eps={self.eps}, "
                f"momentum={self.momentum}, relu={self.relu}")

    def forward_pooled(self, x: torch.Tensor,
                       partial: Optional[torch.Tensor] = None
                       ) -> torch.Tensor:
        """``maxpool3x3s2(relu(bn(x)))`` with the normalized map never
        materialized (stem fusion; relu layers without residual only).
        ``partial``: per-block channel sums of ``x`` already produced by
        the kernel that wrote it (``StemConv2d.forward_with_stats``); in
        training mode on the HIP path the reduce pass over ``x`` is then
        skipped. Falls back to the composed ops off the GPU bf16 path."""
        assert self.relu, "pooled fusion is relu-only"
        if _hip_supported(x):
            require_ext()
            # training: bn_fwd_finalize bumps num_batches_tracked on the
            # device (no separate `+= 1` kernel); eval leaves it alone
            x = x.contiguous(memory_format=torch.channels_last)
            return _FusedBNPoolFn.apply(
                x, self.weight, self.bias, self.running_mean,
                self.running_var, self.momentum, self.eps, self.training,
                self.num_batches_tracked,
                partial if self.training else None)
        return F.max_pool2d(self.forward(x), 3, stride=2, padding=1)

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        if _hip_supported(x):
            require_ext()  # GPU bf16 path never falls back silently
            x = x.contiguous(memory_format=torch.channels_last)
            if residual is not None:
                residual = residual.contiguous(
                    memory_format=torch.channels_last)
            if self.training:
                # bn_fwd_finalize bumps num_batches_tracked on the device
                join = (residual is not None and
                        os.environ.get("MI355X_BN_JOIN", "1") != "0")
                out = _FusedBNFn.apply(
                    x, residual, self.weight, self.bias, self.running_mean,
                    self.running_var, self.momentum, self.eps, self.relu,
                    self.num_batches_tracked, join)
                if not join:
                    return out
                # Residual layer = a block's output, which the next block
                # reads twice (conv1 and identity / downsample). Callers
                # still get ONE tensor; it carries a second autograd output
                # over the same storage, and a block that feeds one path
                # from each (models/resnet.py) gets its two gradients
                # summed inside the joined bn_bwd_reduce instead of by a
                # stand-alone add kernel. A caller that ignores the twin
                # behaves as before. The returned tensor is the view and
                # holds the base, not the other way round: a base that held
                # its own view would be a reference cycle through the
                # view's base pointer and never be freed.
                y, alias = out
                setattr(alias, FusedBNReLU2d.JOIN_ATTR, y)
                return alias
            if not (torch.is_grad_enabled() and
                    (x.requires_grad or self.weight.requires_grad)):
                # inference: apply-only with running stats
                invstd = torch.rsqrt(self.running_var + self.eps)
                y = torch.empty_like(x)
                res = (residual if residual is not None else x.new_empty(0))
                _C.bn_fwd_apply(x, res, y, self.running_mean, invstd,
                                self.weight, self.bias, x.shape[1],
                                self.relu)
                return y
        # reference composition (CPU path and numerics oracle)
        if self.training:
            self.num_batches_tracked += 1
        if x.is_cuda and len(FusedBNReLU2d.gpu_fallbacks) < 256:
            # bounded: diagnostic only (tests assert it stays empty on
            # the flagship path)
            FusedBNReLU2d.gpu_fallbacks.append(
                (tuple(x.shape), str(x.dtype), self.training))
        y = F.batch_norm(x, self.running_mean, self.running_var, self.weight,
                         self.bias, self.training, self.momentum, self.eps)
        if residual is not None:
            y = y + residual
        return F.relu(y) if self.relu else y
