"""3x3/s1/p1 conv MFMA kernels against fp64 (ops/csrc/conv3x3.hip).

Inputs are bf16 values from a seeded generator; every reference casts
THOSE values to fp64 and computes on the CPU. The bound is the one derived
in tests/test_conv1x1.py with K = 9 * (reduced channels): |y - ref| <=
2^-8 * |ref| + 2*K * 2^-24 * S, S the same convolution of the absolute
values.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_scale.models.resnet import BasicBlock
from mi355x_scale.ops import _C
from mi355x_scale.ops.conv3x3 import Conv3x3
from mi355x_scale.ops.fused_bn import FusedBNReLU2d

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -8, 2.0 ** -24
BF16 = torch.bfloat16

# (N, H, W, Cin, Cout)
FWD_SHAPES = [
    (2, 7, 7, 64, 64),       # 162 virtual pixels: a tile spans two images, tail
    (1, 14, 14, 192, 192),   # 256: two full tiles, three chunks, three col tiles
    (1, 9, 15, 128, 64),     # H != W, Cin != Cout, band restaged once
    (3, 5, 6, 64, 128),      # W < 16: every fragment crosses rows; Cout > Cin
    (1, 3, 64, 64, 64),      # the widest band the gate allows
    (1, 7, 7, 512, 512),     # the longest reduction (K = 4608)
]
DGRAD_SHAPES = [(2, 7, 7, 64, 128), (1, 9, 15, 128, 64), (1, 7, 7, 512, 512)]


@functools.lru_cache(maxsize=None)
def _operands(shape, cmap):
    """bf16 map [N,H,W,cmap] and weight [Cout,3,3,Cin], CPU and GPU copies."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(cin * 4096 + cout + n)
    a = torch.randn(n, h, w, cmap, generator=g).to(BF16)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) * (9 * cin) ** -0.5).to(BF16)
    return a, wt, a.cuda(), wt.cuda()


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double()


def _assert_bound(y, ref, s, k):
    """y (bf16 NHWC, GPU) against the fp64 NCHW ref within the derived bound."""
    err = (_nchw64(y.cpu()) - ref).abs()
    bound = U16 * ref.abs() + 2 * k * U32 * s
    print(f"max err/bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_fp64(shape):
    n, h, w, cin, cout = shape
    x, wt, xg, wg = _operands(shape, cin)
    y = torch.full((n, h, w, cout), float("nan"), dtype=BF16, device="cuda")
    _C.conv3x3_fwd(xg, wg, y)
    x64, w64 = _nchw64(x), _nchw64(wt)
    _assert_bound(y, F.conv2d(x64, w64, padding=1),
                  F.conv2d(x64.abs(), w64.abs(), padding=1), 9 * cin)


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_stats_of_own_output(shape):
    n, h, w, cin, cout = shape
    m = n * h * w
    _, _, xg, wg = _operands(shape, cin)
    nb = _C.conv3x3_fwd_blocks(n, h, w)
    assert nb == -(-n * (h + 2) * (w + 2) // 128)
    runs = []
    for _ in range(2):
        y = torch.empty(n, h, w, cout, dtype=BF16, device="cuda")
        partial = torch.full((2 * cout * nb,), float("nan"), device="cuda")
        _C.conv3x3_fwd(xg, wg, y, partial)
        runs.append((y, partial))
    (y, partial), (y2, partial2) = runs
    assert torch.equal(y, y2) and torch.equal(partial, partial2)
    plain = torch.empty_like(y)
    _C.conv3x3_fwd(xg, wg, plain)
    assert torch.equal(y, plain)
    got = partial.double().cpu().reshape(2 * cout, nb).sum(1)
    y64 = y.double().cpu().reshape(m, cout)
    s1, s2 = y64.sum(0), (y64 * y64).sum(0)
    assert ((got[:cout] - s1).abs() <= m * U32 * y64.abs().sum(0)).all()
    assert ((got[cout:] - s2).abs() <= m * U32 * s2).all()


@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_dgrad_fp64(shape):
    n, h, w, cin, cout = shape
    dy, wt, dyg, wg = _operands(shape, cout)
    dx = torch.full((n, h, w, cin), float("nan"), dtype=BF16, device="cuda")
    _C.conv3x3_dgrad(dyg, wg, torch.empty_like(wg), dx)
    dy64, w64 = _nchw64(dy), _nchw64(wt)
    size = (n, cin, h, w)
    _assert_bound(
        dx, torch.nn.grad.conv2d_input(size, w64, dy64, padding=1),
        torch.nn.grad.conv2d_input(size, w64.abs(), dy64.abs(), padding=1),
        9 * cout)


def _rel(got, ref):
    return ((got.double().cpu() - ref.double()).norm()
            / ref.double().norm()).item()


def test_basic_block_through_public_interface(monkeypatch):
    """BasicBlock(64, 64) with both switches on against its fp32 CPU
    composition, by the recipe of test_bottleneck_through_public_interface:
    bf16-representable conv weights, and BN biases four standard deviations
    of their ReLU's input above zero so that no ReLU mask moves (bn2's ReLU
    sees bn2(..) + x, of variance 2). A bare block has no zero-initialised
    BN weight, and none of its gradients is zero by construction: a shift
    of bn1's output reaches conv2's zero padding, so bn2 does not cancel
    it. Every gradient is held to 3e-2 of its own norm."""
    torch.manual_seed(0)
    ref = BasicBlock(64, 64).train()
    torch.nn.init.constant_(ref.bn1.bias, 4.0)
    torch.nn.init.constant_(ref.bn2.bias, 4.0 * 2 ** 0.5)
    for conv in (ref.conv1, ref.conv2):
        conv.weight.data = conv.weight.data.to(BF16).float()
    blk = copy.deepcopy(ref).cuda()
    blk.conv1.to(BF16)
    blk.conv2.to(BF16)
    blk.to(memory_format=torch.channels_last)
    x = torch.randn(2, 64, 9, 9).to(BF16)
    dy = torch.randn(2, 64, 9, 9).to(BF16)
    xg = x.cuda().contiguous(memory_format=torch.channels_last)
    xg.requires_grad_(True)

    assert isinstance(blk.conv1, Conv3x3) and isinstance(blk.conv2, Conv3x3)
    monkeypatch.delenv("MI355X_CONV_WRW", raising=False)
    monkeypatch.delenv("MI355X_CONV3X3", raising=False)
    assert not blk.conv1.stats_ok(xg) and not blk.conv2.stats_ok(xg)
    monkeypatch.setenv("MI355X_CONV3X3", "1")
    monkeypatch.setenv("MI355X_CONV3X3_DGRAD", "1")
    assert blk.conv1.stats_ok(xg) and blk.conv2.stats_ok(xg)

    seen = {}
    for name in ("bn1", "bn2"):  # the conv outputs the BNs are fed
        getattr(blk, name).register_forward_pre_hook(
            lambda m, args, name=name: seen.__setitem__(name, args[0]))
    fallbacks = len(FusedBNReLU2d.gpu_fallbacks)
    out = blk(xg)
    out.backward(dy.cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert len(FusedBNReLU2d.gpu_fallbacks) == fallbacks

    xr = x.float().requires_grad_(True)
    out_ref = ref(xr)
    out_ref.backward(dy.float())
    ref_params = dict(ref.named_parameters())
    rels = {"out": _rel(out, out_ref), "dx": _rel(xg.grad, xr.grad)}
    for name, p in blk.named_parameters():
        rels[name] = _rel(p.grad, ref_params[name].grad)
    print({k: round(v, 4) for k, v in rels.items()})
    assert max(rels.values()) < 3e-2, rels

    for name in ("bn1", "bn2"):
        bn = getattr(blk, name)
        y64 = seen[name].double().cpu().transpose(0, 1).flatten(1)
        mean = bn.running_mean.double().cpu() / bn.momentum
        var = (bn.running_var.double().cpu() - (1 - bn.momentum)) / bn.momentum
        assert _rel(mean, y64.mean(1)) < 1e-4, name
        assert _rel(var, y64.var(1, unbiased=True)) < 1e-4, name
        assert bn.num_batches_tracked.item() == 1
