"""Stride-2 pointwise conv MFMA kernels against fp64 (ops/csrc/conv1x1.hip).

The conventions of tests/test_conv1x1.py: bf16 operands from a seeded CPU
generator, random at the skipped pixels too; the reference casts THOSE
values to fp64 and slices ``x[:, ::2, ::2]``. With u16 = 2^-8 and u32 =
2^-24 a K-term reduction obeys |y - ref| <= u16*|ref| + 2*K*u32*S, S =
sum |a||b| (derived, not measured): K is Cin for the forward, Cout for the
data-grad and M' = N*Ho*Wo for the weight-grad.
"""
import pytest
import torch
import torch.nn.functional as F

from mi355x_scale.models.resnet import resnet18
from mi355x_scale.ops import _C
from mi355x_scale.ops.conv1x1 import Conv1x1
from mi355x_scale.ops.fused_bn import FusedBNReLU2d

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -8, 2.0 ** -24
BF16 = torch.bfloat16

# (N, H, W, Cin, Cout)
FWD_SHAPES = [
    (3, 7, 7, 64, 64),      # odd map, M' = 48: a tail, rows cross images
    (2, 16, 16, 128, 64),   # M' = 128: exactly one tile, two K-steps
    (1, 9, 30, 192, 128),   # H odd, W even, Wo != Ho, three K-steps
    (3, 14, 13, 64, 256),   # M' = 147: a block boundary inside an image row
    (1, 5, 5, 2048, 512),   # the longest reduction
]
DGRAD_SHAPES = [(3, 7, 7, 64, 128), (1, 9, 30, 192, 64), (2, 16, 16, 128, 64),
                (1, 5, 5, 512, 2048)]
# (..., chunks). M' = 48 is two 32-row K-steps, the second with 16 live rows.
WRW_SHAPES = [(3, 7, 7, 64, 64, 1), (3, 7, 7, 64, 64, 2),
              (3, 14, 13, 64, 256, 4), (1, 9, 30, 192, 128, 0),
              (1, 5, 5, 2048, 512, 0)]


def _operands(n, h, w, cin, cout):
    """bf16 x [N,H,W,Cin], dy [N,Ho,Wo,Cout] and weight [Cout,Cin] (CPU)."""
    g = torch.Generator().manual_seed(cin * 4096 + cout + n)
    return (torch.randn(n, h, w, cin, generator=g).to(BF16),
            torch.randn(n, (h + 1) // 2, (w + 1) // 2, cout,
                        generator=g).to(BF16),
            (torch.randn(cout, cin, generator=g) * cin ** -0.5).to(BF16))


def _assert_matmul(y, a, b):
    """y (bf16, GPU) against fp64 a @ b within the derived bound."""
    a, b = a.double(), b.double()
    ref, s = a @ b, a.abs() @ b.abs()
    err = (y.double().cpu().reshape(ref.shape) - ref).abs()
    bound = U16 * ref.abs() + 2 * a.shape[1] * U32 * s
    print(f"max err/bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def _assert_dgrad(dx, dy, wt):
    """dx [N,H,W,Cin]: dy . w at the even pixels, exactly 0.0 elsewhere."""
    _assert_matmul(dx[:, ::2, ::2], dy.flatten(0, 2), wt)
    skipped = torch.ones(dx.shape[1:3], dtype=torch.bool)
    skipped[::2, ::2] = False
    assert (dx.cpu()[:, skipped] == 0).all()


def _assert_wrw(dw, x, dy):
    _assert_matmul(dw, dy.flatten(0, 2).t(), x[:, ::2, ::2].flatten(0, 2))


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_and_stats(shape):
    n, h, w, cin, cout = shape
    x, dy, wt = _operands(*shape)
    m = dy[..., 0].numel()
    nb = _C.conv1x1_fwd_blocks(m)
    xg, wg = x.cuda(), wt.cuda()
    plain = torch.full_like(dy, float("nan"), device="cuda")
    _C.conv1x1_s2_fwd(xg, wg, plain)
    _assert_matmul(plain, x[:, ::2, ::2].reshape(m, cin), wt.t())
    runs = []
    for _ in range(2):
        y = torch.empty_like(plain)
        partial = torch.full((2 * cout * nb,), float("nan"), device="cuda")
        _C.conv1x1_s2_fwd(xg, wg, y, partial)
        runs.append((y, partial))
    (y, partial), (y2, partial2) = runs
    assert torch.equal(y, plain)
    assert torch.equal(y, y2) and torch.equal(partial, partial2)
    got = partial.double().cpu().reshape(2 * cout, nb).sum(1)
    y64 = y.double().cpu().reshape(m, cout)
    s1, s2 = y64.sum(0), (y64 * y64).sum(0)
    assert ((got[:cout] - s1).abs() <= m * U32 * y64.abs().sum(0)).all()
    assert ((got[cout:] - s2).abs() <= m * U32 * s2).all()


@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_dgrad_fp64_and_zeros(shape):
    x, dy, wt = _operands(*shape)
    dx = torch.full_like(x, float("nan"), device="cuda")
    _C.conv1x1_s2_dgrad(dy.cuda(), wt.cuda(), dx)
    _assert_dgrad(dx, dy, wt)


def _run_wrw(x, dy, chunks, dw=None, accumulate=False):
    cin, cout = x.shape[-1], dy.shape[-1]
    nch = _C.conv1x1_wrw_nchunks(dy[..., 0].numel(), cin, cout, chunks)
    part = torch.full((nch * cout * cin,), float("nan"), device="cuda")
    if dw is None:
        dw = torch.empty(cout, cin, dtype=BF16, device="cuda")
    _C.conv1x1_s2_wrw(x.cuda(), dy.cuda(), part, dw, accumulate, chunks)
    return dw


@pytest.mark.parametrize("shape", WRW_SHAPES)
def test_wrw_fp64(shape):
    *dims, chunks = shape
    x, dy, _ = _operands(*dims)
    dw = _run_wrw(x, dy, chunks)
    _assert_wrw(dw, x, dy)
    if shape == WRW_SHAPES[1]:  # reproducible, and accumulate adds in bf16
        assert torch.equal(dw, _run_wrw(x, dy, chunks))
        g0 = torch.randn(dw.shape, generator=torch.Generator().manual_seed(1)
                         ).to(BF16).cuda()
        assert torch.equal(_run_wrw(x, dy, chunks, g0.clone(), True), g0 + dw)


def test_module_through_public_interface(monkeypatch):
    torch.manual_seed(0)
    conv = Conv1x1(128, 256, stride=2).to(BF16).cuda().to(
        memory_format=torch.channels_last)
    x, dy, _ = _operands(2, 9, 9, 128, 256)
    wt = conv.weight.detach().cpu().reshape(256, 128)
    xg = x.cuda().permute(0, 3, 1, 2).requires_grad_(True)  # channels-last
    monkeypatch.delenv("MI355X_CONV1X1", raising=False)
    monkeypatch.delenv("MI355X_CONV1X1_WRW", raising=False)
    assert not conv.stats_ok(xg)
    assert torch.equal(conv(xg), F.conv2d(xg, conv.weight, stride=2))
    monkeypatch.setenv("MI355X_CONV1X1", "1")
    monkeypatch.setenv("MI355X_CONV1X1_WRW", "1")
    assert conv.stats_ok(xg)
    out = conv(xg)
    out.backward(dy.cuda().permute(0, 3, 1, 2))
    assert out.shape == (2, 256, 5, 5)
    _assert_matmul(out.permute(0, 2, 3, 1), x[:, ::2, ::2].reshape(-1, 128),
                   wt.t())
    _assert_dgrad(xg.grad.permute(0, 2, 3, 1), dy, wt)
    _assert_wrw(conv.weight.grad, x, dy)


def test_resnet18_downsample_bn_gets_epilogue_stats(monkeypatch):
    monkeypatch.setenv("MI355X_CONV1X1", "1")
    monkeypatch.setenv("MI355X_CONV1X1_WRW", "1")
    torch.manual_seed(0)
    blk = resnet18().layer2[0].train().cuda()
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(BF16)
    blk.to(memory_format=torch.channels_last)
    conv, bn = blk.downsample
    assert isinstance(conv, Conv1x1) and conv.stride == (2, 2)
    xg = torch.randn(2, 64, 9, 9).to(BF16).cuda().contiguous(
        memory_format=torch.channels_last).requires_grad_(True)
    assert conv.stats_ok(xg)
    seen = []
    bn.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    fallbacks = len(FusedBNReLU2d.gpu_fallbacks)
    out = blk(xg)
    out.backward(torch.randn(out.shape).to(BF16).cuda().contiguous(
        memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert len(FusedBNReLU2d.gpu_fallbacks) == fallbacks
    assert conv.weight.grad is not None and xg.grad is not None

    def rel(got, ref):
        return ((got.double().cpu() - ref).norm() / ref.norm()).item()

    y64 = seen[0].double().cpu().transpose(0, 1).flatten(1)
    mean = bn.running_mean.double().cpu() / bn.momentum
    var = (bn.running_var.double().cpu() - (1 - bn.momentum)) / bn.momentum
    assert rel(mean, y64.mean(1)) < 1e-4
    assert rel(var, y64.var(1, unbiased=True)) < 1e-4
    assert bn.num_batches_tracked.item() == 1
