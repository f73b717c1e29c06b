"""Pointwise conv weight-grad MFMA kernels against fp64 (ops/csrc/conv1x1.hip).

Operands are bf16 values from a seeded generator; the reference casts THOSE
values to fp64 on the CPU. With u16 = 2^-8 and u32 = 2^-24, |dw - ref| <=
u16*|ref| + 2*M*u32*S, S = |dY|^T . |X|: one bf16 rounding of an fp32 sum
over M terms (the chunk sums and their sum), no measured constant.
"""
import pytest
import torch

from mi355x_scale.ops import _C
from mi355x_scale.ops.conv1x1 import Conv1x1

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -8, 2.0 ** -24
BF16 = torch.bfloat16

# (N, H, W, Cin, Cout, chunks requested, chunks expected; None = the default
# rule's). The K-step is 32 rows, so M = 147 is five steps, the last with 19
# live rows.
SHAPES = [
    (3, 7, 7, 64, 64, 1, 1),       # tail rows inside a single chunk
    (3, 7, 7, 64, 64, 2, 2),       # chunks of 3 + 2 steps: ragged last chunk
    (3, 7, 7, 64, 64, 4, 3),       # 4 does not divide 5: 2 + 2 + 1, returns 3
    (2, 8, 8, 128, 64, 0, None),   # M = 128 = four full steps; 64 x 128 tile
    (1, 9, 15, 192, 128, 2, 2),    # Cin = 192 takes 64-wide tiles, Cout 128
    (2, 14, 14, 64, 256, 0, None),  # default rule, two 128 x 64 tiles
    (1, 7, 7, 2048, 512, 0, None),  # widest output, 64 tiles of 128 x 128
    (1, 7, 7, 512, 2048, 0, None),  # the other widest output
]


def _operands(n, h, w, cin, cout):
    """bf16 x [N,H,W,Cin] and dy [N,H,W,Cout] on the CPU."""
    g = torch.Generator().manual_seed(cin * 4096 + cout + n)
    return (torch.randn(n, h, w, cin, generator=g).to(BF16),
            torch.randn(n, h, w, cout, generator=g).to(BF16))


def _assert_wrw(dw, x, dy):
    """dw (bf16, GPU) against fp64 dy^T @ x within the derived bound."""
    a, b = dy.double().flatten(0, 2).t(), x.double().flatten(0, 2)
    ref, s = a @ b, a.abs() @ b.abs()
    err = (dw.double().cpu().reshape(ref.shape) - ref).abs()
    bound = U16 * ref.abs() + 2 * a.shape[1] * U32 * s
    print(f"max err/bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def _run(x, dy, chunks, dw=None, accumulate=False):
    m, cin, cout = x[..., 0].numel(), x.shape[-1], dy.shape[-1]
    nch = _C.conv1x1_wrw_nchunks(m, cin, cout, chunks)
    part = torch.full((nch * cout * cin,), float("nan"), device="cuda")
    if dw is None:
        dw = torch.empty(cout, cin, dtype=BF16, device="cuda")
    _C.conv1x1_wrw(x.cuda(), dy.cuda(), part, dw, accumulate, chunks)
    return dw, nch


@pytest.mark.parametrize("shape", SHAPES)
def test_wrw_fp64(shape):
    *dims, chunks, expect = shape
    x, dy = _operands(*dims)
    dw, nch = _run(x, dy, chunks)
    assert expect is None or nch == expect
    _assert_wrw(dw, x, dy)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]])
def test_reproducible_and_accumulate(shape):
    *dims, chunks, _ = shape
    x, dy = _operands(*dims)
    dw, _ = _run(x, dy, chunks)
    assert torch.equal(dw, _run(x, dy, chunks)[0])
    g0 = torch.randn(dw.shape, generator=torch.Generator().manual_seed(1)) \
        .to(BF16).cuda()
    acc, _ = _run(x, dy, chunks, g0.clone(), True)
    assert torch.equal(acc, g0 + dw)


def test_public_interface_writes_grad_view(monkeypatch):
    monkeypatch.setenv("MI355X_CONV1X1", "1")
    monkeypatch.setenv("MI355X_CONV1X1_WRW", "1")
    torch.manual_seed(0)
    conv = Conv1x1(256, 64).to(BF16).cuda().to(
        memory_format=torch.channels_last)
    x, dy = _operands(2, 9, 9, 256, 64)
    xg = x.cuda().permute(0, 3, 1, 2)    # channels-last NCHW views
    dyg = dy.cuda().permute(0, 3, 1, 2)
    conv(xg).backward(dyg)
    dw = conv.weight.grad.clone()
    _assert_wrw(dw, x, dy)
    assert torch.equal(dw.reshape(64, 256), _run(x, dy, 0)[0])

    g0 = torch.randn(dw.shape, generator=torch.Generator().manual_seed(2)) \
        .to(BF16).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        conv(xg).backward(dyg)
    torch.cuda.current_stream().wait_stream(side)
    conv.weight.grad = g0.clone()
    view = conv.weight.grad.data_ptr()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        conv(xg).backward(dyg)
    graph.replay()
    torch.cuda.synchronize()
    # the kernel added into the view; autograd did not add a second time
    assert conv.weight.grad.data_ptr() == view
    assert torch.equal(conv.weight.grad, g0 + dw)
