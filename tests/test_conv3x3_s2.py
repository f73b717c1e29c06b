"""3x3/s2/p1 conv MFMA kernels against fp64 (ops/csrc/conv3x3s2.hip).

The conventions of tests/test_conv3x3_fwd.py: bf16 operands from a seeded
CPU generator, every reference computed in fp64 on the CPU from THOSE
values, and the bound derived in tests/test_conv1x1.py, |y - ref| <=
2^-8 * |ref| + 2*K * 2^-24 * S, S the same operation on the absolute values.
K = 9 * Cin for the forward and 4 * Cout for the data-grad (at most four
taps reach an input pixel at stride 2).
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_scale.models.resnet import resnet18
from mi355x_scale.ops import _C
from mi355x_scale.ops.conv3x3 import Conv3x3
from mi355x_scale.ops.fused_bn import FusedBNReLU2d

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -8, 2.0 ** -24
BF16 = torch.bfloat16
CL = torch.channels_last
S1_SWITCHES = ("MI355X_CONV3X3", "MI355X_CONV3X3_DGRAD", "MI355X_CONV_WRW")
S2_SWITCHES = ("MI355X_CONV3X3_S2", "MI355X_CONV3X3_S2_DGRAD")

# (N, H, W, Cin, Cout)
FWD_SHAPES = [
    (3, 7, 7, 64, 128),     # odd map, 75 virtual pixels: spans images, tail
    (2, 14, 14, 128, 64),   # exactly one full tile, even map, two chunks
    (3, 14, 13, 64, 256),   # two tiles, W odd and H even, four column tiles
    (1, 9, 30, 192, 128),   # H odd and W even, three chunks
    (1, 2, 128, 64, 64),    # the widest band the gate allows
    (2, 1, 3, 64, 64),      # H = 1: the odd-row planes are empty
    (1, 7, 7, 512, 512),    # the longest reduction that stays cheap
]
DGRAD_SHAPES = [FWD_SHAPES[i] for i in (0, 2, 3, 6, 5)]


def _osize(h, w):
    return (h + 1) // 2, (w + 1) // 2


@functools.lru_cache(maxsize=None)
def _operands(shape, grad):
    """bf16 map (x, or dy when ``grad``) and weight [Cout,3,3,Cin], NHWC,
    CPU and GPU copies."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(cin * 4096 + cout + n)
    ho, wo = _osize(h, w)
    a = torch.randn(*((n, ho, wo, cout) if grad else (n, h, w, cin)),
                    generator=g).to(BF16)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) * (9 * cin) ** -0.5).to(BF16)
    return a, wt, a.cuda(), wt.cuda()


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double()


def _assert_bound(y, ref, s, k):
    """y (bf16 NHWC, GPU) against the fp64 NCHW ref within the derived bound."""
    err = (_nchw64(y.cpu()) - ref).abs()
    bound = U16 * ref.abs() + 2 * k * U32 * s
    print(f"max err/bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()  # a NaN left in y fails here


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_fp64(shape):
    n, h, w, cin, cout = shape
    x, wt, xg, wg = _operands(shape, False)
    y = torch.full((n, *_osize(h, w), cout), float("nan"), dtype=BF16,
                   device="cuda")
    _C.conv3x3_s2_fwd(xg, wg, y)
    x64, w64 = _nchw64(x), _nchw64(wt)
    _assert_bound(y, F.conv2d(x64, w64, stride=2, padding=1),
                  F.conv2d(x64.abs(), w64.abs(), stride=2, padding=1), 9 * cin)


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_stats_of_own_output(shape):
    n, h, w, cin, cout = shape
    ho, wo = _osize(h, w)
    m = n * ho * wo
    _, _, xg, wg = _operands(shape, False)
    nb = _C.conv3x3_s2_fwd_blocks(n, h, w)
    assert nb == -(-n * (ho + 1) * (wo + 1) // 128)
    runs = []
    for _ in range(2):
        y = torch.empty(n, ho, wo, cout, dtype=BF16, device="cuda")
        partial = torch.full((2 * cout * nb,), float("nan"), device="cuda")
        _C.conv3x3_s2_fwd(xg, wg, y, partial)
        runs.append((y, partial))
    (y, partial), (y2, partial2) = runs
    assert torch.equal(y, y2) and torch.equal(partial, partial2)
    plain = torch.empty_like(y)
    _C.conv3x3_s2_fwd(xg, wg, plain)
    assert torch.equal(y, plain)
    got = partial.double().cpu().reshape(2 * cout, nb).sum(1)
    y64 = y.double().cpu().reshape(m, cout)
    s1, s2 = y64.sum(0), (y64 * y64).sum(0)
    assert ((got[:cout] - s1).abs() <= m * U32 * y64.abs().sum(0)).all()
    assert ((got[cout:] - s2).abs() <= m * U32 * s2).all()


@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_dgrad_fp64(shape):
    n, h, w, cin, cout = shape
    dy, wt, dyg, wg = _operands(shape, True)
    dx = torch.full((n, h, w, cin), float("nan"), dtype=BF16, device="cuda")
    _C.conv3x3_s2_dgrad(dyg, wg, torch.empty_like(wg), dx)
    dy64, w64 = _nchw64(dy), _nchw64(wt)
    size = (n, cin, h, w)
    _assert_bound(
        dx, torch.nn.grad.conv2d_input(size, w64, dy64, stride=2, padding=1),
        torch.nn.grad.conv2d_input(size, w64.abs(), dy64.abs(), stride=2,
                                   padding=1), 4 * cout)


def _rel(got, ref):
    return ((got.double().cpu() - ref.double()).norm()
            / ref.double().norm()).item()


def test_module_through_public_interface(monkeypatch):
    for name in S1_SWITCHES + S2_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    torch.manual_seed(0)
    m = Conv3x3(64, 128, stride=2).cuda().to(BF16).to(memory_format=CL)
    x = torch.randn(2, 64, 9, 9).to(BF16)
    dy = torch.randn(2, 128, 5, 5).to(BF16)
    xg = x.cuda().contiguous(memory_format=CL).requires_grad_(True)
    dyg = dy.cuda().contiguous(memory_format=CL)
    eager = F.conv2d(xg, m.weight, stride=2, padding=1)

    assert not m.stats_ok(xg) and torch.equal(m(xg), eager)
    for name in S1_SWITCHES:  # they must not touch a stride-2 module
        monkeypatch.setenv(name, "1")
    assert not m.stats_ok(xg) and torch.equal(m(xg), eager)
    assert m.forward_with_stats(xg)[1] is None
    for name in S1_SWITCHES:
        monkeypatch.delenv(name)

    for name in S2_SWITCHES:
        monkeypatch.setenv(name, "1")
    assert m.stats_ok(xg)
    out = m(xg)
    out.backward(dyg)
    x64, dy64, w64 = x.double(), dy.double(), m.weight.detach().double().cpu()
    _assert_bound(out.detach().permute(0, 2, 3, 1),
                  F.conv2d(x64, w64, stride=2, padding=1),
                  F.conv2d(x64.abs(), w64.abs(), stride=2, padding=1), 9 * 64)
    _assert_bound(
        xg.grad.permute(0, 2, 3, 1),
        torch.nn.grad.conv2d_input(x.shape, w64, dy64, stride=2, padding=1),
        torch.nn.grad.conv2d_input(x.shape, w64.abs(), dy64.abs(), stride=2,
                                   padding=1), 4 * 128)
    dw64 = torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, stride=2,
                                       padding=1)
    assert _rel(m.weight.grad, dw64) < 3e-2


def test_resnet18_layer2_block(monkeypatch):
    """resnet18().layer2[0] (64 -> 128, stride 2, with its downsample) on the
    stride-2 kernels against its fp32 CPU composition, by the recipe of
    test_basic_block_through_public_interface: bf16-representable conv
    weights, BN biases four standard deviations of their ReLU's input above
    zero so that no ReLU mask moves (bn2's ReLU sees the sum of two unit
    variance BN outputs)."""
    torch.manual_seed(0)
    ref = resnet18().layer2[0].train()
    torch.nn.init.constant_(ref.bn1.bias, 4.0)
    torch.nn.init.ones_(ref.bn2.weight)  # zero-initialised in the model
    torch.nn.init.constant_(ref.bn2.bias, 4.0 * 2 ** 0.5)
    convs = ("conv1", "conv2", "downsample.0")
    for name in convs:
        conv = ref.get_submodule(name)
        conv.weight.data = conv.weight.data.to(BF16).float()
    blk = copy.deepcopy(ref).cuda()
    for name in convs:
        blk.get_submodule(name).to(BF16)
    blk.to(memory_format=CL)
    x = torch.randn(2, 64, 9, 9).to(BF16)
    dy = torch.randn(2, 128, 5, 5).to(BF16)
    xg = x.cuda().contiguous(memory_format=CL).requires_grad_(True)

    assert isinstance(blk.conv1, Conv3x3) and blk.conv1.stride == (2, 2)
    for name in S2_SWITCHES:
        monkeypatch.setenv(name, "1")
    assert blk.conv1.stats_ok(xg)
    seen = {}  # the conv output bn1 is fed
    blk.bn1.register_forward_pre_hook(
        lambda m, args: seen.__setitem__("bn1", args[0]))
    fallbacks = len(FusedBNReLU2d.gpu_fallbacks)
    out = blk(xg)
    out.backward(dy.cuda().contiguous(memory_format=CL))
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

    bn = blk.bn1
    y64 = seen["bn1"].double().cpu().transpose(0, 1).flatten(1)
    mean = bn.running_mean.double().cpu() / bn.momentum
    var = (bn.running_var.double().cpu() - (1 - bn.momentum)) / bn.momentum
    assert _rel(mean, y64.mean(1)) < 1e-4
    assert _rel(var, y64.var(1, unbiased=True)) < 1e-4
    assert bn.num_batches_tracked.item() == 1
