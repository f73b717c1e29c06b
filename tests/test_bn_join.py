"""Residual-join gradient add fused into the BN backward reduce.

A block output has two consumers, so its closing ``FusedBNReLU2d`` used to
see one gradient that autograd had summed with a stand-alone bf16 add. The
joined path hands the two gradients to ``bn_bwd_reduce_join`` unsummed; the
kernel forms ``bf16(float(g1) + float(g2))`` per element, which is what the
add kernel stored, so everything downstream must be bit-identical.

``MI355X_BN_JOIN=0`` is the single-output path these tests compare against.
"""
import gc
import itertools
import weakref

import pytest
import torch
import torch.nn as nn

from mi355x_scale.models.resnet import BasicBlock, Bottleneck
from mi355x_scale.ops.fused_bn import FusedBNReLU2d


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------ kernel

# C -> thread mapping of the reduce kernel (256 threads, C/8 vector lanes
# per row): 8 = one lane per row; 64 = 8 lanes, 32 rows per block
# iteration (98 rows: ragged tail, 4 blocks); 512 = 64 lanes, 4 rows per
# iteration; 2048 = one row per iteration. (64, 1x2x2): fewer rows than
# one block iteration.
_KERNEL_SHAPES = [(8, 3, 5, 5), (64, 2, 7, 7), (512, 3, 5, 5),
                  (2048, 2, 3, 3), (64, 1, 2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C,N,H,W", _KERNEL_SHAPES)
def test_gpu_join_kernel_bit_identical(C, N, H, W, relu):
    from mi355x_scale.ops import _C
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1000 + C + N * H * W)

    def rnd(scale=1.0):
        return _cl((torch.randn(N, C, H, W, device=dev, generator=g)
                    * scale).bfloat16())

    # gradients of mixed magnitude, so the bf16 rounding of the sum matters
    g1, g2, x = rnd(), rnd(0.37), rnd(2.0)
    y = rnd()
    y = _cl(torch.where(
        torch.rand(y.shape, device=dev, generator=g) < 0.25,
        torch.zeros_like(y), y))  # both signs and exact zeros
    assert (y == 0).any() and (y > 0).any() and (y < 0).any()
    mean = torch.randn(C, device=dev, generator=g) * 0.3
    invstd = torch.rand(C, device=dev, generator=g) + 0.5

    dym_a = torch.empty_like(x)
    dym_b = torch.empty_like(x)
    dz = _cl(g1 + g2)  # torch's bf16 add: what autograd hands over today
    pa = _C.bn_bwd_reduce(dz, y, x, mean, invstd, dym_a, C, relu)
    pb = _C.bn_bwd_reduce_join(g1, g2, y, x, mean, invstd, dym_b, C, relu)
    torch.cuda.synchronize()
    assert pa.shape == pb.shape
    assert torch.equal(pa, pb)
    assert torch.equal(dym_a, dym_b)
    # and the sums are not trivially zero
    assert pa.abs().max() > 0 and dym_a.float().abs().max() > 0


@pytest.mark.gpu
def test_gpu_join_binding_checks_second_gradient():
    from mi355x_scale.ops import _C
    dev = torch.device("cuda:0")
    C = 64
    x = _cl(torch.randn(2, C, 4, 4, device=dev).bfloat16())
    mean = torch.zeros(C, device=dev)
    invstd = torch.ones(C, device=dev)
    dym = torch.empty_like(x)
    for bad in (x.float(),                       # dtype
                x[:1].contiguous(memory_format=torch.channels_last),  # shape
                x.contiguous()):                 # NCHW strides
        with pytest.raises(RuntimeError):
            _C.bn_bwd_reduce_join(x, bad, x, x, mean, invstd, dym, C, True)


# ---------------------------------------------------------------- function

class _TwoConsumers(nn.Module):
    """bn(x) + residual, its output read by two different consumers the way
    two chained blocks do: one through the tensor, one through its twin."""

    def __init__(self, C, relu=True):
        super().__init__()
        self.bn = FusedBNReLU2d(C, relu=relu)

    def forward(self, x, res, a, b, two=True):
        y = self.bn(x, residual=res)
        if not two:
            return (y * a).float().sum()
        twin = getattr(y, FusedBNReLU2d.JOIN_ATTR, None)
        skip = y if twin is None else twin
        return (y * a).float().sum() + (skip * b).float().sum()


def _function_run(monkeypatch, join, two, relu=True):
    monkeypatch.setenv("MI355X_BN_JOIN", join)
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    C = 64
    m = _TwoConsumers(C, relu).to(dev)
    with torch.no_grad():
        m.bn.weight.copy_(torch.rand(C) + 0.5)
        m.bn.bias.copy_(torch.randn(C) * 0.1)
    x = _cl(torch.randn(3, C, 7, 7, device=dev).bfloat16()).requires_grad_()
    r = _cl(torch.randn(3, C, 7, 7, device=dev).bfloat16()).requires_grad_()
    a = _cl(torch.randn(3, C, 7, 7, device=dev).bfloat16())
    b = _cl((torch.randn(3, C, 7, 7, device=dev) * 0.3).bfloat16())
    before = FusedBNReLU2d.join_calls
    m(x, r, a, b, two).backward()
    torch.cuda.synchronize()
    return ([x.grad, r.grad, m.bn.weight.grad, m.bn.bias.grad],
            FusedBNReLU2d.join_calls - before)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
def test_gpu_function_two_consumers_bit_identical(monkeypatch, relu):
    on, n_on = _function_run(monkeypatch, "1", True, relu)
    off, n_off = _function_run(monkeypatch, "0", True, relu)
    assert n_on == 1 and n_off == 0
    for name, p, q in zip(("x", "residual", "weight", "bias"), on, off):
        assert p is not None and torch.equal(p, q), name
        assert p.float().abs().max() > 0, name


@pytest.mark.gpu
def test_gpu_function_single_consumer_not_joined(monkeypatch):
    on, n_on = _function_run(monkeypatch, "1", False)
    off, n_off = _function_run(monkeypatch, "0", False)
    assert n_on == 0 and n_off == 0
    for name, p, q in zip(("x", "residual", "weight", "bias"), on, off):
        assert torch.equal(p, q), name


@pytest.mark.gpu
def test_gpu_twin_only_where_joinable(monkeypatch):
    """One tensor comes back either way; the twin rides only on a training
    residual layer's output, shares its storage, and is released with it."""
    monkeypatch.setenv("MI355X_BN_JOIN", "1")
    dev = torch.device("cuda:0")
    m = FusedBNReLU2d(64).to(dev)
    x = _cl(torch.randn(2, 64, 4, 4, device=dev).bfloat16()).requires_grad_()
    r = _cl(torch.randn(2, 64, 4, 4, device=dev).bfloat16())
    attr = FusedBNReLU2d.JOIN_ATTR

    y = m(x, residual=r)
    twin = getattr(y, attr)
    assert isinstance(y, torch.Tensor) and twin.shape == y.shape
    assert twin.data_ptr() == y.data_ptr() and twin.stride() == y.stride()
    assert getattr(m(x), attr, None) is None          # no residual
    monkeypatch.setenv("MI355X_BN_JOIN", "0")
    assert getattr(m(x, residual=r), attr, None) is None
    monkeypatch.setenv("MI355X_BN_JOIN", "1")
    m.eval()
    assert getattr(m(x, residual=r), attr, None) is None
    with torch.no_grad():
        assert getattr(m(x, residual=r), attr, None) is None

    storage = weakref.ref(y.untyped_storage())
    del y, twin
    gc.collect()
    assert storage() is None, "joined output is kept alive by a cycle"


# ------------------------------------------------------------------- model

def _randomize_bn(model, seed):
    # zero_init_residual leaves every block's closing BN with weight 0,
    # which zeroes the gradients this change is about
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, FusedBNReLU2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g)
                                 + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)


def _grads_of(model, fn, monkeypatch, join):
    monkeypatch.setenv("MI355X_BN_JOIN", join)
    for p in model.parameters():
        p.grad = None
    before = FusedBNReLU2d.join_calls
    fn().backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    return grads, FusedBNReLU2d.join_calls - before


def _max_diff(a, b):
    return max((a[n].float() - b[n].float()).abs().max().item() for n in a)


def _check_model(model, fn, monkeypatch, want_joins):
    """Gradients with the join against the single-output path. The conv
    weight-grad kernels (MIOpen's, the stem's) use atomics, so the limit is
    twice the largest difference seen between runs of the single-output
    path itself, measured here (0 when those runs are deterministic)."""
    FusedBNReLU2d.gpu_fallbacks.clear()
    offs = []
    for _ in range(3):
        g, n = _grads_of(model, fn, monkeypatch, "0")
        assert n == 0
        offs.append(g)
    noise = max(_max_diff(p, q) for p, q in itertools.combinations(offs, 2))
    on, n = _grads_of(model, fn, monkeypatch, "1")
    assert n == want_joins
    assert not FusedBNReLU2d.gpu_fallbacks, FusedBNReLU2d.gpu_fallbacks[:8]
    assert set(on) == set(offs[0])
    for name, gr in on.items():
        assert torch.isfinite(gr).all(), name
    diff = _max_diff(on, offs[0])
    print(f"join-vs-single max|d|={diff:.3e}  single-vs-single "
          f"max|d|={noise:.3e}")
    assert diff <= 2 * noise
    assert max(g.float().abs().max().item() for g in on.values()) > 0


@pytest.mark.gpu
def test_gpu_resnet18_join_matches_single_output(monkeypatch):
    from mi355x_scale.models import resnet18
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    model = resnet18(num_classes=10)
    _randomize_bn(model, 12)
    model = model.to(dev).to(memory_format=torch.channels_last)
    x = torch.randint(0, 255, (2, 3, 64, 64), device=dev).float()

    def fn():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            return model(x).float().logsumexp(1).mean()

    # 8 blocks: every block output but the last is read by a next block
    _check_model(model, fn, monkeypatch, want_joins=7)


@pytest.mark.gpu
def test_gpu_resnet50_stage_join_matches_single_output(monkeypatch):
    from mi355x_scale.models import resnet50
    dev = torch.device("cuda:0")
    torch.manual_seed(13)
    net = resnet50(num_classes=10)
    _randomize_bn(net, 14)
    stage = net.layer2  # 4 bottlenecks, the first with a strided downsample
    assert all(isinstance(b, Bottleneck) for b in stage)
    stage = stage.to(dev).to(memory_format=torch.channels_last)
    x = _cl(torch.randn(2, 256, 16, 16, device=dev).bfloat16())

    def fn():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            return stage(x).float().square().mean()

    _check_model(stage, fn, monkeypatch, want_joins=3)


# --------------------------------------------------------------------- cpu

def _cpu_model_run(monkeypatch, join):
    from mi355x_scale.models import resnet18
    monkeypatch.setenv("MI355X_BN_JOIN", join)
    torch.manual_seed(21)
    model = resnet18(num_classes=10)
    _randomize_bn(model, 22)
    x = torch.randn(2, 3, 32, 32)
    before = FusedBNReLU2d.join_calls
    out = model(x)
    out.logsumexp(1).mean().backward()
    assert FusedBNReLU2d.join_calls == before
    return out.detach(), {n: p.grad for n, p in model.named_parameters()}


def test_cpu_model_unchanged_by_join_switch(monkeypatch):
    out1, g1 = _cpu_model_run(monkeypatch, "1")
    out0, g0 = _cpu_model_run(monkeypatch, "0")
    assert torch.equal(out1, out0)
    for n in g0:
        assert g1[n] is not None and torch.equal(g1[n], g0[n]), n


def test_cpu_fused_bn_output_has_no_twin(monkeypatch):
    monkeypatch.setenv("MI355X_BN_JOIN", "1")
    m = FusedBNReLU2d(8)
    y = m(torch.randn(2, 8, 4, 4), residual=torch.randn(2, 8, 4, 4))
    assert getattr(y, FusedBNReLU2d.JOIN_ATTR, None) is None


@pytest.mark.parametrize("block,cin", [(BasicBlock, 8), (Bottleneck, 32)])
def test_cpu_block_takes_plain_tensor(block, cin):
    """A block fed a tensor without a twin reads it on both paths, and
    autograd adds the two gradients as before."""
    torch.manual_seed(31)
    blk = block(cin, 8)
    _randomize_bn(blk, 32)
    x = torch.randn(2, cin, 6, 6, requires_grad=True)
    out = blk(x)
    out.square().sum().backward()

    x2 = x.detach().clone().requires_grad_(True)
    mods = list(blk.children())  # conv/bn pairs in order, downsample last
    h = x2
    convs = [m for m in mods if isinstance(m, nn.Conv2d)]
    bns = [m for m in mods if isinstance(m, FusedBNReLU2d)]
    assert len(convs) == len(bns) >= 2
    for conv, bn in zip(convs[:-1], bns[:-1]):
        h = bn(conv(h))
    want = bns[-1](convs[-1](h), residual=x2)
    want.square().sum().backward()
    assert torch.equal(out, want)
    assert torch.equal(x.grad, x2.grad)
