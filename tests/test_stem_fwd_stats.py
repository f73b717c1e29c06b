"""Stem forward conv with wide stores and BN batch statistics in its epilogue.

``stem_conv_fwd_stats_kernel`` (``MI355X_STEM_FUSED_STATS``, default on)
handles several output rows per block, stores its output as 16-byte vectors
and leaves per-block channel sums of the bf16 values it stored in the
``[2C][nblocks]`` layout ``bn_fwd_finalize`` reads, so the stem's
``bn_fwd_reduce`` pass disappears. Checked here:

1. the output is bit-identical to the one-row-per-block kernel's;
2. the block slots sum to the float64 sums of the kernel's own output within
   the bound for fp32 summation in any order, ``(n-1) * 2^-24 * sum|x_i|``
   (likewise for the squares), and exactly where every partial sum is an
   integer below 2^24; ``mean``/``invstd`` from ``bn_fwd_finalize`` on that
   partial follow within the same bound, propagated;
3. the ``ResNet`` stem (``conv1`` -> ``bn1.forward_pooled``) in training
   mode, switch on and off: counter, running statistics, pooled output and
   all gradients;
4. conv + ``forward_pooled`` captured in a graph replays to bit-identical
   ``mean``/``invstd``.

Every shape has ``n = N*HO*WO < 4096``; there the bound stays below the
mean ``|x_i|``, i.e. below what one typical missing or doubled pixel costs
(``test_bound_arithmetic`` checks that arithmetic on the CPU), and the
integer cases catch any single pixel whatever its size.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_scale.models.resnet import BasicBlock, ResNet
from mi355x_scale.ops.fused_bn import FusedBNReLU2d
from mi355x_scale.ops.stemconv import (StemConv2d, _StemConvFn,
                                       _StemConvStatsFn)

U = 2.0 ** -24                     # fp32 unit roundoff
EPS = 1e-5
MOMENTUM = 0.1
# (N, 3, H, W): odd sizes (HO 38 = 4 full row chunks + a tail of 6, WO 27 =
# a partial pixel tile); even; HO 7 < one chunk; WO 128 = the full tile
SHAPES = ((3, 3, 75, 53), (2, 3, 64, 64), (1, 3, 14, 14), (1, 3, 16, 256))
SWITCH = "MI355X_STEM_FUSED_STATS"


def _C():
    from mi355x_scale.ops import _C as ext, require_ext
    require_ext()
    return ext


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """bf16 channels-last (x, weight) on the GPU; built once, never modified.

    kind "random": gaussian x, kaiming-sized weights.
    kind "integer": x in {0, 1}, weights in {-1, 0, 1} (one in four
    non-zero): every output is an integer of magnitude <= 147, which bf16
    holds exactly, so every partial sum and sum of squares the kernel can
    form is an integer; the test asserts the totals stay below 2^24, which
    makes them exact in fp32 in any order."""
    n, _, h, w = shape
    g = torch.Generator().manual_seed(7 * h + w + n)
    if kind == "integer":
        x = torch.randint(0, 2, shape, generator=g).float()
        wt = (torch.randint(-1, 2, (64, 3, 7, 7), generator=g)
              * (torch.randint(0, 4, (64, 3, 7, 7), generator=g) == 0)).float()
    else:
        x = torch.randn(shape, generator=g)
        wt = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    return (_cl(x.to(torch.bfloat16).cuda()), _cl(wt.to(torch.bfloat16).cuda()))


@functools.lru_cache(maxsize=None)
def _fused(shape, kind):
    """(out, partial) of the fused kernel for one case; shared, read-only."""
    x, wt = _inputs(shape, kind)
    out, partial = _StemConvStatsFn.apply(x, wt)
    torch.cuda.synchronize()
    return out, partial


def _slot_sums(partial, c=64):
    """float64 per-channel (sum, sum of squares) over the block slots."""
    p = partial.double().view(2 * c, -1).sum(1)
    return p[:c], p[c:]


def _f64_stats(y):
    """float64 per-channel figures of a bf16 NCHW map and the error bounds
    that follow from them for fp32 sums in any order."""
    y64 = y.double()
    n = y64.numel() // y64.shape[1]
    s = y64.sum((0, 2, 3))
    q = (y64 * y64).sum((0, 2, 3))
    a = y64.abs().sum((0, 2, 3))
    b_s = (n - 1) * U * a                     # sum|x_i|
    b_q = (n - 1) * U * q                     # sum|x_i^2| = q
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0)
    # propagated through the finalize arithmetic (fp32: m = s/n,
    # var = q/n - m*m, invstd = rsqrt(var + eps)); each fp32 operation adds
    # one rounding (u relative) of its own result:
    e_mean = b_s / n + U * mean.abs()
    e_var = (b_q / n + 2 * mean.abs() * e_mean + e_mean ** 2
             + 4 * U * (q / n + mean * mean))
    invstd = torch.rsqrt(var + EPS)
    # |d invstd| <= 0.5 * e_var * (var + eps - e_var)^-3/2, plus the add's
    # rounding and a rsqrt good to a few ulp (8u relative in all)
    low = (var + EPS - e_var).clamp_min(1e-300)
    e_invstd = 0.5 * e_var * low ** -1.5 + 8 * U * invstd
    return dict(n=n, s=s, q=q, a=a, b_s=b_s, b_q=b_q, mean=mean, var=var,
                invstd=invstd, e_mean=e_mean, e_var=e_var, e_invstd=e_invstd)


# ------------------------------------------------- 0. the bound's arithmetic
def test_bound_arithmetic():
    """CPU: fp32 sums of n < 4096 terms taken in three different orders stay
    within (n-1)*2^-24*sum|x_i| of the float64 sum, and for every n used
    below that bound is smaller than the mean |x_i| (one typical pixel)."""
    g = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        ho, wo = _out_hw(shape[2], shape[3])
        n = shape[0] * ho * wo
        assert n < 4096
        x = torch.randn(n, generator=g).to(torch.bfloat16).float()
        for v in (x, x * x):
            exact = v.double().sum()
            bound = (n - 1) * U * v.double().abs().sum()
            seq = torch.zeros((), dtype=torch.float32)
            for t in v:                          # strictly sequential
                seq = seq + t
            chunked = torch.stack([c.sum() for c in v.split(37)]).sum()
            strided = torch.stack([v[i::64].sum() for i in range(64)]).sum()
            for got in (seq, chunked, strided):
                assert abs(got.double() - exact) <= bound
            assert bound < v.double().abs().mean()


# ------------------------------------------------------ 1. bit-identical output
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("shape", SHAPES)
def test_output_bit_identical_to_unfused(monkeypatch, shape, kind):
    x, wt = _inputs(shape, kind)
    monkeypatch.setenv(SWITCH, "0")
    ref = _StemConvFn.apply(x, wt)
    monkeypatch.setenv(SWITCH, "1")
    on = _StemConvFn.apply(x, wt)              # single-tensor entry point
    out, partial = _fused(shape, kind)         # (out, partial) entry point
    torch.cuda.synchronize()
    ho, wo = _out_hw(shape[2], shape[3])
    assert ref.shape == (shape[0], 64, ho, wo)
    assert partial.numel() == 2 * 64 * _C().stem_fwd_blocks(shape[0], ho)
    assert not partial.requires_grad
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(on, ref)
    assert torch.equal(out, ref)
    # against an independent fp32 convolution of the same bf16 inputs
    want = F.conv2d(x.float(), wt.float(), None, 2, 3)
    rel = ((ref.float() - want).norm() / want.norm()).item()
    assert rel < 1e-2, rel


# ---------------------------------------------------------------- 2. statistics
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_partial_sums_within_fp32_bound(shape):
    out, partial = _fused(shape, "random")
    st = _f64_stats(out)
    assert st["n"] < 4096
    s, q = _slot_sums(partial)
    err_s = (s - st["s"]).abs()
    err_q = (q - st["q"]).abs()
    print(f"{shape}: n={st['n']} max err/bound sum "
          f"{(err_s / st['b_s']).max().item():.3e} sumsq "
          f"{(err_q / st['b_q']).max().item():.3e}; bound/mean|x| "
          f"{(st['b_s'] / (st['a'] / st['n'])).max().item():.3e}")
    assert (err_s <= st["b_s"]).all()
    assert (err_q <= st["b_q"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_partial_sums_exact_on_integers(shape):
    """Integer outputs: every partial sum is exact, so one pixel counted
    twice, dropped, or taken from the padding shows as an inequality."""
    out, partial = _fused(shape, "integer")
    st = _f64_stats(out)
    assert (out.float() == out.float().round()).all()
    assert st["a"].max() > 0 and st["q"].max() < 2 ** 24
    s, q = _slot_sums(partial)
    assert torch.equal(s, st["s"])
    assert torch.equal(q, st["q"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_finalize_on_partial_matches_f64(shape):
    out, partial = _fused(shape, "random")
    st = _f64_stats(out)
    dev = out.device
    mean = torch.empty(64, dtype=torch.float32, device=dev)
    invstd = torch.empty(64, dtype=torch.float32, device=dev)
    rm = torch.zeros(64, device=dev)
    rv = torch.ones(64, device=dev)
    _C().bn_fwd_finalize(partial, mean, invstd, rm, rv, MOMENTUM, EPS,
                         st["n"], 64, True)
    torch.cuda.synchronize()
    err_m = (mean.double() - st["mean"]).abs()
    err_i = (invstd.double() - st["invstd"]).abs()
    print(f"{shape}: max err/bound mean {(err_m / st['e_mean']).max().item():.3e}"
          f" invstd {(err_i / st['e_invstd']).max().item():.3e}")
    assert (err_m <= st["e_mean"]).all()
    assert (err_i <= st["e_invstd"]).all()
    # and the separate reduce over the same map lands inside the same bound
    mean2 = torch.empty_like(mean)
    invstd2 = torch.empty_like(invstd)
    _C().bn_fwd_finalize(_C().bn_fwd_reduce(out, 64), mean2, invstd2,
                         torch.zeros_like(rm), torch.ones_like(rv), MOMENTUM,
                         EPS, st["n"], 64, True)
    assert ((mean2.double() - st["mean"]).abs() <= st["e_mean"]).all()
    assert ((invstd2.double() - st["invstd"]).abs() <= st["e_invstd"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1024, 1025, 2968, 4100])
def test_finalize_long_partial_runs(nb):
    """The flagship stem hands finalize 2,968 slots per channel; above 1,024
    a block-per-channel kernel sums them. Slot counts on both sides of the
    threshold, a multiple of the 1,024-slot stride plus a remainder, against
    the float64 sums of the same slots; bound as above with n = nb terms."""
    g = torch.Generator().manual_seed(nb)
    c, rows = 64, 37 * nb
    ps = torch.randn(c, nb, generator=g) * 30 + 5
    pq = torch.rand(c, nb, generator=g) * 4000 + 1500     # E[x^2] > mean^2
    partial = torch.cat([ps, pq]).reshape(-1).cuda()
    s, q = ps.double().sum(1), pq.double().sum(1)
    b_s = (nb - 1) * U * ps.double().abs().sum(1)
    b_q = (nb - 1) * U * pq.double().sum(1)
    mean64 = s / rows
    var64 = q / rows - mean64 ** 2
    assert (var64 > 1).all()
    e_mean = b_s / rows + U * mean64.abs()
    e_var = (b_q / rows + 2 * mean64.abs() * e_mean + e_mean ** 2
             + 4 * U * (q / rows + mean64 ** 2))
    invstd64 = torch.rsqrt(var64 + EPS)
    e_invstd = 0.5 * e_var * (var64 + EPS - e_var) ** -1.5 + 8 * U * invstd64
    mean = torch.empty(c, dtype=torch.float32, device="cuda")
    invstd = torch.empty_like(mean)
    rm, rv = torch.zeros_like(mean), torch.ones_like(mean)
    nbt = torch.zeros((), dtype=torch.long, device="cuda")
    _C().bn_fwd_finalize(partial, mean, invstd, rm, rv, MOMENTUM, EPS, rows,
                         c, True, nbt)
    torch.cuda.synchronize()
    assert ((mean.cpu().double() - mean64).abs() <= e_mean).all()
    assert ((invstd.cpu().double() - invstd64).abs() <= e_invstd).all()
    assert nbt.item() == 1
    want_rm = MOMENTUM * mean64
    want_rv = (1 - MOMENTUM) + MOMENTUM * var64 * rows / (rows - 1)
    assert ((rm.cpu().double() - want_rm).abs()
            <= MOMENTUM * e_mean + U * want_rm.abs()).all()
    assert ((rv.cpu().double() - want_rv).abs()
            <= MOMENTUM * e_var * 1.001 + 4 * U * want_rv.abs()).all()


# ---------------------------------------------------------------- 3. module path
def _stem_model():
    """ResNet whose forward is only its stem: conv1 -> bn1.forward_pooled,
    the pooled map flattened. conv1 in bf16 as in the flagship."""
    torch.manual_seed(5)
    m = ResNet(BasicBlock, [1, 1, 1, 1], num_classes=8)
    for name in ("layer1", "layer2", "layer3", "layer4", "avgpool", "fc"):
        setattr(m, name, torch.nn.Identity())
    m = m.cuda().to(memory_format=torch.channels_last)
    m.conv1.to(torch.bfloat16)
    with torch.no_grad():                       # a non-trivial affine
        m.bn1.weight.copy_(1.0 + 0.25 * torch.randn(64))
        m.bn1.bias.copy_(0.1 * torch.randn(64))
    return m.train()


def _run_stem(monkeypatch, model0, toggle, x, g):
    monkeypatch.setenv(SWITCH, toggle)
    m = copy.deepcopy(model0)
    seen = {}
    inner = m.bn1.forward_pooled

    def spy(y, partial=None):                   # observe what forward hands over
        y.retain_grad()
        seen["y"], seen["partial"] = y, partial
        return inner(y, partial)

    m.bn1.forward_pooled = spy
    reduces = []
    ext = _C()
    real_reduce = ext.bn_fwd_reduce
    monkeypatch.setattr(ext, "bn_fwd_reduce",
                        lambda *a: (reduces.append(1), real_reduce(*a))[1])
    pooled = m(x)                               # [N, 64*16*16]
    pooled.backward(g)
    torch.cuda.synchronize()
    monkeypatch.setattr(ext, "bn_fwd_reduce", real_reduce)
    return dict(m=m, pooled=pooled.detach(), y=seen["y"].detach(),
                dx=seen["y"].grad, had_partial=seen["partial"] is not None,
                reduces=len(reduces))


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.gpu
def test_resnet_stem_training_both_paths(monkeypatch):
    model0 = _stem_model()
    gen = torch.Generator().manual_seed(11)
    x = _cl(torch.randn(2, 3, 64, 64, generator=gen).to(torch.bfloat16).cuda())
    g = torch.randn(2, 64 * 16 * 16, generator=gen).to(torch.bfloat16).cuda()
    on = _run_stem(monkeypatch, model0, "1", x, g)
    off = _run_stem(monkeypatch, model0, "0", x, g)

    # routing: the switch decides who sums the statistics
    assert on["had_partial"] and on["reduces"] == 0
    assert not off["had_partial"] and off["reduces"] == 1
    assert torch.equal(on["y"], off["y"])
    for r in (on, off):
        assert r["m"].bn1.num_batches_tracked.item() == 1

    # running statistics: the two paths agree within the summation bound
    # carried through the momentum update
    st = _f64_stats(on["y"])
    n = st["n"]
    d_rm = (on["m"].bn1.running_mean - off["m"].bn1.running_mean).double().abs()
    d_rv = (on["m"].bn1.running_var - off["m"].bn1.running_var).double().abs()
    b_rm = MOMENTUM * st["e_mean"]
    b_rv = MOMENTUM * st["e_var"] * n / (n - 1)
    print(f"running mean diff/bound {(d_rm / b_rm).max().item():.3e} "
          f"var {(d_rv / b_rv).max().item():.3e}")
    assert (d_rm <= b_rm).all()
    assert (d_rv <= b_rv).all()
    want_rm = MOMENTUM * st["mean"]
    want_rv = (1 - MOMENTUM) + MOMENTUM * st["var"] * n / (n - 1)
    for r in (on, off):
        assert ((r["m"].bn1.running_mean.double() - want_rm).abs()
                <= b_rm + U * want_rm.abs()).all()
        assert ((r["m"].bn1.running_var.double() - want_rv).abs()
                <= b_rv + 4 * U * want_rv.abs()).all()   # the update's own
        # roundings: n/(n-1), the two products, the sum

    # fp32 composition from the same bf16 inputs and parameters. BN and the
    # pool are fed the bf16 stem map itself (as tests/test_stem_bwd_fused.py
    # feeds them the bf16 x): pooling the unrounded fp32 conv output instead
    # moves the argmax of windows whose two largest values differ by less
    # than a bf16 ulp, which is a property of the reference, not of the path
    # under test (measured that way: dx 6.5e-2). The conv's weight grad
    # reference is the fp32 conv backward of that composition's dx.
    wref = model0.conv1.weight.detach().float().requires_grad_(True)
    bn_ref = torch.nn.BatchNorm2d(64, eps=EPS, momentum=MOMENTUM).cuda()
    with torch.no_grad():
        bn_ref.weight.copy_(model0.bn1.weight)
        bn_ref.bias.copy_(model0.bn1.bias)
    y32 = F.conv2d(x.float(), wref, None, 2, 3)
    assert _rel(on["y"], y32) < 1e-2
    y_ref = on["y"].float().requires_grad_(True)
    p_ref = F.max_pool2d(F.relu(bn_ref(y_ref)), 3, stride=2, padding=1)
    p_ref.backward(g.float().view_as(p_ref))
    y32.backward(y_ref.grad)
    for name, r in (("on", on), ("off", off)):
        figs = dict(
            pooled=_rel(r["pooled"].reshape(p_ref.shape), p_ref),
            dx=_rel(r["dx"], y_ref.grad),
            dweight=_rel(r["m"].bn1.weight.grad, bn_ref.weight.grad),
            dbias=_rel(r["m"].bn1.bias.grad, bn_ref.bias.grad),
            conv_dw=_rel(r["m"].conv1.weight.grad, wref.grad))
        print(name, " ".join(f"{k} {v:.3e}" for k, v in figs.items()))
        for k, v in figs.items():
            assert v < 3e-2, f"{k} rel {v} (switch {name})"


@pytest.mark.gpu
def test_eval_and_switch_off_take_the_plain_path(monkeypatch):
    """Eval mode never asks the conv for statistics, and forward_pooled
    ignores a partial outside training."""
    m = _stem_model().eval()
    x = _cl(torch.randn(2, 3, 64, 64).to(torch.bfloat16).cuda())
    monkeypatch.setenv(SWITCH, "1")
    called = []
    real = m.conv1.forward_with_stats
    m.conv1.forward_with_stats = lambda t: (called.append(1), real(t))[1]
    with torch.no_grad():
        a = m(x)
        y, partial = real(x)
        b = m.bn1.forward_pooled(y, partial).flatten(1)
    assert not called
    assert partial is not None
    assert torch.equal(a, b)
    assert m.bn1.num_batches_tracked.item() == 0
    monkeypatch.setenv(SWITCH, "0")
    assert not m.conv1.stats_ok(x)
    assert real(x)[1] is None


# ---------------------------------------------------------------- 4. graph replay
@pytest.mark.gpu
def test_graph_replay_statistics_bit_identical():
    conv = StemConv2d().cuda().to(torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    bn = FusedBNReLU2d(64).cuda().train()
    x = _inputs(SHAPES[0], "random")[0]

    def step():
        y, partial = conv.forward_with_stats(x)
        assert partial is not None
        out = bn.forward_pooled(y, partial)
        _, mean, invstd = out.grad_fn.saved_tensors[:3]
        return out, mean, invstd

    out_e, mean_e, invstd_e = (t.clone() for t in step())   # eager
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, mean, invstd = step()
    start = bn.num_batches_tracked.item()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mean, mean_e)
        assert torch.equal(invstd, invstd_e)
        assert torch.equal(out, out_e)
    assert bn.num_batches_tracked.item() == start + 3
    st = _f64_stats(conv(x).detach())
    assert ((mean_e.double() - st["mean"]).abs() <= st["e_mean"]).all()
