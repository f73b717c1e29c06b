"""Pointwise conv micro-benchmark: the MFMA GEMM kernels (ops/csrc/
conv1x1.hip) vs MIOpen on the twelve stride-1 1x1 shapes of ResNet-50 at
batch 212, bf16 channels-last. One JSON line per shape, times in us:

  miopen_fwd / miopen_fwd+reduce   F.conv2d, and F.conv2d + bn_fwd_reduce
  hip_fwd / hip_fwd_stats          conv1x1_fwd without / with BN partials
  miopen_dgrad / hip_dgrad         data-grad
  miopen_wrw                       MIOpen weight-grad + the bf16 add into a
                                   preallocated grad tensor (what autograd's
                                   AccumulateGrad does with the result)
  hip_wrw                          conv1x1_wrw, accumulate mode (both launches)
  hip_*_phase                      phase_mask 1 = loads + LDS staging only,
                                   4 = MFMA only, 2 = epilogue only (the
                                   weight-grad figures include the reduce launch)

Every shape also reports ``wrw_rel_vs_miopen`` and, to tell which of the
two is off when they differ, both weight-grads against fp64.

``--batch`` shrinks the batch (smoke runs); ``--chunks`` forces the
weight-grad's chunk count (0 = its default rule) for sweeps; ``--shapes``
picks shapes by index into SHAPES (default all)."""
import argparse
import json
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from mi355x_scale.ops import _C  # noqa: E402

# (Cin, Cout, H)
SHAPES = [(64, 64, 56), (64, 256, 56), (256, 64, 56), (256, 128, 56),
          (128, 512, 28), (512, 128, 28), (512, 256, 28),
          (256, 1024, 14), (1024, 256, 14), (1024, 512, 14),
          (512, 2048, 7), (2048, 512, 7)]


def timeit(fn, iters=30, warmup=8):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / iters * 1e6, 1)  # us


def bench_shape(n, cin, cout, h, g, chunks=0):
    dev = "cuda"
    cl = torch.channels_last
    x = torch.randn(n, cin, h, h, generator=g).to(dev).to(torch.bfloat16) \
        .to(memory_format=cl)
    wt = (torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5).to(dev) \
        .to(torch.bfloat16)
    y = torch.empty((n, cout, h, h), dtype=torch.bfloat16, device=dev,
                    memory_format=cl)
    dy = torch.randn(n, cout, h, h, generator=g).to(dev).to(torch.bfloat16) \
        .to(memory_format=cl)
    dx = torch.empty_like(x)
    m = n * h * h
    part = torch.empty(2 * cout * _C.conv1x1_fwd_blocks(m),
                       dtype=torch.float32, device=dev)
    xn, yn = x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)
    dyn, dxn = dy.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)

    def mio_dgrad():
        return torch.ops.aten.convolution_backward(
            dy, x, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            [True, False, False])[0]

    def mio_wrw():
        grad.add_(torch.ops.aten.convolution_backward(
            dy, x, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            [False, True, False])[1])

    grad = torch.zeros_like(wt)
    nch = _C.conv1x1_wrw_nchunks(m, cin, cout, chunks)
    wpart = torch.empty(nch * cout * cin, dtype=torch.float32, device=dev)

    res = {"shape": f"{cin}->{cout}@{h}", "batch": n, "M": m}
    res["miopen_fwd"] = timeit(lambda: F.conv2d(x, wt))
    ref = F.conv2d(x, wt)
    res["miopen_fwd+reduce"] = timeit(
        lambda: _C.bn_fwd_reduce(F.conv2d(x, wt), cout))
    res["hip_fwd"] = timeit(lambda: _C.conv1x1_fwd(xn, wt, yn))
    res["hip_fwd_stats"] = timeit(lambda: _C.conv1x1_fwd(xn, wt, yn, part))
    res["miopen_dgrad"] = timeit(mio_dgrad)
    res["hip_dgrad"] = timeit(lambda: _C.conv1x1_dgrad(dyn, wt, dxn))
    res["miopen_wrw"] = timeit(mio_wrw)
    res["hip_wrw"] = timeit(
        lambda: _C.conv1x1_wrw(xn, dyn, wpart, grad, True, chunks))
    res["wrw_chunks"] = nch
    for label, mask in (("load", 1), ("mfma", 4), ("epilogue", 2)):
        # a partial mask accumulates garbage (unstaged LDS, unwritten
        # partials, NaN included) into ``grad``: timing only, and the
        # store-mode call before the cross-check below overwrites it
        res[f"hip_wrw_{label}"] = timeit(
            lambda: _C.conv1x1_wrw(xn, dyn, wpart, grad, True, chunks, mask))
        res[f"hip_fwd_stats_{label}"] = timeit(
            lambda: _C.conv1x1_fwd(xn, wt, yn, part, mask))
        res[f"hip_dgrad_{label}"] = timeit(
            lambda: _C.conv1x1_dgrad(dyn, wt, dxn, mask))
    # numerics cross-check at this exact shape (the masked runs above left
    # garbage in y / dx: run the full kernels again first)
    _C.conv1x1_fwd(xn, wt, yn, part)
    _C.conv1x1_dgrad(dyn, wt, dxn)
    res["fwd_rel_vs_miopen"] = round(
        ((y.float() - ref.float()).norm() / ref.float().norm()).item(), 5)
    dref = mio_dgrad().float()
    res["dgrad_rel_vs_miopen"] = round(
        ((dx.float() - dref).norm() / dref.norm()).item(), 5)
    wref = torch.ops.aten.convolution_backward(
        dy, x, wt, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
        [False, True, False])[1].float()
    _C.conv1x1_wrw(xn, dyn, wpart, grad, False, chunks)
    res["wrw_rel_vs_miopen"] = round(
        ((grad.float() - wref).norm() / wref.norm()).item(), 5)
    # which of the two is off when they differ: both against fp64
    w64 = dyn.reshape(m, cout).double().t() @ xn.reshape(m, cin).double()
    for key, got in (("wrw_rel_vs_fp64", grad), ("miopen_wrw_rel_vs_fp64",
                                                 wref)):
        res[key] = round(((got.double().reshape(cout, cin) - w64).norm()
                          / w64.norm()).item(), 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=212)
    ap.add_argument("--chunks", type=int, default=0)
    ap.add_argument("--shapes", type=str, default="",
                    help="comma-separated indices into SHAPES (default all)")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = True
    g = torch.Generator().manual_seed(0)
    picked = [int(i) for i in args.shapes.split(",")] if args.shapes \
        else range(len(SHAPES))
    for cin, cout, h in (SHAPES[i] for i in picked):
        print(json.dumps(bench_shape(args.batch, cin, cout, h, g,
                                     args.chunks)), flush=True)


if __name__ == "__main__":
    main()
