"""Stride-2 pointwise conv micro-benchmark: the S2 MFMA kernels (ops/csrc/
conv1x1.hip) vs MIOpen on the six downsample projections of ResNet-18/34
and ResNet-50 at batch 212, bf16 channels-last. One JSON line per shape;
every timing is ``[median, min, max]`` in us over ``--rounds`` (default
three) rounds, each of which times every variant once in turn, so the
variants alternate:

  miopen_fwd / miopen_fwd+reduce   F.conv2d(stride=2), and that + bn_fwd_reduce
  hip_fwd / hip_fwd_stats          conv1x1_s2_fwd without / with BN partials
  miopen_dgrad / hip_dgrad         data-grad (ours writes the zeros as well)
  miopen_wrw                       MIOpen weight-grad + the bf16 add into a
                                   preallocated grad tensor (AccumulateGrad)
  hip_wrw                          conv1x1_s2_wrw, accumulate mode (both
                                   launches)
  hip_*_load / _mfma / _epilogue   phase_mask 1 / 4 / 2 alone (the
                                   weight-grad figures include the reduce)

and the relative norm of each kernel's result against MIOpen's.
``--batch`` shrinks the batch (smoke runs); ``--shapes`` picks shapes by
index into SHAPES (default all)."""
import argparse
import json
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from mi355x_scale.ops import _C  # noqa: E402

# (Cin, Cout, H of the input map): ResNet-18/34, then ResNet-50
SHAPES = [(64, 128, 56), (128, 256, 28), (256, 512, 14),
          (256, 512, 56), (512, 1024, 28), (1024, 2048, 14)]


def timeit(fn, iters=30, warmup=8):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def bench_shape(n, cin, cout, h, g, rounds):
    dev, cl = "cuda", torch.channels_last
    ho = (h + 1) // 2
    x = torch.randn(n, cin, h, h, generator=g).to(dev).to(torch.bfloat16) \
        .to(memory_format=cl)
    wt = (torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5).to(dev) \
        .to(torch.bfloat16)
    y = torch.empty((n, cout, ho, ho), dtype=torch.bfloat16, device=dev,
                    memory_format=cl)
    dy = torch.randn(n, cout, ho, ho, generator=g).to(dev) \
        .to(torch.bfloat16).to(memory_format=cl)
    dx = torch.empty_like(x)
    m = n * ho * ho
    part = torch.empty(2 * cout * _C.conv1x1_fwd_blocks(m),
                       dtype=torch.float32, device=dev)
    xn, yn = x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)
    dyn, dxn = dy.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)
    grad = torch.zeros_like(wt)
    nch = _C.conv1x1_wrw_nchunks(m, cin, cout)
    wpart = torch.empty(nch * cout * cin, dtype=torch.float32, device=dev)

    def mio_bwd(mask):
        return torch.ops.aten.convolution_backward(
            dy, x, wt, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1, mask)

    variants = {
        "miopen_fwd": lambda: F.conv2d(x, wt, stride=2),
        "miopen_fwd+reduce":
            lambda: _C.bn_fwd_reduce(F.conv2d(x, wt, stride=2), cout),
        "hip_fwd": lambda: _C.conv1x1_s2_fwd(xn, wt, yn),
        "hip_fwd_stats": lambda: _C.conv1x1_s2_fwd(xn, wt, yn, part),
        "miopen_dgrad": lambda: mio_bwd([True, False, False])[0],
        "hip_dgrad": lambda: _C.conv1x1_s2_dgrad(dyn, wt, dxn),
        "miopen_wrw": lambda: grad.add_(mio_bwd([False, True, False])[1]),
        "hip_wrw": lambda: _C.conv1x1_s2_wrw(xn, dyn, wpart, grad, True),
    }
    for label, mask in (("load", 1), ("mfma", 4), ("epilogue", 2)):
        # a partial mask leaves garbage in the outputs and in ``grad``:
        # timing only; the cross-check below runs the full kernels again
        variants[f"hip_fwd_stats_{label}"] = \
            lambda mask=mask: _C.conv1x1_s2_fwd(xn, wt, yn, part, mask)
        variants[f"hip_dgrad_{label}"] = \
            lambda mask=mask: _C.conv1x1_s2_dgrad(dyn, wt, dxn, mask)
        variants[f"hip_wrw_{label}"] = \
            lambda mask=mask: _C.conv1x1_s2_wrw(xn, dyn, wpart, grad, True, 0,
                                                mask)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timeit(fn))
    res = {"shape": f"{cin}->{cout}@{h}", "batch": n, "M'": m,
           "wrw_chunks": nch}
    for k, t in times.items():
        res[k] = [round(v, 1) for v in (statistics.median(t), min(t), max(t))]

    def rel(got, ref):
        return round(((got.float() - ref.float()).norm()
                      / ref.float().norm()).item(), 5)

    _C.conv1x1_s2_fwd(xn, wt, yn, part)
    _C.conv1x1_s2_dgrad(dyn, wt, dxn)
    _C.conv1x1_s2_wrw(xn, dyn, wpart, grad, False)
    res["fwd_rel_vs_miopen"] = rel(y, F.conv2d(x, wt, stride=2))
    res["dgrad_rel_vs_miopen"] = rel(dx, mio_bwd([True, False, False])[0])
    res["wrw_rel_vs_miopen"] = rel(grad, mio_bwd([False, True, False])[1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=212)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", type=str, default="",
                    help="comma-separated indices into SHAPES (default all)")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = True
    g = torch.Generator().manual_seed(0)
    picked = [int(i) for i in args.shapes.split(",")] if args.shapes \
        else range(len(SHAPES))
    for cin, cout, h in (SHAPES[i] for i in picked):
        print(json.dumps(bench_shape(args.batch, cin, cout, h, g,
                                     args.rounds)), flush=True)


if __name__ == "__main__":
    main()
