"""3x3/s1/p1 conv micro-benchmark: the MFMA kernels of ops/csrc/conv3x3.hip
vs MIOpen on the four ResNet-18 shapes at batch 212, bf16 channels-last.
One JSON line per shape; every timing is ``[median, min, max]`` in us over
``--rounds`` (default three) rounds, each of which times every variant once
in turn, so the variants alternate:

  miopen_fwd / miopen_fwd+reduce   F.conv2d, and that + bn_fwd_reduce
  hip_fwd / hip_fwd_stats          conv3x3_fwd without / with BN partials
  miopen_dgrad / hip_dgrad         data-grad (ours includes the weight repack)
  hip_fwd_stats_load / _mfma / _epilogue   phase_mask 1 / 4 / 2 alone

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

# (C = Cin = Cout, H = W): ResNet-18 layer1..layer4
SHAPES = [(64, 56), (128, 28), (256, 14), (512, 7)]


def timeit(fn, iters=30, warmup=8):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def bench_shape(n, c, h, g, rounds):
    dev, cl = "cuda", torch.channels_last

    def rand(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev) \
            .to(torch.bfloat16).to(memory_format=cl)

    x, dy = rand(n, c, h, h), rand(n, c, h, h)
    wt = rand(c, c, 3, 3, scale=(9 * c) ** -0.5)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    part = torch.empty(2 * c * _C.conv3x3_fwd_blocks(n, h, h),
                       dtype=torch.float32, device=dev)
    wflip = torch.empty(wt.numel(), dtype=torch.bfloat16, device=dev)
    xn, yn, wn = (t.permute(0, 2, 3, 1) for t in (x, y, wt))
    dyn, dxn = dy.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)

    def mio_dgrad():
        return torch.ops.aten.convolution_backward(
            dy, x, wt, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
            [True, False, False])[0]

    variants = {
        "miopen_fwd": lambda: F.conv2d(x, wt, padding=1),
        "miopen_fwd+reduce":
            lambda: _C.bn_fwd_reduce(F.conv2d(x, wt, padding=1), c),
        "hip_fwd": lambda: _C.conv3x3_fwd(xn, wn, yn),
        "hip_fwd_stats": lambda: _C.conv3x3_fwd(xn, wn, yn, part),
        "miopen_dgrad": mio_dgrad,
        "hip_dgrad": lambda: _C.conv3x3_dgrad(dyn, wn, wflip, dxn),
    }
    for label, mask in (("load", 1), ("mfma", 4), ("epilogue", 2)):
        # a partial mask leaves garbage in the outputs: timing only; the
        # cross-check below runs the full kernels again
        variants[f"hip_fwd_stats_{label}"] = \
            lambda mask=mask: _C.conv3x3_fwd(xn, wn, yn, part, mask)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timeit(fn))
    res = {"shape": f"{c}@{h}", "batch": n,
           "useful_mfma_share": round(h * h / (h + 2) ** 2, 3)}
    for k, t in times.items():
        res[k] = [round(v, 1) for v in (statistics.median(t), min(t), max(t))]

    def rel(got, ref):
        return round(((got.float() - ref.float()).norm()
                      / ref.float().norm()).item(), 5)

    _C.conv3x3_fwd(xn, wn, yn, part)
    _C.conv3x3_dgrad(dyn, wn, wflip, dxn)
    res["fwd_rel_vs_miopen"] = rel(y, F.conv2d(x, wt, padding=1))
    res["dgrad_rel_vs_miopen"] = rel(dx, mio_dgrad())
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
    for c, h in (SHAPES[i] for i in picked):
        print(json.dumps(bench_shape(args.batch, c, h, g, args.rounds)),
              flush=True)


if __name__ == "__main__":
    main()
