"""3x3/s2/p1 conv micro-benchmark: the MFMA kernels of ops/csrc/conv3x3s2.hip
vs MIOpen on the six ResNet stride-2 shapes at batch 212, bf16 channels-last.
One JSON line per shape; every timing is ``[median, min, max]`` in us over
``--rounds`` (default three) rounds, each of which times every variant once
in turn, so the variants alternate:

  miopen_fwd / miopen_fwd+reduce   F.conv2d, and that + bn_fwd_reduce
  hip_fwd / hip_fwd_stats          conv3x3_s2_fwd without / with BN partials
  miopen_dgrad / hip_dgrad         data-grad (ours includes the weight repack)
  hip_fwd_stats_load / _mfma / _epilogue   phase_mask 1 / 4 / 2 alone
  hip_dgrad_load / _mfma / _epilogue       the same for the data-grad

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

# (Cin, Cout, H = W of the input): ResNet-18/34 layer{2,3,4}[0].conv1, then
# ResNet-50 layer{2,3,4}[0].conv2
SHAPES = [(64, 128, 56), (128, 256, 28), (256, 512, 14),
          (128, 128, 56), (256, 256, 28), (512, 512, 14)]
_S2 = ([2, 2], [1, 1], [1, 1], False, [0, 0], 1)


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

    def rand(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev) \
            .to(torch.bfloat16).to(memory_format=cl)

    x, dy = rand(n, cin, h, h), rand(n, cout, ho, ho)
    wt = rand(cout, cin, 3, 3, scale=(9 * cin) ** -0.5)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    part = torch.empty(2 * cout * _C.conv3x3_s2_fwd_blocks(n, h, h),
                       dtype=torch.float32, device=dev)
    wflip = torch.empty(wt.numel(), dtype=torch.bfloat16, device=dev)
    xn, yn, wn = (t.permute(0, 2, 3, 1) for t in (x, y, wt))
    dyn, dxn = dy.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)

    def mio_fwd():
        return F.conv2d(x, wt, stride=2, padding=1)

    def mio_dgrad():
        return torch.ops.aten.convolution_backward(
            dy, x, wt, None, *_S2, [True, False, False])[0]

    variants = {
        "miopen_fwd": mio_fwd,
        "miopen_fwd+reduce": lambda: _C.bn_fwd_reduce(mio_fwd(), cout),
        "hip_fwd": lambda: _C.conv3x3_s2_fwd(xn, wn, yn),
        "hip_fwd_stats": lambda: _C.conv3x3_s2_fwd(xn, wn, yn, part),
        "miopen_dgrad": mio_dgrad,
        "hip_dgrad": lambda: _C.conv3x3_s2_dgrad(dyn, wn, wflip, dxn),
    }
    for label, mask in (("load", 1), ("mfma", 4), ("epilogue", 2)):
        # a partial mask leaves garbage in the outputs: timing only; the
        # cross-check below runs the full kernels again
        variants[f"hip_fwd_stats_{label}"] = \
            lambda mask=mask: _C.conv3x3_s2_fwd(xn, wn, yn, part, mask)
        variants[f"hip_dgrad_{label}"] = \
            lambda mask=mask: _C.conv3x3_s2_dgrad(dyn, wn, wflip, dxn, mask)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timeit(fn))
    res = {"shape": f"{cin}->{cout}@{h}", "batch": n,
           "useful_mfma_share": round(ho * ho / (ho + 1) ** 2, 3)}
    for k, t in times.items():
        res[k] = [round(v, 1) for v in (statistics.median(t), min(t), max(t))]

    def rel(got, ref):
        return round(((got.float() - ref.float()).norm()
                      / ref.float().norm()).item(), 5)

    _C.conv3x3_s2_fwd(xn, wn, yn, part)
    _C.conv3x3_s2_dgrad(dyn, wn, wflip, dxn)
    res["fwd_rel_vs_miopen"] = rel(y, mio_fwd())
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
    for cin, cout, h in (SHAPES[i] for i in picked):
        print(json.dumps(bench_shape(args.batch, cin, cout, h, g,
                                     args.rounds)), flush=True)


if __name__ == "__main__":
    main()
