"""3x3/s1/p1 weight-grad micro-benchmark: the padded-flat split-K MFMA kernel
of ops/csrc/conv3x3wrw.hip vs MIOpen on the four ResNet-18 shapes at batch
212, bf16 channels-last. One JSON line per shape; every timing is
``[median, min, max]`` in us over ``--rounds`` (default three) rounds, each
of which times every variant once in turn, so the variants alternate:

  miopen_wrw+add     aten.convolution_backward, mask [False, True, False],
                     plus the bf16 add into a preallocated grad
  hip_wrw            conv3x3_wrw + the reduce in accumulate mode
  hip_wrw_load / _mfma / _epilogue   phase_mask 1 / 4 / 2 alone (the reduce
                     launch runs in all three)
  hip_wrw_x0.25 ... x4   the chunk request forced to that multiple of the
                     default rule's count (``--sweep``)

plus the byte counts the shapes imply (operands once; the fp32 partials
written and read back; what the blocks pull through L2) and the relative
norm of the result against MIOpen's. ``--batch`` shrinks the batch (smoke
runs); ``--shapes`` picks shapes by index into SHAPES (default all)."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from mi355x_scale.ops import _C  # noqa: E402

# (C = Cin = Cout, H = W): ResNet-18 layer1..layer4
SHAPES = [(64, 56), (128, 28), (256, 14), (512, 7)]
SWEEP = [0.25, 0.5, 0.75, 1.5, 2.0, 4.0]


def timeit(fn, iters=30, warmup=8):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def bench_shape(n, c, h, g, rounds, sweep):
    dev, cl = "cuda", torch.channels_last

    def rand(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev) \
            .to(torch.bfloat16).to(memory_format=cl)

    x, dy = rand(n, c, h, h), rand(n, c, h, h)
    wt = rand(c, c, 3, 3, scale=(9 * c) ** -0.5)
    grad = torch.zeros_like(wt)
    dw = torch.empty_like(wt)
    xn, dyn = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    gn, dwn = grad.permute(0, 2, 3, 1), dw.permute(0, 2, 3, 1)
    nch = _C.conv3x3_wrw_nchunks(n, h, h, c)
    steps = -(-n * (h + 2) * (h + 2) // 32)

    def part_for(chunks):
        k = _C.conv3x3_wrw_nchunks(n, h, h, c, chunks)
        return torch.empty(k * 9 * c * c, dtype=torch.float32, device=dev)

    part = part_for(0)

    def mio_wrw():
        return torch.ops.aten.convolution_backward(
            dy, x, wt, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
            [False, True, False])[1]

    variants = {
        "miopen_wrw+add": lambda: grad.add_(mio_wrw()),
        "hip_wrw": lambda: _C.conv3x3_wrw(xn, dyn, part, gn, True),
    }
    for label, mask in (("load", 1), ("mfma", 4), ("epilogue", 2)):
        # a partial mask leaves garbage in grad: timing only
        variants[f"hip_wrw_{label}"] = \
            lambda mask=mask: _C.conv3x3_wrw(xn, dyn, part, gn, True, 0, mask)
    forced = {}
    if sweep:
        for f in SWEEP:
            req = max(1, min(steps, round(nch * f)))
            p = part_for(req)
            forced[f"x{f:g}"] = p.numel() // (9 * c * c)
            variants[f"hip_wrw_x{f:g}"] = \
                lambda p=p, req=req: _C.conv3x3_wrw(xn, dyn, p, gn, True, req)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timeit(fn))
    q = n * (h + 2) * (h + 2)
    res = {"shape": f"{c}@{h}", "batch": n, "chunks": nch,
           "forced_chunks": forced,
           "useful_q_share": round(h * h / (h + 2) ** 2, 3),
           # MB: each map once; partials written + read back; rows the
           # blocks load (every tile re-reads its chunk's rows of both
           # maps, plus a halo of 2W + 6 rows of X per block)
           "operands_mb": round(2 * n * h * h * c * 2 / 1e6, 1),
           "partials_mb": round(2 * nch * 9 * c * c * 4 / 1e6, 1),
           "block_loads_mb": round(
               (c // 64) ** 2 * 128 * (2 * q + nch * (2 * h + 6)) / 1e6, 1)}
    for k, t in times.items():
        res[k] = [round(v, 1) for v in (statistics.median(t), min(t), max(t))]
    ours, theirs = res["hip_wrw"], res["miopen_wrw+add"]
    res["verdict"] = ("faster" if ours[2] < theirs[1] else
                      "slower" if ours[1] > theirs[2] else "level")

    _C.conv3x3_wrw(xn, dyn, part, dwn)
    ref = mio_wrw().float()
    res["wrw_rel_vs_miopen"] = round(
        ((dw.float() - ref).norm() / ref.norm()).item(), 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=212)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", type=str, default="",
                    help="comma-separated indices into SHAPES (default all)")
    ap.add_argument("--sweep", action="store_true",
                    help="also time forced chunk counts, 0.25x-4x the default")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = True
    g = torch.Generator().manual_seed(0)
    picked = [int(i) for i in args.shapes.split(",")] if args.shapes \
        else range(len(SHAPES))
    for c, h in (SHAPES[i] for i in picked):
        print(json.dumps(bench_shape(args.batch, c, h, g, args.rounds,
                                     args.sweep)), flush=True)


if __name__ == "__main__":
    main()
