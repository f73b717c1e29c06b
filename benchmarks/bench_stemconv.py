"""Stem conv micro-benchmark: MFMA kernel vs MIOpen at the flagship
shape ([212,3,224,224] bf16 channels-last, 7x7 s2 p3, 3->64)."""
import json
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])

from mi355x_scale.ops.stemconv import _StemConvFn  # noqa: E402


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def main():
    torch.backends.cudnn.benchmark = True
    dev = "cuda"
    n, h, w = 212, 224, 224
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, 3, h, w, generator=g).to(dev).to(torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    wt = (torch.randn(64, 3, 7, 7, generator=g) * 0.05).to(dev) \
        .to(torch.bfloat16).to(memory_format=torch.channels_last)
    x.requires_grad_(False)

    # --- MIOpen paths
    wt_m = wt.clone().requires_grad_(True)
    t_mio_fwd = timeit(lambda: F.conv2d(x, wt_m, None, 2, 3))
    out = F.conv2d(x, wt_m, None, 2, 3)
    dy = torch.randn(out.shape, generator=g).to(dev).to(torch.bfloat16) \
        .to(memory_format=torch.channels_last)

    def mio_wrw():
        wg = torch.ops.aten.convolution_backward(
            dy, x, wt_m, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
            [False, True, False])[1]
        return wg
    t_mio_wrw = timeit(mio_wrw)

    # --- MFMA paths
    t_fwd = timeit(lambda: _StemConvFn.apply(x, wt))

    wt_g = wt.clone().requires_grad_(True)
    out2 = _StemConvFn.apply(x, wt_g)

    def mfma_wrw():
        wt_g.grad = None
        out2.backward(dy, retain_graph=True)
    t_wrw = timeit(mfma_wrw)

    # --- forward phase split, both kernels: phase_mask 1 = band staging
    # only, 4 = MFMA + epilogue only (on an unstaged band), 7 = all.
    # "rows1" is the one-row-per-block kernel, "fused" the multi-row
    # kernel with wide stores and BN partial sums (pad-weights launch
    # included in every figure, ~2 us).
    from mi355x_scale.ops import _C
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    o_nhwc = torch.empty(n, ho, wo, 64, dtype=torch.bfloat16, device=dev)
    wp = torch.empty(64 * 160, dtype=torch.bfloat16, device=dev)
    part = torch.empty(2 * 64 * _C.stem_fwd_blocks(n, ho),
                       dtype=torch.float32, device=dev)
    xn, wn = x.permute(0, 2, 3, 1), wt.permute(0, 2, 3, 1)
    phases = {}
    for name, p in (("rows1", None), ("fused", part)):
        phases[name] = {
            label: round(timeit(
                lambda: _C.stem_conv_fwd(xn, wn, o_nhwc, wp, mask, p)), 1)
            for label, mask in (("stage", 1), ("mfma_store", 4), ("all", 7))}
    # what the BN statistics of the stem map cost on top of each
    out_cl = _StemConvFn.apply(x, wt)
    mean = torch.empty(64, dtype=torch.float32, device=dev)
    invstd = torch.empty(64, dtype=torch.float32, device=dev)
    rm, rv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    rows = n * ho * wo

    def stats_separate():
        _C.bn_fwd_finalize(_C.bn_fwd_reduce(out_cl, 64), mean, invstd, rm,
                           rv, 0.1, 1e-5, rows, 64, True)
    t_stats_sep = timeit(stats_separate)
    _C.stem_conv_fwd(xn, wn, o_nhwc, wp, 7, part)
    t_stats_fin = timeit(lambda: _C.bn_fwd_finalize(
        part, mean, invstd, rm, rv, 0.1, 1e-5, rows, 64, True))

    # --- wrw phase split, both kernels ("tr" = transposed LDS reads,
    # "gather" = element gather): phase_mask 1 = band staging, 2 = dy
    # staging, 4 = MFMA (on whatever the enabled stages left in LDS).
    # Memset and cast launches are included in every figure (~10 us).
    dyn = dy.permute(0, 2, 3, 1)
    dw_out = torch.empty((64, 3, 7, 7), dtype=torch.bfloat16, device=dev,
                         memory_format=torch.channels_last).permute(0, 2, 3, 1)
    wscr = torch.empty(_C.stem_wrw_scratch(), dtype=torch.float32,
                       device=dev)
    wrw_phases = {}
    for name, tr in (("tr", 1), ("gather", 0)):
        wrw_phases[name] = {
            label: round(timeit(
                lambda: _C.stem_conv_wrw(xn, dyn, wscr, dw_out, mask, tr)), 1)
            for label, mask in (("band", 1), ("dy", 2), ("band+dy", 3),
                                ("mfma", 4), ("all", 7))}

    # numerics cross-check at this exact shape
    ref = F.conv2d(x.float(), wt.float(), None, 2, 3)
    got = _StemConvFn.apply(x, wt).float()
    rel = ((got - ref).norm() / ref.norm()).item()

    print(json.dumps({
        "shape": [n, 3, h, w],
        "fwd_us": {"miopen": round(t_mio_fwd, 1), "mfma": round(t_fwd, 1),
                   "speedup": round(t_mio_fwd / t_fwd, 2)},
        "wrw_us": {"miopen": round(t_mio_wrw, 1), "mfma": round(t_wrw, 1),
                   "speedup": round(t_mio_wrw / t_wrw, 2)},
        "fwd_phase_us": phases,
        "wrw_phase_us": wrw_phases,
        "stem_bn_stats_us": {"reduce+finalize": round(t_stats_sep, 1),
                             "finalize_on_conv_partial":
                                 round(t_stats_fin, 1)},
        "fwd_rel_err_vs_fp32": round(rel, 5),
    }))


if __name__ == "__main__":
    main()
