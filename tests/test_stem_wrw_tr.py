"""Stem conv weight-grad on transposed LDS reads (``stem_conv_wrw_kernel``
in ops/csrc/stemconv.hip) and the element-gather kernel it replaced
(``MI355X_STEM_WRW_TR=0``).

The shapes leave the one-row-per-block regime of tests/test_stemconv.py
(``rows_per_block`` is 1 below 768 output rows): ring band, register
prefetch of dy and (row length a multiple of 4 elements, as in the
flagship) of the two new band rows with their ring-slot writes, blocks
that cross an image boundary, partial and empty 32-px slices, the scalar
staging path.

Reference: the fp32 weight gradient of ``F.conv2d`` (CPU) on the
bf16-rounded x and dy widened to fp32. Beyond fp32 accumulation the only
rounding is the final bf16 cast, at most 2^-9 relative per element, so the
relative L2 bound is 2^-8 (2x margin) and the cosine bound 0.9999. The two
kernels are compared with each other under the same bound (not bitwise:
atomics and K order differ).
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from mi355x_scale.ops.stemconv import StemConv2d

REL_BOUND = 2.0 ** -8
COS_BOUND = 0.9999

# name -> (N, H, W); what each exercises is in the ids below
CASES = {
    "one_full_slice": (2, 64, 64),      # WO=32: one full slice, 1 row/block
    "partial_slice": (2, 64, 70),       # WO=35: partial 2nd slice, 3-4 empty
    "odd_size": (3, 75, 53),            # row length % 4 != 0: scalar staging;
                                        # WO=27 < 32; top/bottom padding rows
    "full_width": (1, 16, 256),         # WO=128: all four slices, last px
    "multi_row_blocks": (50, 62, 70),   # 1550 rows -> 3 rows/block, 517
                                        # blocks; HO=31: blocks cross images,
                                        # last block short. Row length 210:
                                        # the SCALAR ring staging
    "multi_row_vector": (50, 62, 72),   # same rows and blocks, WO=36, row
                                        # length 216 = 54 8-byte chunks: the
                                        # register-prefetched band rows and
                                        # their ring writes to both images;
                                        # the last output row's new input
                                        # rows (62, 63) lie beyond H
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, dy) bf16 NCHW on the CPU and the fp32 reference dw; computed once
    per case and never modified."""
    n, h, w = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.randn(n, 3, h, w, generator=g).to(torch.bfloat16)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = torch.randn(n, 64, ho, wo, generator=g).to(torch.bfloat16)
    ref = torch.nn.grad.conv2d_weight(x.float(), (64, 3, 7, 7), dy.float(),
                                      stride=2, padding=3)
    return x, dy, ref


def _wrw(x, dy, tr=-1, return_scratch=False):
    """dw (fp32, [64,3,7,7], on the CPU) from ``_C.stem_conv_wrw``; with
    ``tr`` = -1 which kernel runs is MI355X_STEM_WRW_TR's choice at this
    call, 0 / 1 name it."""
    from mi355x_scale.ops import _C
    xb = x.cuda().contiguous(memory_format=torch.channels_last)
    dyb = dy.cuda().contiguous(memory_format=torch.channels_last)
    dw = torch.empty((64, 3, 7, 7), dtype=torch.bfloat16, device="cuda",
                     memory_format=torch.channels_last)
    scratch = torch.empty(_C.stem_wrw_scratch(), dtype=torch.float32,
                          device="cuda")
    _C.stem_conv_wrw(xb.permute(0, 2, 3, 1), dyb.permute(0, 2, 3, 1),
                     scratch, dw.permute(0, 2, 3, 1), 7, tr)
    torch.cuda.synchronize()
    if return_scratch:
        return dw.float().cpu(), scratch.cpu()
    return dw.float().cpu()


def _rel_cos(got, want):
    rel = ((got - want).norm() / want.norm()).item()
    cos = F.cosine_similarity(got.reshape(-1).double(),
                              want.reshape(-1).double(), dim=0).item()
    return rel, cos


def test_references_are_well_conditioned():
    """No case's reference is a near-cancellation: every dw has a norm far
    from zero relative to its terms (|x|,|dy| ~ 1, K = N*HO*WO terms)."""
    for name, (n, h, w) in CASES.items():
        _, dy, ref = _case(name)
        k = dy.shape[0] * dy.shape[2] * dy.shape[3]
        rms = ref.pow(2).mean().sqrt().item()
        assert torch.isfinite(ref).all()
        assert rms > 0.25 * k ** 0.5, (name, rms, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wrw_both_kernels_match_reference_and_each_other(name, monkeypatch):
    x, dy, ref = _case(name)
    got = {}
    for label, env in (("tr", "1"), ("gather", "0")):
        monkeypatch.setenv("MI355X_STEM_WRW_TR", env)
        got[label] = _wrw(x, dy)
    figures = {label: _rel_cos(g, ref) for label, g in got.items()}
    figures["tr_vs_gather"] = _rel_cos(got["tr"], got["gather"])
    print(name, {k: (f"{r:.3e}", f"{c:.7f}") for k, (r, c) in figures.items()})
    for label, (rel, cos) in figures.items():
        assert torch.isfinite(torch.tensor(rel)), (name, label)
        assert rel < REL_BOUND, f"{name} {label}: rel L2 {rel}"
        assert cos > COS_BOUND, f"{name} {label}: cosine {cos}"


def _ran_transposed_read_kernel(scratch):
    """Which kernel filled the fp32 scratch. The launcher zeroes all of it;
    the gather kernel accumulates into a [64][160] tile at its start and
    leaves the rest zero, the transposed-read kernel fills [64][176] (its
    rows 58..63 lie in that rest and hold sums of ~N*HO*WO random terms)."""
    return bool((scratch[64 * 160:] != 0).any())


@pytest.mark.gpu
def test_switch_is_read_per_call_and_argument_overrides_it(monkeypatch):
    """Unset and "1" run the transposed-read kernel, "0" the gather kernel,
    read at each call; an explicit ``tr`` argument wins over the variable.
    Every result is within the bound."""
    x, dy, ref = _case("partial_slice")
    runs = []  # (environment value or None, tr argument, expected kernel)
    for env, tr, want_tr in ((None, -1, True), ("0", -1, False),
                             ("1", -1, True), ("0", 1, True),
                             ("1", 0, False), (None, -1, True)):
        if env is None:
            monkeypatch.delenv("MI355X_STEM_WRW_TR", raising=False)
        else:
            monkeypatch.setenv("MI355X_STEM_WRW_TR", env)
        got, scratch = _wrw(x, dy, tr, return_scratch=True)
        rel, cos = _rel_cos(got, ref)
        runs.append((env, tr, want_tr, _ran_transposed_read_kernel(scratch),
                     rel, cos))
    print(runs)
    for env, tr, want_tr, ran_tr, rel, cos in runs:
        assert ran_tr == want_tr, (env, tr)
        assert rel < REL_BOUND and cos > COS_BOUND, (env, tr, rel, cos)


@pytest.mark.gpu
def test_width_beyond_128_output_px_falls_back_to_conv2d():
    """W=258 gives WO=129, one more than the kernels' row cap: the module
    must take F.conv2d (W in 257..262 used to pass the gate), W=256 must
    still take the HIP path."""
    m = StemConv2d().to("cuda").to(torch.bfloat16).to(
        memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(7)
    mk = lambda w: torch.randn(1, 3, 16, w, generator=g).cuda().to(
        torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x = mk(258)
    assert not m._hip_ok(x)
    assert m._hip_ok(mk(256))
    out = m(x)
    want = F.conv2d(x, m.weight, None, 2, 3)
    assert out.shape == (1, 64, 8, 129)
    rel, cos = _rel_cos(out.float().cpu(), want.float().cpu())
    assert rel < REL_BOUND and cos > COS_BOUND, (rel, cos)
    dy = torch.randn(out.shape, generator=g).cuda().to(torch.bfloat16)
    out.backward(dy)
    ref = torch.nn.grad.conv2d_weight(x.float().cpu(), (64, 3, 7, 7),
                                      dy.float().cpu(), stride=2, padding=3)
    rel, cos = _rel_cos(m.weight.grad.float().cpu(), ref)
    assert rel < REL_BOUND and cos > COS_BOUND, (rel, cos)


@pytest.mark.gpu
def test_graph_replay_matches_eager_gradient(monkeypatch):
    """Capture StemConv2d fwd+bwd once, replay three times: finite results
    and a weight gradient within the bound of the eager run's."""
    monkeypatch.delenv("MI355X_STEM_WRW_TR", raising=False)
    m = StemConv2d().to("cuda").to(torch.bfloat16).to(
        memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 64, 70, generator=g).cuda().to(torch.bfloat16).to(
        memory_format=torch.channels_last)
    dy = torch.randn(4, 64, 32, 35, generator=g).cuda().to(
        torch.bfloat16).contiguous(memory_format=torch.channels_last)
    for _ in range(2):  # warmup; the second is the eager reference
        m.weight.grad = None
        m(x).backward(dy)
    torch.cuda.synchronize()
    eager = m.weight.grad.float().cpu()
    m.weight.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        y = m(x)
        y.backward(dy)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    got = m.weight.grad.float().cpu()
    assert torch.isfinite(got).all()
    rel, cos = _rel_cos(got, eager)
    print("graph vs eager", rel, cos)
    assert rel < REL_BOUND and cos > COS_BOUND, (rel, cos)
