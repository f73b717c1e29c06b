"""Padded-flat split-K 3x3 weight-grad (ops/csrc/conv3x3wrw.hip) against fp64.

Inputs are bf16 values from a seeded generator; the reference is fp64
``conv2d`` backward on THOSE values, computed on the CPU. Bound: relative L2
<= 2^-8 (one bf16 rounding of the result plus fp32 summation, the bound of
tests/test_stem_wrw_tr.py) and cosine > 0.9999. The partial scratch is
filled with NaN before every call, so a slot no block writes shows.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_scale.ops import conv3x3 as c3

BF16 = torch.bfloat16
REL, COS = 2.0 ** -8, 0.9999

# (N, C, H, W), the smallest at which each mechanism can go wrong
SHAPES = [
    (2, 64, 9, 9),     # 242 virtual pixels: a K-step spans three rows
    (3, 64, 5, 7),     # H != W; 63 pixels per image: a step straddles images
    (5, 64, 3, 1),     # W = 1
    (1, 64, 1, 1),     # Q = 9: less than one K-step
    (1, 64, 2, 64),    # widest band: ring capacity
    (2, 128, 6, 6),    # four tiles: tile indexing
    (1, 192, 4, 5),    # C a multiple of 64, not of 128
]
# chunk requests at 2 x 64 x 9 x 9 (8 K-steps): a short last chunk (3 ->
# 3 + 3 + 2 steps), a halo at every chunk start and a chunk boundary inside
# an image row (the maximum: one step per chunk)
CHUNKS = [1, 2, 3, 8]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """bf16 NCHW channels-last x and dy (CPU), and the fp64 weight-grad."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * c + 100 * h + 10 * w + n)
    x = torch.randn(n, c, h, w, generator=g).to(BF16)
    dy = torch.randn(n, c, h, w, generator=g).to(BF16)
    wt = torch.zeros(c, c, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wt, padding=1).backward(dy.double())
    return x, dy, wt.grad.detach()


def _gpu(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _wrw(xg, dyg, chunks=0, into=None):
    """One call of the binding on NaN-filled partials. ``into``: accumulate
    into that bf16 channels-last tensor; otherwise a fresh NaN-filled dw."""
    from mi355x_scale.ops import _C
    n, c, h, w = xg.shape
    nch = _C.conv3x3_wrw_nchunks(n, h, w, c, chunks)
    part = torch.full((nch * 9 * c * c,), float("nan"), dtype=torch.float32,
                      device="cuda")
    dw = into
    if dw is None:
        dw = torch.full((c, c, 3, 3), float("nan"), dtype=BF16,
                        device="cuda").contiguous(
                            memory_format=torch.channels_last)
    _C.conv3x3_wrw(xg.permute(0, 2, 3, 1), dyg.permute(0, 2, 3, 1), part,
                   dw.permute(0, 2, 3, 1), into is not None, chunks)
    return dw, nch


def _assert_close(dw, ref, what):
    got = dw.detach().cpu().double()
    assert torch.isfinite(got).all(), f"{what}: non-finite dW"
    rel = ((got - ref).norm() / ref.norm()).item()
    cos = F.cosine_similarity(got.reshape(-1), ref.reshape(-1), dim=0).item()
    print(f"{what}: rel L2 {rel:.3e} (bound {REL:.3e}), cos {cos:.7f}")
    assert rel <= REL, f"{what}: rel L2 {rel}"
    assert cos > COS, f"{what}: cos {cos}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_wrw_fp64(shape):
    x, dy, ref = _case(shape)
    dw, _ = _wrw(_gpu(x), _gpu(dy))
    _assert_close(dw, ref, str(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", CHUNKS)
def test_wrw_chunk_requests(chunks):
    shape = SHAPES[0]
    x, dy, ref = _case(shape)
    dw, nch = _wrw(_gpu(x), _gpu(dy), chunks)
    assert nch == chunks
    _assert_close(dw, ref, f"{shape} chunks={chunks}")


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [0, 3])
def test_wrw_all_ones_counts_valid_pixels(chunks):
    """x = dy = 1: dW[co][kh][kw][ci] is the number of output pixels whose
    tap (kh, kw) lands inside the map, exact in bf16. A border row leaking
    into either operand changes a count."""
    n, c, h, w = 2, 64, 9, 9
    ones = torch.ones(n, c, h, w, dtype=BF16)
    dw, _ = _wrw(_gpu(ones), _gpu(ones), chunks)
    want = torch.empty(3, 3)
    for kh in range(3):
        for kw in range(3):
            want[kh, kw] = n * (h - abs(kh - 1)) * (w - abs(kw - 1))
    assert want[1, 1] == 162 and want[0, 1] == 144 and want[0, 0] == 128
    assert torch.equal(dw.cpu().float(), want.expand(c, c, 3, 3))


@pytest.mark.gpu
def test_wrw_bit_reproducible():
    x, dy, _ = _case(SHAPES[5])
    xg, dyg = _gpu(x), _gpu(dy)
    a, _ = _wrw(xg, dyg)
    b, _ = _wrw(xg, dyg)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.gpu
def test_wrw_accumulate_is_a_bf16_tensor_add():
    shape = SHAPES[5]
    x, dy, _ = _case(shape)
    xg, dyg = _gpu(x), _gpu(dy)
    dw, _ = _wrw(xg, dyg)
    c = shape[1]
    g = torch.Generator().manual_seed(7)
    view = _gpu(torch.randn(c, c, 3, 3, generator=g).to(BF16))
    want = view + dw
    got, _ = _wrw(xg, dyg, into=view)
    assert got.data_ptr() == view.data_ptr()
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_wrw_captured_adds_into_grad_view(monkeypatch):
    """Under capture the reduce adds into the installed bf16 channels-last
    grad and backward returns None for the weight; with the zero fill inside
    the graph, replays give the eager gradient and do not pile up."""
    monkeypatch.setenv("MI355X_CONV_WRW", "1")
    shape = SHAPES[0]
    x, dy, ref = _case(shape)
    xg, dyg = _gpu(x), _gpu(dy)
    m = c3.Conv3x3(shape[1], shape[1]).cuda().to(BF16).to(
        memory_format=torch.channels_last)
    assert m._hip_ok(xg)
    m(xg).backward(dyg)  # eager: a fresh tensor
    eager = m.weight.grad.detach().clone()
    _assert_close(eager, ref, "eager")
    gview = torch.zeros_like(m.weight)
    m.weight.grad = gview
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        gview.fill_(0)
        m(xg).backward(dyg)
    assert m.weight.grad.data_ptr() == gview.data_ptr()
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _assert_close(gview, ref, f"replay {replay}")
        assert torch.equal(gview, eager)


def test_switches_are_tri_state(monkeypatch):
    table = {(64, 56, 56): 212}
    name = "MI355X_CONV_WRW"
    monkeypatch.delenv(name, raising=False)
    assert not c3._engaged(name, table, 64, 2, 9, 9)       # not in the table
    assert c3._engaged(name, table, 64, 212, 56, 56)
    assert c3._engaged(name, table, 64, 256, 56, 56)
    assert not c3._engaged(name, table, 64, 211, 56, 56)   # below the floor
    assert not c3._engaged(name, table, 128, 212, 56, 56)
    monkeypatch.setenv(name, "1")
    assert c3._engaged(name, table, 64, 2, 9, 9)
    assert c3._engaged(name, table, 64, 211, 56, 56)
    monkeypatch.setenv(name, "0")
    assert not c3._engaged(name, table, 64, 212, 56, 56)
    assert not c3._engaged(name, table, 64, 2, 9, 9)


def test_default_tables_respect_their_floor(monkeypatch):
    for name in ("MI355X_CONV3X3", "MI355X_CONV3X3_DGRAD", "MI355X_CONV_WRW"):
        monkeypatch.delenv(name, raising=False)
    for name, table in (("MI355X_CONV3X3", c3._FWD_TABLE),
                        ("MI355X_CONV_WRW", c3._WRW_TABLE)):
        assert not c3._engaged(name, table, 64, 2, 9, 9)
        for (c, h, w), floor in table.items():
            assert floor >= 1
            assert c3._engaged(name, table, c, floor, h, w)
            assert not c3._engaged(name, table, c, floor - 1, h, w)
