"""Both fused Adam kernels against a float64 reference of one step.

``adam_step_kernel`` (fp32) and ``adam_step_mixed_kernel`` (bf16
gradients and bf16 working parameters for the first ``nb`` elements)
are called through their raw bindings, so that ``n`` and ``nb`` can be
set to every size at which the kernels take another path: the float4
groups, the scalar tail, the group that straddles ``nb``, the fp32
segment that goes scalar when ``nb % 4 != 0``, and the grid-stride
sweeps past 2080 blocks x 1024 elements.

The reference is one Adam step in float64 (``_adam_ref64``); the
per-element bounds of ``_check_adam`` count the float32 roundings in the
kernel's expression chain, with eps = 2**-24:

    |m - m'| <= 4 eps (b1 |m0| + (1 - b1)(|g| + wd |p|))
    |v - v'| <= 8 eps v'
    |p - p'| <= eps |p| + |u| (8 eps + d1 + d2 / 2),
               di = 2 eps bi^t / (1 - bi^t)

The d terms are the only place where ``powf`` enters; they allow it
2 ulp. ``test_checker_accepts_emulation_rejects_wrong_variants`` shows
on the CPU that a float32 emulation of the kernel's operation order
stays inside these bounds and that five plausible wrong optimizers do
not; ``test_emulation_passes_on_every_gpu_test_input`` does the first on
the very inputs of the GPU tests, and
``test_p_bound_is_missed_only_where_m_cancels`` records the one thing the
p bound has no term for.

Worst ratios seen on an MI355X (both kernels, all sizes; the tests print
them): t = 1: m 0.43, v 0.45, p 0.92; t = 2: m 0.66, v 0.57, p 0.99;
t = 1000: m 0.60, v 0.46, p 0.99. The p figures are the emulation's to
three digits (0.924, 0.993, 0.987), so ``powf`` is within its allowance
at every t tested; m and v come out a little below the emulation's, as
the compiler fuses their last multiply and add.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from mi355x_scale.train.flat_adam import FlatAdam

EPS24 = 2.0 ** -24
B1, B2 = 0.9, 0.999
GUARD = 64          # sentinel elements before and after each payload
SENTINEL = -7.25    # exact in bf16 and fp32
SWEEP = 2080 * 1024  # elements one grid sweep of either kernel covers
N_LARGE = 2 * SWEEP + 5 * 1024 + 3  # 4,264,963: third sweep partial + tail


def _f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------ reference
def _adam_ref64(p, g, m, v, t, lr, b1, b2, eps, wd):
    """One Adam step (L2 weight decay) in float64. The hyperparameters
    are rounded to float32 first, as the binding casts them to float.
    Returns p', m', v' and the update u = p - p'."""
    lr, b1, b2, eps, wd = (_f32(x) for x in (lr, b1, b2, eps, wd))
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    grad = g + wd * p
    m1 = b1 * m + (1.0 - b1) * grad
    v1 = b2 * v + (1.0 - b2) * grad * grad
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    u = (lr / bc1) * m1 / (np.sqrt(v1 / bc2) + eps)
    return p - u, m1, v1, u


def _ratio(err, bound):
    """err / bound per element; 0 where err is 0, inf where a non-zero
    error meets a zero bound or the value is not finite."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return np.nan_to_num(r, nan=np.inf, posinf=np.inf)


def _adam_ratios(got_p, got_m, got_v, ref, t, p, g, m, v, b1, b2, wd,
                 mask=None):
    """Worst ratio of the error in m, v and p to its bound, and whether
    every element with no gradient and no history kept its bits."""
    b1, b2, wd = _f32(b1), _f32(b2), _f32(wd)
    p1, m1, v1, u = ref
    p64, g64, m64 = (np.asarray(a, dtype=np.float64) for a in (p, g, m))
    bound_m = 4 * EPS24 * (b1 * np.abs(m64)
                           + (1 - b1) * (np.abs(g64) + wd * np.abs(p64)))
    bound_v = 8 * EPS24 * v1
    d1 = 2 * EPS24 * b1 ** t / (1 - b1 ** t)
    d2 = 2 * EPS24 * b2 ** t / (1 - b2 ** t)
    bound_p = EPS24 * np.abs(p64) + np.abs(u) * (8 * EPS24 + d1 + d2 / 2)
    r_m = _ratio(np.abs(np.asarray(got_m, np.float64) - m1), bound_m)
    r_v = _ratio(np.abs(np.asarray(got_v, np.float64) - v1), bound_v)
    r_p = _ratio(np.abs(np.asarray(got_p, np.float64) - p1), bound_p)
    # no gradient, no history, nothing decayed: the update is 0 / eps
    # and p keeps its bits
    still = ((np.asarray(g) == 0) & (np.asarray(m) == 0)
             & (np.asarray(v) == 0))
    if wd != 0.0:
        still &= np.asarray(p) == 0
    same = (np.asarray(got_p, np.float32).view(np.uint32)
            == np.asarray(p, np.float32).view(np.uint32))
    if mask is not None:
        r_m, r_v, r_p = r_m[mask], r_v[mask], r_p[mask]
        still = still & mask
    worst = tuple(float(r.max()) if r.size else 0.0
                  for r in (r_m, r_v, r_p))
    return worst, bool(same[still].all())


def _check_adam(got_p, got_m, got_v, ref, t, p, g, m, v, b1, b2, wd,
                mask=None, tag=""):
    worst, still_ok = _adam_ratios(got_p, got_m, got_v, ref, t, p, g, m, v,
                                   b1, b2, wd, mask)
    assert still_ok, f"{tag}: p changed where g = m0 = v0 = 0"
    assert worst[0] <= 1.0, f"{tag}: m at {worst[0]:.3g} of its bound"
    assert worst[1] <= 1.0, f"{tag}: v at {worst[1]:.3g} of its bound"
    assert worst[2] <= 1.0, f"{tag}: p at {worst[2]:.3g} of its bound"
    return worst


# ------------------------------------------------------------- data generator
def _make_data(n, t, seed):
    """p ~ N(0, 0.05) with a few entries of magnitude 10; |g| log-uniform
    over 1e-8..1e2 with random sign and about 1 % exact zeros, some of
    them where m0 = v0 = 0 too; m0 ~ 1e-2 N, v0 = (1e-2 N)^2, both zero
    at t = 1. One zero-gradient, zero-history element is the last one, so
    it lands in the scalar tail when there is one."""
    rng = np.random.default_rng(seed)
    p = (0.05 * rng.standard_normal(n)).astype(np.float32)
    g = (10.0 ** rng.uniform(-8.0, 2.0, n)
         * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    m0 = (1e-2 * rng.standard_normal(n)).astype(np.float32)
    v0 = ((1e-2 * rng.standard_normal(n)) ** 2).astype(np.float32)
    big = rng.random(n) < 0.004
    zero_g = rng.random(n) < 0.01
    cold = zero_g & (rng.random(n) < 0.5)
    if n >= 3:
        big[n // 3] = True
        zero_g[n - 1] = cold[n - 1] = True
    if n >= 8:
        zero_g[2] = True
        zero_g[5] = cold[5] = True
    p[big] = np.where(p[big] < 0, -10.0, 10.0).astype(np.float32)
    g[zero_g] = 0.0
    m0[cold] = 0.0
    v0[cold] = 0.0
    if t == 1:
        m0[:] = 0.0
        v0[:] = 0.0
    return p, g, m0, v0


def _round_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x)).bfloat16()


def _mixed_inputs(n, nb, t, seed, poison=()):
    """The generator's data as adam_step_mixed reads it: the first nb
    gradients rounded to bf16. Returns p, g (what the kernel reads, as
    float32), m0, v0 and the two gradient buffers."""
    p, g, m0, v0 = _make_data(n, t, seed)
    for i, val in poison:
        g[i] = val
    gb = _round_bf16(g[:nb])
    gf = torch.from_numpy(g[nb:].copy())
    g = np.concatenate([gb.float().numpy(), g[nb:]])
    return p, g, m0, v0, gb, gf


# ------------------------------------------------- the cases of the GPU tests
# (t, lr, eps, wd, seed) per size; the CPU emulation test walks the same
# lists, so what it accepts is what the kernels are then given.
FP32_SMALL_N = [1, 3, 4, 5, 1023, 1024, 1027]
HP_CONFIGS = ((1e-3, 1e-8), (1e-5, 1e-8), (1e-3, 1e-3))  # (lr, eps)
FP32_LARGE = (2, 1e-3, 1e-8, 0.01, 77)
MIXED_SMALL = [(1, 0), (1, 1), (3, 3), (4, 4), (5, 4), (5, 5), (8, 4),
               (7, 3),
               (1031, 516),                              # aligned, tail 3
               (1029, 513), (1030, 514), (1031, 515),    # misaligned
               (1024, 1024),                             # empty gf
               (1024, 0)]                                # empty gb, pb
MIXED_LARGE_NB = [SWEEP, SWEEP + 2]
MIXED_LARGE = (2, 1e-3, 1e-8, 0.01, 78)


def _fp32_cases(n):
    for t in (1, 2, 1000):
        for wd in (0.0, 0.01):
            for lr, eps in HP_CONFIGS:
                yield t, lr, eps, wd, 1000 * n + t


def _mixed_cases(n, nb):
    for t in (1, 2, 1000):
        for lr, eps, wd in ((1e-3, 1e-8, 0.0), (1e-5, 1e-8, 0.01),
                            (1e-3, 1e-3, 0.01)):
            yield t, lr, eps, wd, 100_000 + 1000 * n + 10 * nb + t


def _print_worst(name, worst_by_t):
    for t, w in sorted(worst_by_t.items()):
        print(f"{name} t={t}: m={w[0]:.3g} v={w[1]:.3g} p={w[2]:.3g} "
              "of their bounds")


def _fold(worst_by_t, t, worst):
    old = worst_by_t.get(t, (0.0, 0.0, 0.0))
    worst_by_t[t] = tuple(max(a, b) for a, b in zip(old, worst))


# ---------------------------------------------------- float32 emulation (CPU)
def _fma32(a, b, c):
    """fmaf: a float32 product is exact in float64."""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    return (a * b + c).astype(np.float32)


def _adam_emul32(p, g, m, v, t, lr, b1, b2, eps, wd, variant=None):
    """The kernel's operation order in float32 numpy, one rounding per
    operation; ``variant`` picks one of the wrong optimizers that the
    checker has to reject.

    ``g + wd * p`` is the one place where the order of roundings matters
    to the bounds. hipcc contracts it to a single fma (its default,
    -ffp-contract=fast; the gfx950 code holds a v_pk_fma_f32 there), so
    the error of grad is relative to grad itself. Rounded in two steps,
    wd * p leaves eps * wd * |p| behind even where g cancels it, and at
    t = 1 (v0 = 0) v = (1 - b2) grad^2 then misses 8 eps v' by any
    factor: 6.3 of the bound at n = 1031, 1.3e4 at n = 400000 here.
    The other contractions the compiler makes only remove roundings."""
    f = np.float32
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    one = f(1.0)
    tb = t - 1 if variant == "t_minus_1" else t
    bc1 = one - f(np.float64(b1) ** tb)      # powf, correctly rounded
    bc2 = one - f(np.float64(b2) ** tb)
    if variant == "no_bc2":
        bc2 = one
    step_size = lr / bc1
    grad = g if variant == "decoupled_wd" else _fma32(wd, p, g)
    bm = b2 if variant == "m_beta2" else b1
    m1 = bm * m + (one - bm) * grad
    v1 = b2 * v + (one - b2) * grad * grad
    if variant == "eps_in_sqrt":
        denom = np.sqrt(v1 / bc2 + eps)
    else:
        denom = np.sqrt(v1 / bc2) + eps
    p1 = p - step_size * m1 / denom
    if variant == "decoupled_wd":
        p1 = p1 - lr * wd * p
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


WRONG_VARIANTS = ("t_minus_1", "eps_in_sqrt", "decoupled_wd", "no_bc2",
                  "m_beta2")


def test_ref64_rounds_hyperparameters_to_float32():
    p = np.array([0.5], np.float32)
    g = np.array([0.25], np.float32)
    z = np.zeros(1, np.float32)
    p1, m1, v1, u = _adam_ref64(p, g, z, z, 1, 1e-3, B1, B2, 1e-8, 0.0)
    b1, b2 = _f32(B1), _f32(B2)
    assert m1[0] == (1.0 - b1) * 0.25
    assert v1[0] == (1.0 - b2) * 0.25 * 0.25
    assert m1[0] != (1.0 - B1) * 0.25   # the double 0.9 is another number
    assert p1[0] == 0.5 - u[0]
    # at t = 1 the bias corrections cancel the (1 - beta) factors
    assert abs(u[0] / _f32(1e-3) - 1.0) < 1e-6


def test_checker_accepts_emulation_rejects_wrong_variants():
    """The float32 emulation of the kernel passes ``_check_adam`` at
    t in {1, 2, 1000, 100000}; each wrong variant is rejected wherever it
    differs from Adam at all, with the generator the GPU tests use, at
    the size most of them run."""
    n, lr, eps, wd = 1031, 1e-3, 1e-8, 0.01
    for t in (1, 2, 1000, 100000):
        p, g, m0, v0 = _make_data(n, t, seed=t)
        ref = _adam_ref64(p, g, m0, v0, t, lr, B1, B2, eps, wd)
        args = (ref, t, p, g, m0, v0, B1, B2, wd)
        for cfg_wd in (wd, 0.0):
            ref_c = _adam_ref64(p, g, m0, v0, t, lr, B1, B2, eps, cfg_wd)
            got = _adam_emul32(p, g, m0, v0, t, lr, B1, B2, eps, cfg_wd)
            worst = _check_adam(*got, ref_c, t, p, g, m0, v0, B1, B2,
                                cfg_wd, tag=f"emulation t={t} wd={cfg_wd}")
            print(f"emulation n={n} t={t} wd={cfg_wd}: m={worst[0]:.3g} "
                  f"v={worst[1]:.3g} p={worst[2]:.3g} of their bounds")
        for variant in WRONG_VARIANTS:
            # variants that are Adam itself at this t: t - 1 needs t >= 2
            # and both are the same once beta^t has left float32;
            # bc2 is 1 at t = 100000
            if variant == "t_minus_1" and t in (1, 100000):
                continue
            if variant == "no_bc2" and t == 100000:
                continue
            got = _adam_emul32(p, g, m0, v0, t, lr, B1, B2, eps, wd,
                               variant=variant)
            worst, _ = _adam_ratios(*got, *args)
            print(f"{variant} n={n} t={t}: m={worst[0]:.3g} "
                  f"v={worst[1]:.3g} p={worst[2]:.3g} of their bounds")
            assert max(worst) > 1.0, f"{variant} at t={t} was accepted"
            with pytest.raises(AssertionError):
                _check_adam(*got, *args, tag=variant)


def test_emulation_passes_on_every_gpu_test_input():
    """The emulation meets the bounds on exactly the inputs the GPU
    tests below feed the two kernels: same sizes, steps, hyperparameters
    and seeds, the first nb gradients rounded to bf16 for the mixed
    kernel. A kernel that misses a bound there is wrong, not unlucky."""
    def run(n, t, lr, eps, wd, data, worst_by_t):
        p, g, m0, v0 = data
        ref = _adam_ref64(p, g, m0, v0, t, lr, B1, B2, eps, wd)
        got = _adam_emul32(p, g, m0, v0, t, lr, B1, B2, eps, wd)
        w = _check_adam(*got, ref, t, p, g, m0, v0, B1, B2, wd,
                        tag=f"emulation n={n} t={t} lr={lr} wd={wd}")
        _fold(worst_by_t, t, w)

    small, large = {}, {}
    for n in FP32_SMALL_N:
        for t, lr, eps, wd, seed in _fp32_cases(n):
            run(n, t, lr, eps, wd, _make_data(n, t, seed), small)
    for n, nb in MIXED_SMALL:
        for t, lr, eps, wd, seed in _mixed_cases(n, nb):
            run(n, t, lr, eps, wd, _mixed_inputs(n, nb, t, seed)[:4], small)
    t, lr, eps, wd, seed = FP32_LARGE
    run(N_LARGE, t, lr, eps, wd, _make_data(N_LARGE, t, seed), large)
    t, lr, eps, wd, seed = MIXED_LARGE
    for nb in MIXED_LARGE_NB:
        run(N_LARGE, t, lr, eps, wd,
            _mixed_inputs(N_LARGE, nb, t, seed)[:4], large)
    _print_worst("emulation, small GPU inputs", small)
    _print_worst("emulation, large GPU inputs", large)


def test_p_bound_is_missed_only_where_m_cancels():
    """What the p bound does not cover, so that a miss on other data is
    read right. It charges the update 8 eps of itself, but m carries an
    error of up to 4 eps (b1 |m0| + (1 - b1)|grad|), and where the two
    terms of m cancel that is many times 4 eps |m'|. Any float32 Adam
    shows it; the bound has no term for it. With K = (b1 |m0| +
    (1 - b1)|grad|) / |m'|, on 400000 elements at t = 1000 the emulation
    misses the p bound on 14 elements, the worst at 3.83 of it, the
    least cancelled of them at K = 13; every element with K <= 2 is
    inside (worst 0.985). About 35 elements in a million at t >= 1000 and under one
    in a million at t = 2, where the bound is 60 times wider; the inputs
    of the GPU tests hold none (the test above)."""
    n, t, lr, eps, wd = 400_000, 1000, 1e-3, 1e-8, 0.01
    p, g, m0, v0 = _make_data(n, t, seed=t)
    p1, m1, v1, u = _adam_ref64(p, g, m0, v0, t, lr, B1, B2, eps, wd)
    got_p, got_m, got_v = _adam_emul32(p, g, m0, v0, t, lr, B1, B2, eps, wd)
    b1, b2, wd32 = _f32(B1), _f32(B2), _f32(wd)
    grad = g.astype(np.float64) + wd32 * p.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        K = (b1 * np.abs(m0) + (1 - b1) * np.abs(grad)) / np.abs(m1)
    K = np.nan_to_num(K, nan=1.0)
    d1 = 2 * EPS24 * b1 ** t / (1 - b1 ** t)
    d2 = 2 * EPS24 * b2 ** t / (1 - b2 ** t)
    bound_p = EPS24 * np.abs(p) + np.abs(u) * (8 * EPS24 + d1 + d2 / 2)
    r_p = _ratio(np.abs(got_p.astype(np.float64) - p1), bound_p)
    out = r_p > 1.0
    print(f"p bound at n={n} t={t}: {int(out.sum())} elements outside, "
          f"worst {r_p.max():.3g}, their least K {K[out].min():.3g}; "
          f"worst with K <= 2: {r_p[K <= 2].max():.3g}")
    assert (K[out] > 2).all()
    # m and v hold everywhere
    worst, _ = _adam_ratios(got_p, got_m, got_v, (p1, m1, v1, u), t, p, g,
                            m0, v0, B1, B2, wd)
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_checker_rejects_truncated_and_moved_results():
    """A result that is right but shifted by one element, or whose p was
    cut to bf16, is rejected; so is a p that changes where nothing
    should."""
    t, lr, eps, wd = 2, 1e-3, 1e-8, 0.0
    p, g, m0, v0 = _make_data(1031, t, seed=11)
    ref = _adam_ref64(p, g, m0, v0, t, lr, B1, B2, eps, wd)
    args = (ref, t, p, g, m0, v0, B1, B2, wd)
    p1, m1, v1 = _adam_emul32(p, g, m0, v0, t, lr, B1, B2, eps, wd)
    _check_adam(p1, m1, v1, *args)
    with pytest.raises(AssertionError):
        _check_adam(np.roll(p1, 1), m1, v1, *args)
    cut = (p1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    with pytest.raises(AssertionError):
        _check_adam(cut, m1, v1, *args)
    still = (g == 0) & (m0 == 0) & (v0 == 0)
    assert still.any()
    moved = p1.copy()
    moved[still] = np.nextafter(moved[still], np.float32(np.inf))
    with pytest.raises(AssertionError, match="p changed"):
        _check_adam(moved, m1, v1, *args)


# ------------------------------------------------------------ GPU: raw kernels
def _ext():
    from mi355x_scale.ops import _C, require_ext
    require_ext()
    return _C


def _guarded(payload, dev):
    """payload (1-D CPU tensor) inside a larger device allocation with a
    sentinel guard on both sides; returns (whole, contiguous view)."""
    n = payload.numel()
    whole = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=payload.dtype,
                       device=dev)
    whole[GUARD:GUARD + n] = payload.to(dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole):
    n = whole.numel() - 2 * GUARD
    return bool((whole[:GUARD] == SENTINEL).all()
                and (whole[GUARD + n:] == SENTINEL).all())


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().float().cpu().numpy().copy()


def _run_adam_step(n, t, lr, eps, wd, seed):
    """One adam_step launch on guarded buffers; asserts everything but
    the numerics and returns the worst ratios."""
    _C = _ext()
    dev = torch.device("cuda:0")
    p, g, m0, v0 = _make_data(n, t, seed)
    wp, vp = _guarded(torch.from_numpy(p), dev)
    wm, vm = _guarded(torch.from_numpy(m0), dev)
    wv, vv = _guarded(torch.from_numpy(v0), dev)
    g_dev = torch.from_numpy(g).to(dev)
    step = torch.tensor([t - 1], dtype=torch.int32, device=dev)
    _C.adam_step(vp, g_dev, vm, vv, step, lr, B1, B2, eps, wd)
    torch.cuda.synchronize()
    tag = f"adam_step n={n} t={t} lr={lr} eps={eps} wd={wd}"
    assert int(step.item()) == t, tag
    assert _guards_intact(wp) and _guards_intact(wm) and _guards_intact(wv), \
        f"{tag}: wrote outside the payload"
    assert _same_bits(g_dev, torch.from_numpy(g)), f"{tag}: g changed"
    ref = _adam_ref64(p, g, m0, v0, t, lr, B1, B2, eps, wd)
    return _check_adam(_np(vp), _np(vm), _np(vv), ref, t, p, g, m0, v0,
                       B1, B2, wd, tag=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("n", FP32_SMALL_N)
def test_adam_step_small_sizes(n):
    """float4 groups, the scalar tail and sizes below one group, at
    t in {1, 2, 1000}, with and without weight decay, at lr 1e-3, the
    flagship's 1e-5, and eps 1e-3."""
    worst_by_t = {}
    for t, lr, eps, wd, seed in _fp32_cases(n):
        _fold(worst_by_t, t, _run_adam_step(n, t, lr, eps, wd, seed))
    _print_worst(f"adam_step n={n}", worst_by_t)


@pytest.mark.gpu
def test_adam_step_grid_stride():
    """Three sweeps of the capped grid, the last partial, with a scalar
    tail of 3 in the last sweep."""
    t, lr, eps, wd, seed = FP32_LARGE
    w = _run_adam_step(N_LARGE, t, lr, eps, wd, seed)
    _print_worst(f"adam_step n={N_LARGE}", {t: w})


class _Mixed:
    """Guarded device buffers for one adam_step_mixed case."""

    def __init__(self, n, nb, t, seed, poison=()):
        dev = torch.device("cuda:0")
        self.n, self.nb, self.t = n, nb, t
        # the reference sees exactly the values the kernel reads
        p, g, m0, v0, self.gb_cpu, self.gf_cpu = _mixed_inputs(
            n, nb, t, seed, poison)
        self.p, self.g, self.m0, self.v0 = p, g, m0, v0
        self.w_master, self.master = _guarded(torch.from_numpy(p), dev)
        self.w_m, self.m = _guarded(torch.from_numpy(m0), dev)
        self.w_v, self.v = _guarded(torch.from_numpy(v0), dev)
        self.w_pb, self.pb = _guarded(
            torch.full((nb,), 3.0, dtype=torch.bfloat16), dev)
        self.gb = self.gb_cpu.to(dev)
        self.gf = self.gf_cpu.to(dev)
        self.step = torch.tensor([t - 1], dtype=torch.int32, device=dev)

    def tensors(self):
        return (self.master, self.gb, self.gf, self.m, self.v, self.pb,
                self.step)

    def check_untouched(self, tag):
        assert all(_guards_intact(w) for w in
                   (self.w_master, self.w_m, self.w_v, self.w_pb)), \
            f"{tag}: wrote outside the payload"
        assert _same_bits(self.gb, self.gb_cpu), f"{tag}: gb changed"
        assert _same_bits(self.gf, self.gf_cpu), f"{tag}: gf changed"


def _run_adam_mixed(n, nb, t, lr, eps, wd, seed, poison=()):
    _C = _ext()
    c = _Mixed(n, nb, t, seed, poison)
    _C.adam_step_mixed(*c.tensors(), lr, B1, B2, eps, wd)
    torch.cuda.synchronize()
    tag = f"adam_step_mixed n={n} nb={nb} t={t} lr={lr} wd={wd}"
    assert int(c.step.item()) == t, tag
    c.check_untouched(tag)
    mask = np.ones(n, dtype=bool)
    for i, _ in poison:
        mask[i] = False
    g_ref = np.where(mask, c.g, 0.0).astype(np.float32)
    ref = _adam_ref64(c.p, g_ref, c.m0, c.v0, t, lr, B1, B2, eps, wd)
    master = c.master.cpu()
    worst = _check_adam(master.numpy(), _np(c.m), _np(c.v), ref, t, c.p,
                        g_ref, c.m0, c.v0, B1, B2, wd, mask=mask, tag=tag)
    # pb is the round-to-nearest-even bf16 of the master the kernel wrote
    want_pb = master[:nb].bfloat16()
    keep = torch.from_numpy(mask[:nb])
    assert torch.equal(_bits(c.pb)[keep], _bits(want_pb)[keep]), \
        f"{tag}: pb is not the bf16 rounding of master"
    for i, _ in poison:
        outs = [c.master, c.m, c.v] + ([c.pb] if i < nb else [])
        assert not any(bool(torch.isfinite(o[i])) for o in outs), \
            f"{tag}: element {i} swallowed a non-finite gradient"
    for o in (c.master, c.m, c.v, c.pb):
        finite = torch.isfinite(o).cpu().numpy()
        assert finite[mask[:finite.size]].all(), \
            f"{tag}: a non-finite gradient leaked to another element"
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n,nb", MIXED_SMALL)
def test_adam_step_mixed_small_sizes(n, nb):
    """Every path of the mixed kernel: bf16 groups, fp32 groups, the
    group that straddles nb, the all-scalar fp32 segment when nb % 4 != 0,
    the tail, and the empty segments."""
    worst_by_t = {}
    for t, lr, eps, wd, seed in _mixed_cases(n, nb):
        _fold(worst_by_t, t, _run_adam_mixed(n, nb, t, lr, eps, wd, seed))
    _print_worst(f"adam_step_mixed n={n} nb={nb}", worst_by_t)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", MIXED_LARGE_NB)
def test_adam_step_mixed_grid_stride(nb):
    """Three sweeps with the bf16/fp32 split exactly on the sweep
    boundary, and misaligned inside the second sweep."""
    t, lr, eps, wd, seed = MIXED_LARGE
    w = _run_adam_mixed(N_LARGE, nb, t, lr, eps, wd, seed)
    _print_worst(f"adam_step_mixed n={N_LARGE} nb={nb}", {t: w})


@pytest.mark.gpu
@pytest.mark.parametrize("n,nb,i_nan,i_inf", [
    (1031, 516, 5, 522),    # both inside vector groups
    (1031, 515, 513, 520),  # straddling group, scalar fp32 segment
    (1031, 516, 1029, 2),   # fp32 tail, bf16 vector group
])
def test_adam_step_mixed_isolates_nonfinite_gradients(n, nb, i_nan, i_inf):
    """One NaN and one +inf gradient, one in each segment: only those
    elements of master, m, v and pb become non-finite, every other
    element still meets the bounds."""
    poison = ((i_nan, np.float32(np.nan)), (i_inf, np.float32(np.inf)))
    assert (i_nan < nb) != (i_inf < nb)
    for t in (1, 1000):
        w = _run_adam_mixed(n, nb, t, 1e-3, 1e-8, 0.01, seed=500 + t,
                            poison=poison)
        print(f"adam_step_mixed poisoned n={n} nb={nb} t={t}: m={w[0]:.3g} "
              f"v={w[1]:.3g} p={w[2]:.3g} of their bounds")


@pytest.mark.gpu
def test_adam_step_mixed_graph_replay_matches_eager():
    """One captured adam_step_mixed, replayed 5 times, leaves master, m,
    v, pb and step bit-identical to 5 eager calls from the same start."""
    _C = _ext()
    hp = (1e-3, B1, B2, 1e-8, 0.01)
    c = _Mixed(1031, 516, 4, seed=9)
    state = (c.master, c.m, c.v, c.pb, c.step)
    start = [s.clone() for s in state]

    def reset():
        for s, s0 in zip(state, start):
            s.copy_(s0)

    _C.adam_step_mixed(*c.tensors(), *hp)   # warm up before capture
    reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        _C.adam_step_mixed(*c.tensors(), *hp)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    replayed = [s.clone() for s in state]
    reset()
    for _ in range(5):
        _C.adam_step_mixed(*c.tensors(), *hp)
    torch.cuda.synchronize()
    assert int(c.step.item()) == 3 + 5
    for name, a, b in zip(("master", "m", "v", "pb"), replayed, state):
        assert _same_bits(a, b), f"{name} differs between replay and eager"
    assert torch.equal(replayed[4], c.step)
    assert not _same_bits(c.master, start[0])
    c.check_untouched("graph replay")


# --------------------------------------------------- GPU: binding rejections
def _mixed_args(c, **swap):
    names = ("master", "gb", "gf", "m", "v", "pb", "step")
    return tuple(swap.get(k, getattr(c, k)) for k in names)


@pytest.mark.gpu
def test_adam_bindings_reject_bad_buffers():
    """A CPU gb, a strided pb, a length mismatch and a payload view that
    starts one element off the vector alignment all raise in host code;
    the step counter shows that nothing was launched."""
    _C = _ext()
    dev = torch.device("cuda:0")
    hp = (1e-3, B1, B2, 1e-8, 0.0)
    n, nb = 1031, 516
    c = _Mixed(n, nb, 3, seed=21)
    before = [s.clone() for s in (c.master, c.m, c.v, c.pb)]
    wide_pb = torch.zeros(2 * nb, dtype=torch.bfloat16, device=dev)
    bad = {
        "cpu gb": dict(gb=c.gb_cpu),
        "cpu pb": dict(pb=c.pb.cpu()),
        "strided pb": dict(pb=wide_pb[::2]),
        "strided gb": dict(gb=wide_pb[::2]),
        "short m": dict(m=c.m[:n - 1]),
        "short pb": dict(pb=c.pb[:nb - 4]),
        "long gf": dict(gf=torch.zeros(n - nb + 1, device=dev)),
        "f64 gf": dict(gf=c.gf.double()),
        "strided gf": dict(gf=torch.zeros(2 * (n - nb), device=dev)[::2]),
        "master off by one": dict(master=c.w_master[GUARD + 1:GUARD + 1 + n]),
        "m off by one": dict(m=c.w_m[GUARD + 1:GUARD + 1 + n]),
        "v off by one": dict(v=c.w_v[GUARD - 1:GUARD - 1 + n]),
        "pb off by one": dict(pb=c.w_pb[GUARD + 1:GUARD + 1 + nb]),
        "gb off by one": dict(
            gb=torch.zeros(nb + 1, dtype=torch.bfloat16, device=dev)[1:]),
        "gf off by one": dict(gf=torch.zeros(n - nb + 1, device=dev)[1:]),
    }
    for what, swap in bad.items():
        with pytest.raises(RuntimeError):
            _C.adam_step_mixed(*_mixed_args(c, **swap), *hp)
        torch.cuda.synchronize()
        assert int(c.step.item()) == 2, f"{what}: a kernel was launched"
    for name, s, s0 in zip(("master", "m", "v", "pb"),
                           (c.master, c.m, c.v, c.pb), before):
        assert _same_bits(s, s0), f"{name} changed by a rejected call"

    g = torch.zeros(n, device=dev)
    bad32 = {
        "p off by one": (c.w_master[GUARD + 1:GUARD + 1 + n], g, c.m, c.v),
        "g off by one": (c.master, torch.zeros(n + 1, device=dev)[1:], c.m,
                         c.v),
        "m off by one": (c.master, g, c.w_m[GUARD + 1:GUARD + 1 + n], c.v),
        "v off by one": (c.master, g, c.m, c.w_v[GUARD + 1:GUARD + 1 + n]),
        "short g": (c.master, g[:n - 1], c.m, c.v),
    }
    for what, bufs in bad32.items():
        with pytest.raises(RuntimeError):
            _C.adam_step(*bufs, c.step, *hp)
        torch.cuda.synchronize()
        assert int(c.step.item()) == 2, f"{what}: a kernel was launched"
    # and the well-formed call still goes through
    _C.adam_step_mixed(*c.tensors(), *hp)
    torch.cuda.synchronize()
    assert int(c.step.item()) == 3


# ------------------------------------------------- GPU: FlatAdam(bf16_params)
@pytest.mark.gpu
@pytest.mark.parametrize("lin_in", [32, 31])
def test_flat_adam_bf16_params_gpu(lin_in):
    """FlatAdam(bf16_params=True) with a channels-last conv weight: two
    steps with distinct gradients written through each p.grad. Each step
    is judged from the state the optimizer actually held before it.
    lin_in = 31 makes n_bf16 odd, so the fp32 segment runs scalar."""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8),
                          nn.Flatten(), nn.Linear(lin_in, 5)).to(dev)
    model.to(memory_format=torch.channels_last)
    conv_w = model[0].weight
    assert conv_w.stride() == (27, 1, 9, 3)
    lr, eps, wd = 1e-3, 1e-8, 0.01
    opt = FlatAdam(model.parameters(), lr=lr, eps=eps, weight_decay=wd,
                   bf16_params=True)
    nb, n = opt.n_bf16, opt.flat_master.numel()
    assert nb == 8 * 27 + 5 * lin_in and n == nb + 8 + 8 + 8 + 5
    assert conv_w.dtype == torch.bfloat16
    assert conv_w.stride() == (27, 1, 9, 3)

    lo = opt.flat_master.data_ptr()
    hi = lo + 4 * n
    for p in opt.params:
        if p.dim() < 2:
            assert p.dtype == torch.float32
            assert lo <= p.data_ptr() and p.data_ptr() + 4 * p.numel() <= hi

    gen = torch.Generator().manual_seed(13)
    for t in (1, 2):
        p0, m0, v0 = (_np(x) for x in
                      (opt.flat_master, opt.exp_avg, opt.exp_avg_sq))
        opt.zero_grad()
        flat_g = torch.zeros(n, dtype=torch.float64)
        for p, key, off, cnt in opt.param_layout:
            gr = (torch.randn(p.shape, generator=gen)
                  * 10.0 ** torch.randint(-4, 2, p.shape, generator=gen))
            p.grad.copy_(gr.to(dev))
            seen = gr.to(p.grad.dtype).double()   # bf16-rounded where bf16
            at = off if key == "bf16" else nb + off
            flat_g[at:at + cnt].as_strided(p.shape, p.stride()).copy_(seen)
        opt.step()
        torch.cuda.synchronize()
        assert int(opt.step_t.item()) == t
        g = flat_g.numpy()
        ref = _adam_ref64(p0, g, m0, v0, t, lr, B1, B2, eps, wd)
        w = _check_adam(_np(opt.flat_master), _np(opt.exp_avg),
                        _np(opt.exp_avg_sq), ref, t, p0, g, m0, v0, B1, B2,
                        wd, tag=f"FlatAdam bf16 step {t}")
        print(f"FlatAdam bf16_params n={n} nb={nb} t={t}: m={w[0]:.3g} "
              f"v={w[1]:.3g} p={w[2]:.3g} of their bounds")
        assert (_np(opt.flat_master) != p0).all()
        for p, key, off, cnt in opt.param_layout:
            if key != "bf16":
                continue
            want = opt.flat_master[off:off + cnt].as_strided(
                p.shape, p.stride()).bfloat16()
            assert _same_bits(p.data, want), \
                "a bf16 parameter is not the rounding of its master slice"
