"""Group-fit kernels (``ops/csrc/groupfit.hip``, ``mfma_project.hip``) on
the production orders, across wave boundaries, in mixed-order waves and at
grid tails.

Data is the generator panel ``generate_demand_data(5, 26, 157)``: 130
groups (two full waves and a 2-lane tail), integer-valued 423..1644.

Two layers of bounds, neither fitted to the kernel:

* tight -- whatever is downstream of the solved coefficients
  (differencing, regression term, innovation recursion, one-step
  prediction, integration) is well conditioned because the shrinkage
  keeps sum|phi|, sum|theta| <= 0.98. ``groupfit_final`` returns its
  coefficients, so its fitted values are compared with an f64
  recomputation from the kernel's OWN ``params``.
* conditioning-limited -- the validation MSE against the f64 oracle. A
  few (group, order) pairs have ill-conditioned normal equations and move
  by up to 1e-1 in ANY f32 implementation; they are capped by count.

Every bound is 10x what the oracle itself does when run in float32 on the
CPU (``dtype=np.float32``), and ``test_f32_oracle_keeps_a_tenth_of_every_
gpu_bound`` re-asserts that in every CPU run, so the bounds are tied to
the reference and cannot drift towards the kernel. The 10x is for what
numpy does differently from the kernel: pairwise/BLAS summation and a
LAPACK solve against sequential sums, a hand Cholesky and FMA contraction.
"""
import functools

import numpy as np
import pytest

import groupfit_parent_oracle as parent
from mi355x_scale.data.generator import generate_demand_data
from mi355x_scale.forecast.batched import (_design_as, _fit_arma_one,
                                           batched_fit_reference,
                                           fitted_values_reference,
                                           make_exog_designs)
from mi355x_scale.forecast.pipeline import DEFAULT_GPU_ORDERS, EXO_COLS

PROD = [tuple(o) for o in DEFAULT_GPU_ORDERS]
ALL = PROD + [(2, 0, 2), (1, 2, 1)]
CAPPED = {(2, 1, 2), (2, 0, 2), (4, 1, 2)}
S_EVAL = 117
T_FULL = 157
G_FULL = 130
KX = len(EXO_COLS)
NPAR = 1 + KX + 8

# ---- the GPU bounds of this file (section numbers: see the tests) -------
FITTED_BOUND = 5e-6        # (a) x mean|y_g|; f32 oracle 4.8e-7
SHRINK_SLACK = 1e-6        # (a) sum|phi| <= 0.98 (1 + slack)
MSE_BOUND = 5e-3           # (c) relative; f32 oracle 5.0e-4 outside CAPPED
CAPPED_MIN_GROUPS = 120    # (c) of 130 within MSE_BOUND; f32 oracle >= 128
ARGMIN_MIN_GROUPS = 117    # (c) of 130; f32 oracle 128
REGRET_BOUND = 1e-2        # (c) f32 oracle 1e-14
REGRET_MIN_GROUPS = 120    # (c) of 130; f32 oracle 130
# What the f32 oracle may leave out, per order: groups above a tenth of
# MSE_BOUND and groups above MSE_BOUND itself (CPU emulation, numpy).
F32_ORACLE_OUT = {(0, 2, 1): (1, 0), (2, 1, 2): (4, 0), (2, 0, 2): (2, 1),
                  (4, 1, 2): (7, 2)}
F32_ORACLE_ARGMIN_OUT = 2


def _wm_bound(w):
    """|wm - mean64(w)|: sequential f32 sum of n terms, rows of w."""
    return w.shape[-1] * 2.0 ** -24 * np.abs(w).mean(axis=-1)


def _dot_bound(P, wc):
    """|P @ wc| rounding: f32 product + sequential f32 sum of n terms."""
    return P.shape[1] * 2.0 ** -23 * (np.abs(P) @ np.abs(wc))


def _frac(err, bound):
    """err as a fraction of bound; 0 where both are 0 (an exog column that
    is constant over the window has an all-zero row of P)."""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64),
                                     np.asarray(bound, dtype=np.float64))
    out = np.where(err == 0, 0.0, np.inf)
    np.divide(err, bound, out=out, where=bound > 0)
    return out


# ------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def _panel():
    df = generate_demand_data(5, 26, T_FULL)
    y = df.pivot_table(index=["Product", "SKU"], columns="Date",
                       values="Demand").to_numpy(dtype=np.float64)
    exog = df[df["SKU"] == df["SKU"].iloc[0]][EXO_COLS].to_numpy(
        dtype=np.float64)
    assert y.shape == (G_FULL, T_FULL) and exog.shape == (T_FULL, KX)
    # integer-valued: every difference and every w-sum is exact in f32
    assert (y == np.round(y)).all() and y.min() > 0 and y.max() < 2 ** 11
    y.setflags(write=False)
    exog.setflags(write=False)
    return y, exog


@functools.lru_cache(maxsize=None)
def _designs(train_len):
    return make_exog_designs(_panel()[1], train_len)


@functools.lru_cache(maxsize=None)
def _oracle_mse(dtype_name):
    """[130, 12] validation MSE of the oracle over ALL, computed once."""
    y, exog = _panel()
    out = batched_fit_reference(y, exog, ALL, S_EVAL,
                                designs=_designs(S_EVAL),
                                dtype=np.dtype(dtype_name))
    out.setflags(write=False)
    return out


def _diffed(y, d):
    w = np.asarray(y, dtype=np.float64)
    for _ in range(d):
        w = np.diff(w, axis=-1)
    return w


def _fitted_batch(y, Xc32, d, wm, beta, phi, theta):
    """``fitted_from_params`` for rows of y that share d ([G, T] f64)."""
    y = np.asarray(y, dtype=np.float64)
    G, T = y.shape
    n = T - d
    X = np.asarray(Xc32, dtype=np.float32).astype(np.float64)[:n]
    wm = np.asarray(wm, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    w = _diffed(y, d)
    reg = beta @ X.T                          # [G, n]
    u = (w - wm[:, None]) - reg
    what = wm[:, None] + reg
    eps = np.zeros((G, n))
    for t in range(n):
        acc = np.zeros(G)
        for i in range(min(4, t)):
            acc += phi[:, i] * u[:, t - 1 - i] + theta[:, i] * eps[:, t - 1 - i]
        what[:, t] += acc
        eps[:, t] = u[:, t] - acc
    fit = np.empty((G, T))
    fit[:, :d] = y[:, :d]
    if d == 0:
        fit[:] = what
    elif d == 1:
        fit[:, 1:] = y[:, :-1] + what
    else:
        fit[:, 2:] = 2 * y[:, 1:-1] - y[:, :-2] + what
    return fit


def fitted_from_params(y_g, design_d, d, wm, beta, phi, theta):
    """One-step-ahead fitted values [T] in f64 with the coefficients
    GIVEN, not estimated: the fitted-value recursion of
    ``fitted_values_reference``. The design is rounded to f32 and upcast,
    since that is what the kernel read; phi and theta have length 4."""
    return _fitted_batch(np.asarray(y_g)[None], design_d.Xc_full, d,
                         [wm], np.asarray(beta)[None],
                         np.asarray(phi)[None], np.asarray(theta)[None])[0]


def _fitted_from_param_rows(y, orders, params):
    """Per-lane orders: fitted_from_params of every row from its own
    ``params`` row (wm, beta[KX], phi[4], theta[4])."""
    ds = np.array([o[1] for o in orders])
    out = np.empty(y.shape)
    par = params.astype(np.float64)
    for d in np.unique(ds):
        rows = np.nonzero(ds == d)[0]
        dz = [z for z in _designs(y.shape[1]) if z.d == d][0]
        out[rows] = _fitted_batch(
            y[rows], dz.Xc_full, int(d), par[rows, 0], par[rows, 1:1 + KX],
            par[rows, 1 + KX:5 + KX], par[rows, 5 + KX:9 + KX])
    return out


# ------------------------------------------------------------------- CPU
def test_default_dtype_is_bit_identical_to_the_parent_oracle():
    """The dtype keyword must not move a single bit of the f64 oracle."""
    df = generate_demand_data(2, 4, T_FULL)
    y = df.pivot_table(index=["Product", "SKU"], columns="Date",
                       values="Demand").to_numpy()
    exog = df[df["SKU"] == df["SKU"].iloc[0]][EXO_COLS].to_numpy()
    orders = ALL + [(0, 1, 0), (2, 0, 2), (4, 0, 4), (3, 1, 3), (0, 0, 0)]
    new = batched_fit_reference(y, exog, orders, S_EVAL)
    old = parent.batched_fit_reference(y, exog, orders, S_EVAL)
    assert new.dtype == np.float64 and np.array_equal(new, old)
    assert np.array_equal(
        batched_fit_reference(y, exog, orders, S_EVAL, dtype=np.float64),
        old)
    for g in (0, 5):
        for order in orders:
            assert np.array_equal(
                fitted_values_reference(y[g], exog, order, T_FULL),
                parent.fitted_values_reference(y[g], exog, order, T_FULL)), \
                (g, order)


def test_f32_oracle_runs_in_f32():
    y, exog = _panel()
    mse = batched_fit_reference(y[:2], exog, [(1, 1, 1), (0, 2, 1)], S_EVAL,
                                dtype=np.float32)
    assert mse.dtype == np.float32 and np.isfinite(mse).all()
    fit = fitted_values_reference(y[0], exog, (2, 1, 2), T_FULL,
                                  dtype=np.float32)
    assert fit.dtype == np.float32 and fit.shape == (T_FULL,)
    u = np.linspace(-1, 1, 50, dtype=np.float32) ** 3
    for part in _fit_arma_one(u, 2, 1, dtype=np.float32):
        assert part.dtype == np.float32


def test_fitted_from_params_reproduces_the_f64_oracle():
    """Given the oracle's own coefficients (and the f64 design), the
    helper is the oracle's fitted-value pass."""
    y, exog = _panel()
    for order in [(4, 1, 2), (0, 2, 1), (2, 0, 1), (1, 1, 0), (0, 1, 0)]:
        p, d, q = order
        dz = [z for z in _designs(T_FULL) if z.d == d][0]
        w = _diffed(y[3], d)
        wm = w.mean()
        beta = dz.P @ (w - wm)
        u = (w - wm) - dz.Xc_full[:T_FULL - d] @ beta
        phi, theta, _ = _fit_arma_one(u, p, q)
        phi4 = np.concatenate([phi, np.zeros(4 - p)])
        theta4 = np.concatenate([theta, np.zeros(4 - q)])
        ref = fitted_values_reference(y[3], exog, order, T_FULL)
        got = fitted_from_params(y[3], dz, d, wm, beta, phi4, theta4)
        # the f32 rounding of the design is the only difference left
        scale = np.abs(y[3]).mean()
        assert np.abs(got - ref).max() <= 1e-6 * scale, order


def _f32_oracle_final(order):
    """The f32 oracle's full-series fit of all 130 groups: its fitted
    values and the coefficients it solved for, as a ``params`` array."""
    y, exog = _panel()
    p, d, q = order
    dz = _design_as([z for z in _designs(T_FULL) if z.d == d][0],
                    np.float32)
    n = T_FULL - d
    fitted = np.empty((G_FULL, T_FULL), dtype=np.float32)
    params = np.zeros((G_FULL, NPAR), dtype=np.float32)
    wcs = np.empty((G_FULL, n), dtype=np.float32)
    for g in range(G_FULL):
        w = y[g].astype(np.float32)
        for _ in range(d):
            w = np.diff(w)
        wm = w.mean()
        wc = w - wm
        beta = dz.P @ wc
        u = wc - dz.Xc_full[:n] @ beta
        phi, theta, _ = _fit_arma_one(u, p, q, dtype=np.float32)
        params[g, 0] = wm
        params[g, 1:1 + KX] = beta
        params[g, 1 + KX:1 + KX + p] = phi
        params[g, 5 + KX:5 + KX + q] = theta
        wcs[g] = wc
        fitted[g] = fitted_values_reference(y[g], exog, order, T_FULL,
                                            designs=_designs(T_FULL),
                                            dtype=np.float32)
    return fitted, params, wcs, dz


def test_f32_oracle_keeps_a_tenth_of_every_gpu_bound():
    """The f32 oracle (numpy on the CPU) stays within ONE TENTH of every
    bound the GPU tests below assert; where a GPU test allows a share of
    the groups out, the f32 oracle leaves out no more than
    ``F32_ORACLE_OUT`` records.

    Measured (numpy 2.2, f32 against f64 over the 130 groups): relative
    MSE deviation <= 1.9e-6 for the pure-AR / single-MA d <= 1 orders,
    2.0e-4 (1,1,1), 2.5e-4 (2,0,1), 2.2e-4 (1,2,1), 5.04e-4 (0,2,1),
    2.6e-3 (2,1,2), 6.6e-3 (2,0,2), 1.1e-1 (4,1,2); argmin over PROD
    equal in 128 of 130, regret 6e-15; fitted values against the f64
    recomputation from the run's own coefficients 4.8e-7 of mean|y|."""
    y, exog = _panel()
    r64, r32 = _oracle_mse("float64"), _oracle_mse("float32")
    assert np.isfinite(r32).all()
    rel = np.abs(r32 - r64) / r64
    for ci, order in enumerate(ALL):
        over_tenth = int((rel[:, ci] > MSE_BOUND / 10).sum())
        over = int((rel[:, ci] > MSE_BOUND).sum())
        print(f"f32 oracle mse {order}: worst={rel[:, ci].max():.3g} "
              f">{MSE_BOUND / 10:g}: {over_tenth}  >{MSE_BOUND:g}: {over}")
        allow_tenth, allow = F32_ORACLE_OUT.get(order, (0, 0))
        assert over_tenth <= allow_tenth, (order, over_tenth)
        assert over <= allow, (order, over)
        # what the GPU test lets out of MSE_BOUND covers what f32 costs
        gpu_allow = G_FULL - CAPPED_MIN_GROUPS if order in CAPPED else 0
        assert allow <= gpu_allow, order
    P = len(PROD)
    a32, a64 = r32[:, :P].argmin(1), r64[:, :P].argmin(1)
    argmin_out = int((a32 != a64).sum())
    regret = r64[np.arange(G_FULL), a32] / r64[:, :P].min(1) - 1.0
    print(f"f32 oracle ranking: argmin out={argmin_out} "
          f"regret={regret.max():.3g}")
    assert argmin_out <= F32_ORACLE_ARGMIN_OUT
    assert F32_ORACLE_ARGMIN_OUT <= G_FULL - ARGMIN_MIN_GROUPS
    assert (regret <= REGRET_BOUND / 10).all()

    scale = np.abs(y).mean(axis=1)
    worst_fit = worst_wm = worst_beta = 0.0
    for order in ALL:
        p, d, q = order
        fitted, params, wcs, dz = _f32_oracle_final(order)
        own = _fitted_from_param_rows(y, [order] * G_FULL, params)
        dev = (np.abs(fitted - own).max(axis=1) / scale).max()
        worst_fit = max(worst_fit, dev)
        assert dev <= FITTED_BOUND / 10, (order, dev)
        w = _diffed(y, d)
        r_wm = _frac(np.abs(params[:, 0] - w.mean(axis=1)),
                     _wm_bound(w)).max()
        worst_wm = max(worst_wm, r_wm)
        assert r_wm <= 0.1, (order, r_wm)
        P64 = dz.P.astype(np.float64)
        wc64 = wcs.astype(np.float64).T
        r_beta = _frac(np.abs(params[:, 1:1 + KX].T - P64 @ wc64),
                       _dot_bound(P64, wc64)).max()
        worst_beta = max(worst_beta, r_beta)
        assert r_beta <= 0.1, (order, r_beta)
        ph = np.abs(params[:, 1 + KX:5 + KX].astype(np.float64)).sum(1)
        th = np.abs(params[:, 5 + KX:].astype(np.float64)).sum(1)
        # The one bound without a 10x margin. Rescaling to 0.98 in f32
        # rounds 0.98 itself (+1.9e-8), the quotient 0.98 / sum and each
        # product (2^-24 = 6e-8 each): up to 4 x 2^-24 = 2.4e-7 over, and
        # the f32 oracle does reach 1.1e-7. SHRINK_SLACK is 4x that limit.
        assert 4 * 2.0 ** -24 <= SHRINK_SLACK / 4
        assert ph.max() <= 0.98 * (1 + 4 * 2.0 ** -24), (order, ph.max())
        assert th.max() <= 0.98 * (1 + 4 * 2.0 ** -24), (order, th.max())
    print(f"f32 oracle final: fitted={worst_fit:.3g} of mean|y|, "
          f"wm={worst_wm:.3g} and beta={worst_beta:.3g} of their bounds")

    # (g): numpy's f32 product against the bound of the MFMA test
    rng = np.random.default_rng(0)
    for n in (116, 117, 118, 119):
        P = rng.standard_normal((16, n)).astype(np.float32)
        wc = rng.standard_normal((n, G_FULL)).astype(np.float32)
        P64, wc64 = P.astype(np.float64), wc.astype(np.float64)
        r = _frac(np.abs((P @ wc) - P64 @ wc64), _dot_bound(P64, wc64))
        assert r.max() <= 0.1, (n, r.max())


# ------------------------------------------------------------------- GPU
PAD = 64


class _Bufs:
    """Output buffers followed by PAD canary elements each."""

    def __init__(self):
        self.bufs = {}

    def out(self, name, shape, dtype=None):
        import torch
        dtype = dtype or torch.float32
        n = int(np.prod(shape))
        canary = 173 if dtype == torch.uint8 else -12345.0
        full = torch.full((n + PAD,), canary, dtype=dtype, device="cuda")
        assert name not in self.bufs
        self.bufs[name] = (full, n, canary)
        return full[:n].view(shape)

    def check(self):
        import torch
        torch.cuda.synchronize()
        for name, (full, n, canary) in self.bufs.items():
            assert (full[n:] == canary).all().item(), f"canary after {name}"


def _np(t):
    return t.cpu().numpy()


def _projection(yT, ps, train_len, bufs, keep=None):
    """``batched._mfma_projection`` with canaried buffers; the canaries
    are asserted after each launch. ``keep`` collects wc per d."""
    from mi355x_scale.ops import _C
    G = yT.shape[1]
    betas, wms = [], []
    for d in range(3):
        n = train_len - d
        wc = bufs.out(f"wc{d}", (n, G))
        wm = bufs.out(f"wm{d}", (G,))
        _C.diff_center(yT, wc, wm, train_len, d)
        bufs.check()
        beta = bufs.out(f"beta{d}", (ps[d].shape[0], G))
        _C.exog_project_mfma(ps[d], wc, beta)
        bufs.check()
        betas.append(beta)
        wms.append(wm)
        if keep is not None:
            keep[f"wc{d}"] = _np(wc)
            keep[f"P{d}"] = _np(ps[d])
    return betas, wms


def _stage1(yT, ps, train_len, use_mfma, bufs, keep=None):
    import torch
    if use_mfma:
        return _projection(yT, ps, train_len, bufs, keep)
    empty = torch.empty(0, dtype=torch.float32, device="cuda")
    return [empty] * 3, [empty] * 3


def _panel_rows(G, nan):
    y = _panel()[0][:G]
    if nan:
        y = y.copy()
        y[65, 10] = np.nan
    return y


@functools.lru_cache(maxsize=None)
def _eval(orders, G=G_FULL, use_mfma=True, nan=False):
    """groupfit_eval through the extension: (mse [G, C], status [G, C])."""
    import torch
    from mi355x_scale.forecast.batched import _designs_to_gpu, _to_yT
    from mi355x_scale.ops import _C
    yT = _to_yT(_panel_rows(G, nan), "cuda")
    xs, ps = _designs_to_gpu(_designs(S_EVAL), "cuda")
    bufs = _Bufs()
    betas, wms = _stage1(yT, ps, S_EVAL, use_mfma, bufs)
    orders_t = torch.tensor(list(orders), dtype=torch.int32,
                            device="cuda").reshape(-1, 3).contiguous()
    C = orders_t.shape[0]
    mse = bufs.out("mse", (C, G))
    status = bufs.out("status", (C, G), torch.uint8)
    _C.groupfit_eval(yT, xs[0], xs[1], xs[2], ps[0], ps[1], ps[2],
                     orders_t, mse, status, S_EVAL,
                     betas[0], betas[1], betas[2], wms[0], wms[1], wms[2])
    bufs.check()
    out = _np(mse).T.copy(), _np(status).T.copy()
    for a in out:
        a.setflags(write=False)
    return out


def _mixed_orders(G):
    return tuple(ALL[g % len(ALL)] for g in range(G))


@functools.lru_cache(maxsize=None)
def _final(lane_orders, use_mfma=True, nan=False):
    """groupfit_final through the extension with one order per lane, on
    the first len(lane_orders) rows of the panel."""
    import torch
    from mi355x_scale.forecast.batched import _designs_to_gpu, _to_yT
    from mi355x_scale.ops import _C
    G = len(lane_orders)
    yT = _to_yT(_panel_rows(G, nan), "cuda")
    xs, ps = _designs_to_gpu(_designs(T_FULL), "cuda")
    bufs = _Bufs()
    res = {}
    betas, wms = _stage1(yT, ps, T_FULL, use_mfma, bufs, res)
    best = torch.tensor(list(lane_orders), dtype=torch.int32,
                        device="cuda").reshape(G, 3).contiguous()
    fitted = bufs.out("fitted", (T_FULL, G))
    params = bufs.out("params", (G, NPAR))
    status = bufs.out("status", (G,), torch.uint8)
    _C.groupfit_final(yT, xs[0], xs[1], xs[2], ps[0], ps[1], ps[2],
                      best, fitted, params, status,
                      betas[0], betas[1], betas[2], wms[0], wms[1], wms[2])
    bufs.check()
    res.update(fitted=_np(fitted).T.copy(), params=_np(params),
               status=_np(status))
    for a in res.values():
        a.setflags(write=False)
    return res


def _check_final(res, lane_orders, use_mfma, tag):
    """The assertions of (a), per lane. Returns the worst figures, each
    as a fraction of its bound (fitted: of mean|y_g|)."""
    G = len(lane_orders)
    y = _panel()[0][:G]
    par = res["params"]
    assert par.shape == (G, NPAR)
    assert res["status"].tolist() == [1] * G
    own = _fitted_from_param_rows(y, lane_orders, par)
    scale = np.abs(y).mean(axis=1)
    fit_dev = np.abs(res["fitted"] - own).max(axis=1) / scale
    phi, theta = par[:, 1 + KX:5 + KX], par[:, 5 + KX:9 + KX]
    wm_dev = np.empty(G)
    beta_dev = np.zeros(G)
    for g, (p, d, q) in enumerate(lane_orders):
        assert (phi[g, p:] == 0).all() and (theta[g, q:] == 0).all(), g
        w = _diffed(y[g], d)
        wm_dev[g] = _frac(abs(par[g, 0] - w.mean()), _wm_bound(w))
    for d in sorted({o[1] for o in lane_orders}) if use_mfma else ():
        rows = np.nonzero([o[1] == d for o in lane_orders])[0]
        P64 = res[f"P{d}"].astype(np.float64)
        wc64 = res[f"wc{d}"].astype(np.float64)[:, rows]
        beta_dev[rows] = _frac(np.abs(par[rows, 1:1 + KX].T - P64 @ wc64),
                               _dot_bound(P64, wc64)).max(axis=0)
    sums = np.maximum(np.abs(phi.astype(np.float64)).sum(1),
                      np.abs(theta.astype(np.float64)).sum(1))
    print(f"groupfit_final {tag} mfma={use_mfma}: "
          f"fitted={fit_dev.max():.3g} wm={wm_dev.max():.3g} "
          f"beta={beta_dev.max():.3g} sum|coef|-0.98="
          f"{sums.max() - 0.98:.3g}")
    assert (fit_dev <= FITTED_BOUND).all(), (int(fit_dev.argmax()),
                                             fit_dev.max())
    assert (sums <= 0.98 * (1 + SHRINK_SLACK)).all(), sums.max()
    assert (wm_dev <= 1.0).all(), (int(wm_dev.argmax()), wm_dev.max())
    assert (beta_dev <= 1.0).all(), (int(beta_dev.argmax()), beta_dev.max())


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
@pytest.mark.parametrize("order", ALL, ids=str)
def test_gpu_final_fit_matches_its_own_coefficients(order, use_mfma):
    """(a) One order on all 130 lanes, T = 157. status 1; fitted values
    within 5e-6 x mean|y_g| of the f64 recursion run from the kernel's own
    params, at every t from 0; phi/theta zero past p/q and summing to at
    most 0.98 (1 + 1e-6); wm within n 2^-24 mean|w| of the f64 mean; with
    the MFMA projection, beta within n 2^-23 (|P| @ |wc|) of the f64
    product of the f32 operands.

    Measured on an MI355X, the same with and without the MFMA stage 1:
    fitted 1.09e-6 of mean|y| at (2,0,2), 7.9e-7 at (2,0,1), 1.6e-7 at
    (1,0,0) and 9.5e-8..2.2e-7 at the nine d >= 1 orders (f32 oracle on
    the CPU: 4.8e-7); wm at most 5.1e-3 of its bound (f32 oracle 5.1e-3:
    the w-sums of this panel are exact in f32); beta at most 2.0e-2 of its
    bound (f32 oracle 1.2e-2); sum|phi|, sum|theta| at most
    0.98 (1 + 1.3e-7) (f32 oracle 1.1e-7)."""
    res = _final((order,) * G_FULL, use_mfma)
    _check_final(res, (order,) * G_FULL, use_mfma, str(order))


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
def test_gpu_mixed_order_waves_equal_uniform_launches(use_mfma):
    """(b) best_order[g] = ALL[g % 12]: every wave holds K = 0, pure-AR
    and q > 0 lanes with d = 0, 1 and 2 side by side. The wave-voted
    passes (``__any``) must leave each lane exactly what it gets in a
    launch where all 130 lanes run its order: fitted, params and status
    bit-identical."""
    lanes = _mixed_orders(G_FULL)
    mixed = _final(lanes, use_mfma)
    _check_final(mixed, lanes, use_mfma, "mixed")
    for ci, order in enumerate(ALL):
        uni = _final((order,) * G_FULL, use_mfma)
        rows = np.arange(ci, G_FULL, len(ALL))
        for k in ("fitted", "params", "status"):
            assert np.array_equal(mixed[k][rows], uni[k][rows]), (order, k)


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
def test_gpu_eval_matches_oracle_on_production_orders(use_mfma):
    """(c) Validation MSE, S = 117, ALL orders, against the f64 oracle.
    status 1 and finite everywhere; relative error <= 5e-3 for all 130
    groups outside CAPPED and for >= 120 of 130 inside; over PROD the
    argmin equals the oracle's in >= 117 groups and the oracle's MSE at
    the kernel's argmin is within 1e-2 of its minimum in >= 120 groups.

    Measured on an MI355X, the same with and without the MFMA stage 1
    (in brackets the f32 oracle on the CPU). Worst relative error outside
    CAPPED: (1,0,0) 1.3e-6, (2,1,0) 9.7e-6, (1,1,0) 1.5e-5, (0,1,0)
    2.3e-5, (0,1,1) 2.4e-5, (1,1,1) 6.8e-5 [2.0e-4], (2,0,1) 1.7e-4
    [2.5e-4], (1,2,1) 2.2e-4 [2.2e-4], (0,2,1) 4.6e-4 [5.0e-4]. Inside
    CAPPED, groups within 5e-3 and the worst: (2,1,2) 130, 2.4e-3 [130,
    2.6e-3]; (2,0,2) 129, 6.2e-3 [129, 6.6e-3]; (4,1,2) 128, 2.7e-2 [128,
    1.1e-1]. The groups above 5e-4 are 62, 64, 83, 113 at (2,1,2) [62, 64,
    111, 113], 109 at (2,0,2) [109, 111] and 11, 44, 61, 63, 105, 109,
    123 at (4,1,2) [11, 44, 61, 63, 68, 109, 115]: the ill-conditioned
    groups are largely the same ones. Argmin equal in 129 of 130 [128];
    regret within 1e-2 in all 130, worst 5.8e-15 [5.8e-15]."""
    mse, status = _eval(tuple(ALL), G_FULL, use_mfma)
    ref = _oracle_mse("float64")
    assert status.tolist() == [[1] * len(ALL)] * G_FULL
    assert np.isfinite(mse).all()
    rel = np.abs(mse - ref) / ref
    for ci, order in enumerate(ALL):
        ok = int((rel[:, ci] <= MSE_BOUND).sum())
        above = np.nonzero(rel[:, ci] > MSE_BOUND / 10)[0].tolist()
        print(f"groupfit_eval {order} mfma={use_mfma}: "
              f"worst={rel[:, ci].max():.3g} within={ok} "
              f">{MSE_BOUND / 10:g}: {above}")
    for ci, order in enumerate(ALL):
        ok = int((rel[:, ci] <= MSE_BOUND).sum())
        need = CAPPED_MIN_GROUPS if order in CAPPED else G_FULL
        assert ok >= need, (order, ok, rel[:, ci].max())
    P = len(PROD)
    pick, best = mse[:, :P].argmin(1), ref[:, :P].argmin(1)
    regret = ref[np.arange(G_FULL), pick] / ref[:, :P].min(1) - 1.0
    agree = int((pick == best).sum())
    low = int((regret <= REGRET_BOUND).sum())
    print(f"groupfit_eval ranking mfma={use_mfma}: argmin equal={agree} "
          f"regret<=1e-2: {low} worst regret={regret.max():.3g}")
    assert agree >= ARGMIN_MIN_GROUPS, agree
    assert low >= REGRET_MIN_GROUPS, (low, regret.max())


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
def test_gpu_eval_is_independent_of_the_candidate_list(use_mfma):
    """(d) The per-lane LDS state block is reused from candidate to
    candidate: a candidate's MSE column has the same bits with ALL, with
    ALL reversed and alone."""
    fwd, fs = _eval(tuple(ALL), G_FULL, use_mfma)
    rev, rs = _eval(tuple(ALL[::-1]), G_FULL, use_mfma)
    assert np.array_equal(rev[:, ::-1], fwd)
    assert np.array_equal(rs[:, ::-1], fs)
    for order in [(0, 1, 0), (0, 2, 1), (4, 1, 2)]:
        one, os_ = _eval((order,), G_FULL, use_mfma)
        ci = ALL.index(order)
        assert np.array_equal(one[:, 0], fwd[:, ci]), order
        assert np.array_equal(os_[:, 0], fs[:, ci]), order


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
@pytest.mark.parametrize("G", [1, 63, 65])
def test_gpu_grid_tail_is_bit_exact_and_in_bounds(G, use_mfma):
    """(e) A block with clamped tail lanes: the first G rows alone give
    the bits of the 130-group run, and nothing is written past G -- the
    canaries after wc, wm, beta, mse, fitted, params and both status
    buffers are asserted inside the runners."""
    full_mse, full_st = _eval(tuple(ALL), G_FULL, use_mfma)
    mse, st = _eval(tuple(ALL), G, use_mfma)
    assert np.array_equal(mse, full_mse[:G])
    assert np.array_equal(st, full_st[:G])
    full = _final(_mixed_orders(G_FULL), use_mfma)
    part = _final(_mixed_orders(G), use_mfma)
    for k in ("fitted", "params", "status"):
        assert np.array_equal(part[k], full[k][:G]), k


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
def test_gpu_non_finite_series_fails_alone(use_mfma):
    """(f) y[65, 10] = nan: group 65 is +inf / status 0 for every order
    in eval and status 0 in final; every other group keeps its bits."""
    keep = np.arange(G_FULL) != 65
    mse, st = _eval(tuple(ALL), G_FULL, use_mfma, nan=True)
    clean_mse, clean_st = _eval(tuple(ALL), G_FULL, use_mfma)
    assert (mse[65] == np.inf).all() and (st[65] == 0).all()
    assert np.array_equal(mse[keep], clean_mse[keep])
    assert np.array_equal(st[keep], clean_st[keep])
    lanes = _mixed_orders(G_FULL)
    got, clean = _final(lanes, use_mfma, nan=True), _final(lanes, use_mfma)
    assert got["status"][65] == 0
    for k in ("fitted", "params", "status"):
        assert np.array_equal(got[k][keep], clean[k][keep]), k


@pytest.mark.gpu
def test_gpu_canaried_projection_is_the_drivers():
    """The canaried stage 1 used above is ``batched._mfma_projection``."""
    from mi355x_scale.forecast.batched import (_designs_to_gpu,
                                               _mfma_projection, _to_yT)
    yT = _to_yT(_panel()[0], "cuda")
    _, ps = _designs_to_gpu(_designs(S_EVAL), "cuda")
    betas, wms = _mfma_projection(yT, ps, S_EVAL, "cuda")
    mine_b, mine_w = _projection(yT, ps, S_EVAL, _Bufs())
    for d in range(3):
        assert np.array_equal(_np(betas[d]), _np(mine_b[d]))
        assert np.array_equal(_np(wms[d]), _np(mine_w[d]))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 130, 257])
def test_gpu_diff_center(G):
    """(g) d in (0, 1, 2) x S in (117, 157). The panel is integer-valued,
    so the differences are exact in f32: wm within n 2^-24 mean|w| of the
    f64 mean, and wc == w32 - wm exactly.

    Measured on an MI355X: wm at most 7.0e-3 of its bound."""
    from mi355x_scale.forecast.batched import _to_yT
    from mi355x_scale.ops import _C
    y = np.tile(_panel()[0], (2, 1))[:G] if G > G_FULL else _panel()[0][:G]
    assert (y == np.round(y)).all()
    yT = _to_yT(y, "cuda")
    worst = 0.0
    for S in (117, 157):
        for d in (0, 1, 2):
            n = S - d
            bufs = _Bufs()
            wc = bufs.out("wc", (n, G))
            wm = bufs.out("wm", (G,))
            _C.diff_center(yT, wc, wm, S, d)
            bufs.check()
            w = _diffed(y[:, :S], d)
            w32 = w.astype(np.float32)
            assert np.array_equal(w32.astype(np.float64), w)
            wm_gpu = _np(wm)
            dev = _frac(np.abs(wm_gpu - w.mean(axis=1)),
                        _wm_bound(w)).max()
            worst = max(worst, dev)
            assert dev <= 1.0, (S, d, dev)
            assert np.array_equal(_np(wc).T, w32 - wm_gpu[:, None]), (S, d)
    print(f"diff_center G={G}: wm={worst:.3g} of its bound")


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 15, 17, 130])
def test_gpu_exog_project_mfma(G):
    """(g) n in (116..119) (every n % 4) x KX in (1, 3, 8, 16), standard
    normal operands: beta within n 2^-23 (|P| @ |wc|) of the f64 product
    of the f32 operands; rows >= KX of a [16, G] buffer stay untouched.

    Measured on an MI355X: at most 1.4e-2 of the bound (numpy's f32
    product on the CPU: below 1e-1 of it)."""
    import torch
    from mi355x_scale.ops import _C
    rng = np.random.default_rng(1000 + G)
    worst = 0.0
    for n in (116, 117, 118, 119):
        for kx in (1, 3, 8, 16):
            P = rng.standard_normal((kx, n)).astype(np.float32)
            wc = rng.standard_normal((n, G)).astype(np.float32)
            bufs = _Bufs()
            sixteen = bufs.out("beta16", (16, G))
            beta = sixteen.view(-1)[:kx * G].view(kx, G)
            _C.exog_project_mfma(torch.tensor(P, device="cuda"),
                                 torch.tensor(wc, device="cuda"), beta)
            bufs.check()
            assert (sixteen.view(-1)[kx * G:] == -12345.0).all().item(), \
                (n, kx)
            P64, wc64 = P.astype(np.float64), wc.astype(np.float64)
            dev = _frac(np.abs(_np(beta) - P64 @ wc64),
                        _dot_bound(P64, wc64)).max()
            worst = max(worst, dev)
            assert dev <= 1.0, (n, kx, dev)
    print(f"exog_project_mfma G={G}: worst={worst:.3g} of its bound")


# ------------------------------------------------- (h) the binding checks
def _binding_args(S, G=G_FULL, C=2):
    """Valid operands of ``groupfit_eval`` (S < T) / ``groupfit_final``
    (S = T) on the panel, outputs canaried: (args by name, call)."""
    import torch
    from mi355x_scale.forecast.batched import _designs_to_gpu, _to_yT
    from mi355x_scale.ops import _C
    final = S == T_FULL
    xs, ps = _designs_to_gpu(_designs(S), "cuda")
    bufs = _Bufs()
    a = dict(yT=_to_yT(_panel()[0][:G], "cuda"))
    for d in range(3):
        a[f"xc{d}"], a[f"pj{d}"] = xs[d], ps[d]
        a[f"b{d}"] = torch.zeros((KX, G), device="cuda")
        a[f"w{d}"] = torch.zeros((G,), device="cuda")
    rows = G if final else C
    a["orders"] = torch.ones((rows, 3), dtype=torch.int32, device="cuda")
    if final:
        a["fitted"] = bufs.out("fitted", (T_FULL, G))
        a["params"] = bufs.out("params", (G, NPAR))
        a["status"] = bufs.out("status", (G,), torch.uint8)
        outs = ("fitted", "params", "status")
    else:
        a["mse"] = bufs.out("mse", (C, G))
        a["status"] = bufs.out("status", (C, G), torch.uint8)
        outs = ("mse", "status")

    def call(**change):
        k = dict(a, **change)
        head = [k[n] for n in ("yT", "xc0", "xc1", "xc2", "pj0", "pj1",
                               "pj2", "orders") + outs]
        tail = [k[f"{n}{d}"] for n in "bw" for d in range(3)]
        if final:
            _C.groupfit_final(*head, *tail)
        else:
            _C.groupfit_eval(*head, S, *tail)
        torch.cuda.synchronize()

    def untouched():
        bufs.check()
        return all((full == canary).all().item()
                   for full, _, canary in bufs.bufs.values())

    return a, call, untouched


@pytest.mark.gpu
@pytest.mark.parametrize("S", [S_EVAL, T_FULL], ids=["eval", "final"])
def test_gpu_fit_bindings_reject_bad_operands(S):
    """(h) ``groupfit_eval`` / ``groupfit_final`` raise before any launch
    for each malformed operand, one at a time, and leave the canaried
    outputs as they were; the stacked designs of a forecast (more rows
    than T - d) are accepted."""
    import torch
    G = G_FULL
    a, call, untouched = _binding_args(S)
    orders4 = torch.ones((a["orders"].shape[0], 4), dtype=torch.int32,
                         device="cuda")
    nine = torch.zeros((T_FULL, 9), device="cuda")
    bad = {
        "xc1 one row short": dict(xc1=a["xc1"][:T_FULL - 2].contiguous()),
        "pj2 with S-1 columns": dict(pj2=torch.zeros((KX, S - 1),
                                                     device="cuda")),
        "b0 [KX][G-1]": dict(b0=torch.zeros((KX, G - 1), device="cuda")),
        "w1 [G+1]": dict(w1=torch.zeros((G + 1,), device="cuda")),
        "non-contiguous orders": dict(orders=orders4[:, :3]),
        "status length": dict(status=torch.full(
            (a["status"].numel() + 1,), 173, dtype=torch.uint8,
            device="cuda")),
        "KX = 9": dict(xc0=nine, xc1=nine[1:].contiguous(),
                       xc2=nine[2:].contiguous()),
    }
    if S == T_FULL:
        bad["params one column short"] = dict(
            params=torch.full((G, NPAR - 1), -12345.0, device="cuda"))
    else:
        bad["mse one row short"] = dict(
            mse=torch.full((1, G), -12345.0, device="cuda"))
    for what, change in bad.items():
        print(what)
        with pytest.raises(RuntimeError):
            call(**change)
        assert untouched(), what
    # three more design rows than the fit reads: accepted
    more = {f"xc{d}": torch.cat([a[f"xc{d}"], a[f"xc{d}"][:3]]).contiguous()
            for d in range(3)}
    call(**more)
    assert not untouched()


@pytest.mark.gpu
def test_gpu_projection_bindings_reject_bad_operands():
    """(h) ``diff_center`` and ``exog_project_mfma`` raise before any
    launch for a wc one row short, a wm one element short, d = 3 and a
    beta of [KX][G-1]; the canaried outputs stay as they were."""
    import torch
    from mi355x_scale.forecast.batched import _designs_to_gpu, _to_yT
    from mi355x_scale.ops import _C
    G, S, d = G_FULL, S_EVAL, 1
    yT = _to_yT(_panel()[0], "cuda")
    _, ps = _designs_to_gpu(_designs(S), "cuda")
    bufs = _Bufs()
    wc = bufs.out("wc", (S - d, G))
    wm = bufs.out("wm", (G,))
    beta = bufs.out("beta", (KX, G))
    short_wc = bufs.out("short_wc", (S - d - 1, G))
    short_wm = bufs.out("short_wm", (G - 1,))
    wc3 = bufs.out("wc3", (S - 3, G))
    short_beta = bufs.out("short_beta", (KX, G - 1))
    for args in ((yT, short_wc, wm, S, d), (yT, wc, short_wm, S, d),
                 (yT, wc3, wm, S, 3), (yT, wc, wm, S, -1),
                 (yT, wc, wm, T_FULL + 1, d)):
        with pytest.raises(RuntimeError):
            _C.diff_center(*args)
    for args in ((ps[d], wc, short_beta), (ps[0], wc, beta)):
        with pytest.raises(RuntimeError):
            _C.exog_project_mfma(*args)
    bufs.check()
    for name, (full, _, canary) in bufs.bufs.items():
        assert (full == canary).all().item(), name
