"""Batched ARIMAX out-of-sample forecast with standard errors
(``groupfit_forecast_kernel`` in ``ops/csrc/groupfit.hip``), its numpy
oracle in ``forecast/batched.py`` and the public interface above them.

Data is the 130-group x 157-week generator panel of
``test_groupfit_kernels`` (two full waves and a 2-lane tail); the 40
future weeks carry two christmas rows and one new-year row. Horizons are
H = 1 (ring edge), 7 (one past the 6-deep psi ring) and 40 (production).

Bounds, as in ``test_groupfit_kernels``: each GPU bound is 10x what the
oracle itself does when run in float32 on the CPU, and
``test_f32_oracle_keeps_a_tenth_of_every_forecast_bound`` re-asserts that
in every CPU run, so the bounds are tied to the reference and cannot drift
towards the kernel.
"""
import functools

import numpy as np
import pandas as pd
import pytest

import test_groupfit_kernels as gk
from mi355x_scale.data.generator import generate_demand_data
from mi355x_scale.forecast.batched import (ExogDesign, batched_fit_reference,
                                           batched_forecast_gpu,
                                           batched_forecast_reference,
                                           forecast_from_params_reference,
                                           psi_weights_reference,
                                           stacked_exog_designs)
from mi355x_scale.forecast.pipeline import (EXO_COLS, _future_dates,
                                            add_exo_variables,
                                            run_fine_grained_forecast)
from mi355x_scale.forecast.sarimax import SARIMAX

ALL = gk.ALL
G_FULL, T_FULL, KX, NPAR = gk.G_FULL, gk.T_FULL, gk.KX, gk.NPAR
HORIZONS = (1, 7, 40)
H_MAX = 40

# ---- the GPU bounds of this file ----------------------------------------
# From given coefficients, H = 40, all 130 groups; each is 10x the f32
# oracle's worst figure against f64, which stands next to it.
FC_BOUND_D01 = 8.5e-6   # x mean|y_g|, d <= 1; f32 oracle 8.49e-7 at (2,1,2)
FC_BOUND_D2 = 8.8e-4    # x mean|y_g|, d = 2;  f32 oracle 8.76e-5 at (0,2,1)
SIGMA2_BOUND = 1.1e-5   # relative; f32 oracle 1.08e-6 at (1,2,1)
# forecast_se, relative, by d. (1-B)^d puts d roots of the AR polynomial
# on the unit circle; rounding a_k to f32 moves them by about
# 2^-24 / (1 - sum phi), and psi_h grows with that over the h steps.
SE_BOUND = {0: 4.9e-6,  # f32 oracle 4.86e-7 at (2,0,2)
            1: 1.7e-4,  # f32 oracle 1.69e-5 at (2,1,2)
            2: 8.7e-4}  # f32 oracle 8.63e-5 at (1,2,1)
# End to end (fit + forecast) against the f64 oracle the forecast is
# conditioning-limited like the validation MSE. Per order, the f32
# oracle's worst group as a fraction of mean|y_g|, H = 40; the GPU bound
# is 10x that. At (2,0,2) one group of the f32 oracle (6.1e-3, above the
# GPU bound too) is left out.
E2E_F32 = {(0, 1, 0): 1.3e-7, (1, 0, 0): 1.9e-7, (1, 1, 0): 1.4e-7,
           (0, 1, 1): 1.6e-7, (1, 1, 1): 7.9e-5, (2, 1, 0): 1.3e-7,
           (2, 0, 1): 7.8e-3, (0, 2, 1): 8.9e-5, (2, 1, 2): 2.3e-3,
           (4, 1, 2): 1.1e-3, (2, 0, 2): 2.0e-4, (1, 2, 1): 6.0e-5}
E2E_MIN_GROUPS = 120    # of 130 within the bound for orders in gk.CAPPED
# Groups the f32 oracle may leave above its own figure (a tenth of the GPU
# bound) and above the bound itself, per order.
F32_E2E_OUT = {(2, 0, 2): (1, 1)}


def _e2e_bound(order):
    return 10 * E2E_F32[order]


def _fc_bound(order):
    return FC_BOUND_D2 if order[1] == 2 else FC_BOUND_D01


# ------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def _future_exog(H=H_MAX):
    dates = generate_demand_data(1, 1, T_FULL)["Date"].to_numpy()
    fx = add_exo_variables(pd.DataFrame(
        {"Date": _future_dates(dates, H)}))[EXO_COLS].to_numpy(
            dtype=np.float64)
    assert fx.shape == (H, KX)
    fx.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def _stacked(H=H_MAX):
    """Stacked designs over the panel's 157 weeks + H future weeks."""
    return stacked_exog_designs(gk._panel()[1], _future_exog(H), T_FULL)


@functools.lru_cache(maxsize=None)
def _stacked_as_read(H=H_MAX):
    """The stacked designs rounded to f32 and upcast, as the kernel read
    them."""
    return {dz.d: ExogDesign(
        d=dz.d, Xc_full=dz.Xc_full.astype(np.float32).astype(np.float64),
        P=dz.P, xmean=dz.xmean) for dz in _stacked(H)}


def _from_params(y, lane_orders, params, H, dtype=np.float64):
    """``forecast_from_params_reference`` of every row from its own
    ``params`` row, on the design as the kernel read it."""
    G = len(lane_orders)
    fc = np.empty((G, H), dtype=dtype)
    se = np.empty((G, H), dtype=dtype)
    s2 = np.empty(G, dtype=dtype)
    by_d = _stacked_as_read(H)
    par = np.asarray(params)
    for g, order in enumerate(lane_orders):
        fc[g], se[g], s2[g] = forecast_from_params_reference(
            y[g], by_d[order[1]], order, par[g, 0], par[g, 1:1 + KX],
            par[g, 1 + KX:5 + KX], par[g, 5 + KX:9 + KX], H, dtype)
    return fc, se, s2


def _deviations(got, ref, y):
    """Worst figures per group: forecast as a fraction of mean|y_g|,
    sigma2 and forecast_se relative."""
    fc, se, s2 = got
    rfc, rse, rs2 = (np.asarray(a, dtype=np.float64) for a in ref)
    scale = np.abs(y).mean(axis=1)
    return (np.abs(fc - rfc).max(axis=1) / scale,
            np.abs(s2 - rs2) / rs2,
            (np.abs(se - rse) / rse).max(axis=1))


@functools.lru_cache(maxsize=None)
def _e2e_reference(dtype_name):
    """{order: forecast [130, 40]} of the end-to-end oracle, computed
    once."""
    y, exog = gk._panel()
    out = {}
    for order in ALL:
        fc, _, _ = batched_forecast_reference(
            y, exog, _future_exog(), order, dtype=np.dtype(dtype_name))
        fc.setflags(write=False)
        out[order] = fc
    return out


def _e2e_dev(fc, order):
    """|fc - f64 end-to-end oracle| as a fraction of mean|y_g|, per
    group."""
    y = gk._panel()[0]
    ref = _e2e_reference("float64")[order]
    return (np.abs(np.asarray(fc, dtype=np.float64) - ref).max(axis=1)
            / np.abs(y).mean(axis=1))


# ------------------------------------------------------------------- CPU
def test_psi_weights_equal_an_independent_filter():
    """(1) The oracle's psi recursion against scipy's rational filter
    ``theta(B) / (phi(B) (1-B)^d)`` applied to a unit impulse, 40 steps,
    to 1e-10 relative (f64 round-off over 40 recursive steps; measured
    here: 8.2e-14)."""
    from scipy import signal
    rng = np.random.default_rng(7)
    impulse = np.zeros(H_MAX)
    impulse[0] = 1.0
    worst = 0.0
    for p, d, q in ALL + [(4, 2, 4), (0, 0, 0)]:
        for _ in range(5):
            phi = rng.uniform(-1, 1, p)
            theta = rng.uniform(-1, 1, q)
            if p:
                phi *= 0.98 * rng.uniform() / np.abs(phi).sum()
            if q:
                theta *= 0.98 * rng.uniform() / np.abs(theta).sum()
            ar = np.concatenate([[1.0], -phi])
            for _ in range(d):
                ar = np.convolve(ar, [1.0, -1.0])
            ref = signal.lfilter(np.concatenate([[1.0], theta]), ar, impulse)
            got = psi_weights_reference(phi, theta, d, H_MAX)
            assert got[0] == 1.0
            dev = np.abs(got - ref).max() / np.abs(ref).max()
            worst = max(worst, dev)
            assert dev <= 1e-10, ((p, d, q), dev)
    print(f"psi weights against lfilter: worst={worst:.3g}")


def test_holdout_forecast_is_the_pinned_validation_forecast():
    """(2) Fitting on the first 117 weeks and forecasting 40 gives the
    validation MSE of ``batched_fit_reference`` to 1e-12 relative: the
    two differ at most in summation order."""
    y, exog = gk._panel()
    S = gk.S_EVAL
    for order in [(1, 1, 1), (0, 2, 1), (2, 0, 1)]:
        fc, se, s2 = batched_forecast_reference(y[:8, :S], exog[:S],
                                                exog[S:], order)
        assert fc.shape == se.shape == (8, T_FULL - S) and s2.shape == (8,)
        mse = ((y[:8, S:] - fc) ** 2).mean(axis=1)
        ref = batched_fit_reference(y[:8], exog, [order], S)[:, 0]
        assert np.abs(mse - ref).max() <= 1e-12 * np.abs(ref).max(), order
        assert (s2 > 0).all() and (se > 0).all()
        assert (np.diff(se, axis=1) >= 0).all()


def test_sarimax_results_describe_the_same_quantities():
    """(3) ``SARIMAXResults.psi_weights`` / ``sigma2`` / ``forecast_se``
    are the batched oracle's formulas at that result's own phi, theta, d
    and eps."""
    y, exog = gk._panel()
    for order in [(2, 1, 2), (0, 2, 1), (1, 0, 0), (0, 1, 0), (4, 1, 2)]:
        p, d, q = order
        res = SARIMAX(y[3], exog=exog, order=order).fit()
        psi = psi_weights_reference(res.phi, res.theta, d, H_MAX)
        assert np.allclose(res.psi_weights(H_MAX), psi, rtol=1e-12, atol=0)
        m = max(p, q)
        s2 = (res.eps[m:] ** 2).sum() / (T_FULL - d - m)
        assert res.sigma2 == pytest.approx(s2, rel=1e-12)
        se = np.sqrt(s2 * np.cumsum(psi * psi))
        assert np.allclose(res.forecast_se(H_MAX), se, rtol=1e-12, atol=0)
        assert res.forecast_se(1)[0] == pytest.approx(np.sqrt(s2), rel=1e-12)


def test_f32_oracle_keeps_a_tenth_of_every_forecast_bound():
    """(4) The f32 oracle (numpy on the CPU) stays within ONE TENTH of
    every bound the GPU tests below assert, from given coefficients and
    end to end. Where the end-to-end GPU test allows a share of the
    groups out, the f32 oracle leaves out no more than ``F32_E2E_OUT``
    records, and above the GPU bound itself no more than it does for the
    validation MSE (2 at (4,1,2), 1 at (2,0,2), 0 elsewhere).

    Measured (numpy 2.2, f32 against f64 over the 130 groups, H = 40).
    From given coefficients: forecast at most 8.49e-7 of mean|y| over the
    d <= 1 orders, 8.76e-5 at (0,2,1) and 5.96e-5 at (1,2,1); sigma2 at
    most 1.08e-6; forecast_se at most 4.86e-7 for d = 0, 1.8e-6 for the
    pure-AR / single-MA d = 1 orders, 1.37e-5 (1,1,1), 1.40e-5 (4,1,2),
    1.69e-5 (2,1,2), 1.2e-6 (0,2,1) and 8.63e-5 (1,2,1). End to end,
    forecast as a fraction of mean|y|: <= 1.82e-7 for the pure-AR /
    single-MA d <= 1 orders, 7.89e-5 (1,1,1), 7.73e-3 (2,0,1), 8.80e-5
    (0,2,1), 5.95e-5 (1,2,1), 2.29e-3 (2,1,2), 1.09e-3 (4,1,2) and at
    (2,0,2) 6.10e-3 in one group, 1.97e-4 in the other 129."""
    y, exog = gk._panel()
    for order in ALL:
        params = gk._f32_oracle_final(order)[1]
        lanes = (order,) * G_FULL
        ref = _from_params(y, lanes, params, H_MAX)
        got = _from_params(y, lanes, params, H_MAX, dtype=np.float32)
        assert all(a.dtype == np.float32 for a in got)
        fc, s2, se = (a.max() for a in _deviations(got, ref, y))
        print(f"f32 oracle from params {order}: forecast={fc:.3g} of "
              f"mean|y| sigma2={s2:.3g} se={se:.3g}")
        assert fc <= _fc_bound(order) / 10, (order, fc)
        assert s2 <= SIGMA2_BOUND / 10, (order, s2)
        assert se <= SE_BOUND[order[1]] / 10, (order, se)

    r32 = _e2e_reference("float32")
    for order in ALL:
        assert r32[order].dtype == np.float32
        dev = _e2e_dev(r32[order], order)
        bound = _e2e_bound(order)
        over_tenth = int((dev > bound / 10).sum())
        over = int((dev > bound).sum())
        print(f"f32 oracle end to end {order}: worst={dev.max():.3g} "
              f">{bound / 10:g}: {over_tenth}  >{bound:g}: {over}")
        allow_tenth, allow = F32_E2E_OUT.get(order, (0, 0))
        assert over_tenth <= allow_tenth, (order, over_tenth)
        assert over <= allow, (order, over)
        # no more left out than for the validation MSE today
        assert allow <= gk.F32_ORACLE_OUT.get(order, (0, 0))[1], order
        # what the GPU test lets out covers what f32 costs
        gpu_allow = G_FULL - E2E_MIN_GROUPS if order in gk.CAPPED else 0
        assert allow <= gpu_allow, order


def test_forecast_gpu_validates_on_the_host():
    """(5) Every shape error raises ValueError before any GPU call."""
    y, exog = gk._panel()
    y = y[:4]
    fx = _future_exog(7)
    best = np.tile(np.array([[1, 1, 1]], dtype=np.int32), (4, 1))
    params = np.zeros((4, NPAR), dtype=np.float32)
    bad = [
        dict(future_exog=fx[:, :2]),                    # KX mismatch
        dict(exog=exog[:-1]),                           # exog rows != T
        dict(future_exog=fx[:0]),                       # H < 1
        dict(params=params[:, :-1]),                    # params columns
        dict(params=params[:3]),                        # params rows
        dict(best_order=best[:, :2]),                   # best_order columns
        dict(best_order=best[:3]),                      # best_order rows
    ]
    for change in bad:
        kw = dict(y=y, exog=exog, future_exog=fx, best_order=best,
                  params=params)
        kw.update(change)
        with pytest.raises(ValueError):
            batched_forecast_gpu(**kw)


def test_pandas_path_appends_future_rows_and_intervals():
    """(6) 2 groups, max_evals=3, forecast_steps=4, interval=0.9."""
    df = generate_demand_data(n_products=1, skus_per_product=2, n_weeks=120)
    T, H = 120, 4
    base = run_fine_grained_forecast(df, num_workers=1, max_evals=3)
    out = run_fine_grained_forecast(df, num_workers=1, max_evals=3,
                                    forecast_steps=H, interval=0.9)
    assert list(base.columns) == ["Product", "SKU", "Date", "Demand",
                                  "Demand_Fitted"]
    assert list(out.columns) == list(base.columns) + ["Demand_Lower",
                                                      "Demand_Upper"]
    assert len(base) == 2 * T and len(out) == 2 * (T + H)
    hist_rows = []
    for sku, grp in out.groupby("SKU", sort=True):
        grp = grp.sort_values("Date")
        assert len(grp) == T + H
        hist, fut = grp.iloc[:T], grp.iloc[T:]
        assert (np.diff(fut["Date"].to_numpy())
                == np.timedelta64(7, "D")).all()
        assert fut["Date"].iloc[0] - hist["Date"].iloc[-1] == \
            pd.Timedelta(days=7)
        assert fut["Demand"].isna().all() and hist["Demand"].notna().all()
        assert (fut["Demand_Lower"] < fut["Demand_Fitted"]).all()
        assert (fut["Demand_Fitted"] < fut["Demand_Upper"]).all()
        assert hist["Demand_Lower"].isna().all()
        assert hist["Demand_Upper"].isna().all()
        hist_rows.append(hist[list(base.columns)])
    # history rows are today's frame, and so is the default call
    got = pd.concat(hist_rows).sort_values(["SKU", "Date"]).reset_index(
        drop=True)
    want = base.sort_values(["SKU", "Date"]).reset_index(drop=True)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    again = run_fine_grained_forecast(df, num_workers=1, max_evals=3,
                                      forecast_steps=0, interval=None)
    pd.testing.assert_frame_equal(again, base, check_exact=True)
    for kw in (dict(forecast_steps=-1), dict(interval=1.0),
               dict(interval=0.0)):
        with pytest.raises(ValueError):
            run_fine_grained_forecast(df, num_workers=1, max_evals=3, **kw)


def test_forecast_endpoint_returns_future_rows():
    """(7) ``/forecast`` on the CPU app: 2 x (60 + 3) rows with
    forecast_steps=3; 400 for negative steps and an interval outside
    (0, 1)."""
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from mi355x_scale.serve import create_app
    rng = np.random.default_rng(1)
    dates = pd.date_range("2021-01-04", periods=60, freq="W-MON")
    records = []
    for sku in ("A", "B"):
        demand = 100 + rng.normal(0, 5, 60).cumsum()
        for d, v in zip(dates, demand):
            records.append({"Product": "P1", "SKU": sku,
                            "Date": str(d.date()), "Demand": float(v)})
    app = create_app(model_name="resnet18", num_classes=10, device="cpu")
    with TestClient(app) as client:
        r = client.post("/forecast", json={
            "records": records, "horizon": 10, "forecast_steps": 3,
            "interval": 0.9})
        assert r.status_code == 200
        rows = r.json()["rows"]
        assert len(rows) == 2 * (60 + 3)
        future = [row for row in rows if row["Demand"] is None]
        assert len(future) == 6
        for row in future:
            assert row["Date"] > str(dates[-1].date())
            assert row["Demand_Lower"] < row["Demand_Fitted"] \
                < row["Demand_Upper"]
        for bad in ({"forecast_steps": -1}, {"interval": 1.5}):
            r = client.post("/forecast", json={
                "records": records, "horizon": 10, **bad})
            assert r.status_code == 400, bad


# ------------------------------------------------------------------- GPU
KEYS = ("forecast", "forecast_se", "sigma2", "status")


@functools.lru_cache(maxsize=None)
def _forecast(lane_orders, H=H_MAX, use_mfma=True, nan=False):
    """groupfit_forecast through the extension, one order per lane, on
    the first len(lane_orders) rows of the panel and on the ``params``
    that ``groupfit_final`` wrote for the same lanes. Outputs in canaried
    buffers, canaries asserted after the launch."""
    import torch
    from mi355x_scale.forecast.batched import _designs_to_gpu, _to_yT
    from mi355x_scale.ops import _C
    G = len(lane_orders)
    params = gk._final(lane_orders, use_mfma, nan)["params"]
    yT = _to_yT(gk._panel_rows(G, nan), "cuda")
    xs, _ = _designs_to_gpu(_stacked(H), "cuda")
    best = torch.tensor(list(lane_orders), dtype=torch.int32,
                        device="cuda").reshape(G, 3).contiguous()
    bufs = gk._Bufs()
    fc = bufs.out("forecast", (H, G))
    se = bufs.out("forecast_se", (H, G))
    s2 = bufs.out("sigma2", (G,))
    st = bufs.out("status", (G,), torch.uint8)
    _C.groupfit_forecast(yT, xs[0], xs[1], xs[2], best,
                         torch.tensor(params, device="cuda"), fc, se, s2, st)
    bufs.check()
    res = dict(forecast=gk._np(fc).T.copy(), forecast_se=gk._np(se).T.copy(),
               sigma2=gk._np(s2), status=gk._np(st), params=params)
    for a in res.values():
        a.setflags(write=False)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
@pytest.mark.parametrize("order", ALL, ids=str)
def test_gpu_forecast_matches_its_own_coefficients(order, use_mfma):
    """(a) One order on all 130 lanes, H = 40, on the params that
    ``groupfit_final`` wrote in the same configuration. status 1;
    forecast within 8.5e-6 (d <= 1) / 8.8e-4 (d = 2) x mean|y_g|, sigma2
    within 1.1e-5 and forecast_se within 4.9e-6 / 1.7e-4 / 8.7e-4 (d = 0,
    1, 2) relative of the f64 oracle run from the kernel's own params on
    the design as the kernel read it; forecast_se strictly increasing in
    h for d >= 1 and non-decreasing for d = 0.

    Measured on an MI355X, the same with and without the MFMA stage 1 (in
    brackets the f32 oracle on the CPU). Forecast: 1.2e-7..1.4e-7 of
    mean|y| at the pure-AR / single-MA d <= 1 orders, 2.7e-7 (2,0,1),
    5.5e-7 (4,1,2), 6.4e-7 (1,1,1), 7.8e-7 (2,1,2), 9.0e-7 (2,0,2) [worst
    8.5e-7]; 8.4e-5 (0,2,1) [8.8e-5], 6.3e-5 (1,2,1) [6.0e-5]. sigma2 at
    most 8.2e-7 for d <= 1 and 1.5e-6 at (1,2,1) [1.1e-6]. forecast_se
    5.1e-7 for d = 0 [4.9e-7], 1.72e-5 for d = 1 [1.69e-5], 7.9e-5 for
    d = 2 [8.6e-5]."""
    lanes = (order,) * G_FULL
    res = _forecast(lanes, H_MAX, use_mfma)
    y = gk._panel()[0]
    assert res["status"].tolist() == [1] * G_FULL
    ref = _from_params(y, lanes, res["params"], H_MAX)
    fc, s2, se = _deviations(
        (res["forecast"], res["forecast_se"], res["sigma2"]), ref, y)
    print(f"groupfit_forecast {order} mfma={use_mfma}: "
          f"forecast={fc.max():.3g} of mean|y| sigma2={s2.max():.3g} "
          f"se={se.max():.3g}")
    assert (fc <= _fc_bound(order)).all(), (int(fc.argmax()), fc.max())
    assert (s2 <= SIGMA2_BOUND).all(), (int(s2.argmax()), s2.max())
    assert (se <= SE_BOUND[order[1]]).all(), (int(se.argmax()), se.max())
    step = np.diff(res["forecast_se"], axis=1)
    assert (step > 0).all() if order[1] >= 1 else (step >= 0).all()
    assert (res["forecast_se"][:, 0] > 0).all()


@pytest.mark.gpu
def test_gpu_forecast_mixed_order_waves_equal_uniform_launches():
    """(b) best_order[g] = ALL[g % 12]: d = 0, 1 and 2 side by side in
    every wave. Each lane gets the bits of the launch where all 130 lanes
    run its order."""
    mixed = _forecast(gk._mixed_orders(G_FULL))
    assert mixed["status"].tolist() == [1] * G_FULL
    for ci, order in enumerate(ALL):
        uni = _forecast((order,) * G_FULL)
        rows = np.arange(ci, G_FULL, len(ALL))
        for k in KEYS:
            assert np.array_equal(mixed[k][rows], uni[k][rows]), (order, k)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 63, 65])
def test_gpu_forecast_grid_tail_is_bit_exact_and_in_bounds(G):
    """(c) Clamped tail lanes: the first G rows alone give the bits of
    the 130-group run; the canaries after all four outputs are asserted
    inside the runner."""
    full = _forecast(gk._mixed_orders(G_FULL))
    part = _forecast(gk._mixed_orders(G))
    for k in KEYS:
        assert part[k].shape[0] == G
        assert np.array_equal(part[k], full[k][:G]), k


@pytest.mark.gpu
def test_gpu_forecast_is_independent_of_the_horizon():
    """(d) H = 1 and H = 7 are the first columns of H = 40 on the same
    params; sigma2 is the same in all three."""
    lanes = gk._mixed_orders(G_FULL)
    full = _forecast(lanes, H_MAX)
    for H in HORIZONS[:-1]:
        part = _forecast(lanes, H)
        assert part["forecast"].shape == (G_FULL, H)
        for k in ("forecast", "forecast_se"):
            assert np.array_equal(part[k], full[k][:, :H]), (H, k)
        assert np.array_equal(part["sigma2"], full["sigma2"]), H
        assert np.array_equal(part["status"], full["status"]), H


@pytest.mark.gpu
def test_gpu_forecast_non_finite_series_fails_alone():
    """(e) y[65, 10] = nan: group 65 has status 0, every other group
    keeps its bits."""
    lanes = gk._mixed_orders(G_FULL)
    got, clean = _forecast(lanes, nan=True), _forecast(lanes)
    keep = np.arange(G_FULL) != 65
    assert got["status"][65] == 0
    assert clean["status"].tolist() == [1] * G_FULL
    for k in KEYS:
        assert np.array_equal(got[k][keep], clean[k][keep]), k


@functools.lru_cache(maxsize=None)
def _driver(orders, use_mfma=True):
    """``batched_fit_gpu`` with and without ``future_exog``, as numpy."""
    from mi355x_scale.forecast.batched import batched_fit_gpu
    y, exog = gk._panel()
    plain = batched_fit_gpu(y, exog, list(orders), gk.S_EVAL,
                            use_mfma=use_mfma)
    with_fc = batched_fit_gpu(y, exog, list(orders), gk.S_EVAL,
                              use_mfma=use_mfma, future_exog=_future_exog())
    return ({k: gk._np(v) for k, v in plain.items()},
            {k: gk._np(v) for k, v in with_fc.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("use_mfma", [True, False])
def test_gpu_driver_forecast_changes_nothing_else(use_mfma):
    """(f) ``batched_fit_gpu(..., future_exog=F)`` over the production
    orders: every key of the plain call has the same bits, and the
    forecast keys are those of ``batched_forecast_gpu`` on the returned
    params."""
    plain, with_fc = _driver(tuple(gk.PROD), use_mfma)
    assert set(with_fc) == set(plain) | {"forecast", "forecast_se",
                                         "sigma2", "forecast_status"}
    for k in plain:
        assert np.array_equal(plain[k], with_fc[k]), k
    assert with_fc["forecast"].shape == (G_FULL, H_MAX)
    assert with_fc["forecast_status"].tolist() == [1] * G_FULL
    y, exog = gk._panel()
    later = batched_forecast_gpu(y, exog, _future_exog(),
                                 with_fc["best_order"], with_fc["params"])
    for k in ("forecast", "forecast_se", "sigma2"):
        assert np.array_equal(gk._np(later[k]), with_fc[k]), k
    assert np.array_equal(gk._np(later["status"]),
                          with_fc["forecast_status"])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ALL, ids=str)
def test_gpu_driver_forecast_against_the_end_to_end_oracle(order):
    """(f) One candidate, so every group runs ``order``: fit + forecast
    on the GPU against the f64 ``batched_forecast_reference``, H = 40.
    Conditioning-limited like the validation MSE: within 10x the f32
    oracle's figure for that order (``E2E_F32``) x mean|y_g|, for all 130
    groups outside ``gk.CAPPED`` and for >= 120 of 130 inside.

    Measured on an MI355X (in brackets the f32 oracle on the CPU), worst
    group: 1.1e-7..2.2e-7 at the pure-AR / single-MA d <= 1 orders
    [1.3e-7..1.8e-7], (1,1,1) 3.1e-5 [7.9e-5], (2,0,1) 1.3e-2 [7.7e-3],
    (0,2,1) 8.4e-5 [8.8e-5], (1,2,1) 1.0e-4 [6.0e-5], (2,1,2) 2.8e-3
    [2.3e-3], (4,1,2) 6.0e-4 [1.1e-3]; (2,0,2) 129 of 130 within 2e-3,
    worst 9.1e-3 [129, 6.1e-3]."""
    _, with_fc = _driver((order,))
    assert (with_fc["best_order"] == np.array(order)).all()
    dev = _e2e_dev(with_fc["forecast"], order)
    bound = _e2e_bound(order)
    ok = int((dev <= bound).sum())
    above = np.nonzero(dev > bound / 10)[0].tolist()
    print(f"batched_fit_gpu forecast {order}: worst={dev.max():.3g} of "
          f"mean|y| within={ok} >{bound / 10:g}: {above}")
    need = E2E_MIN_GROUPS if order in gk.CAPPED else G_FULL
    assert ok >= need, (order, ok, dev.max())


@pytest.mark.gpu
def test_gpu_frame_appends_future_rows_and_intervals():
    """(g) ``run_fine_grained_forecast_gpu(df, forecast_steps=8,
    interval=0.9)`` on 8 groups x 157 weeks."""
    from statistics import NormalDist
    from mi355x_scale.forecast.batched import batched_fit_gpu
    from mi355x_scale.forecast.pipeline import (DEFAULT_GPU_ORDERS,
                                                run_fine_grained_forecast_gpu)
    from mi355x_scale.groupby.gather import panel_from_long
    df = generate_demand_data(2, 4, T_FULL)
    H = 8
    base = run_fine_grained_forecast_gpu(df)
    out = run_fine_grained_forecast_gpu(df, forecast_steps=H, interval=0.9)
    assert len(base) == 8 * T_FULL and len(out) == 8 * (T_FULL + H)
    assert list(out.columns) == list(base.columns) + ["Demand_Lower",
                                                      "Demand_Upper"]
    y, _, dates = panel_from_long(df, ["Product", "SKU"], "Date", "Demand")
    exog = add_exo_variables(
        pd.DataFrame({"Date": pd.to_datetime(dates)}))[EXO_COLS].to_numpy()
    fx = add_exo_variables(pd.DataFrame(
        {"Date": _future_dates(dates, H)}))[EXO_COLS].to_numpy()
    fit = batched_fit_gpu(y, exog, DEFAULT_GPU_ORDERS, T_FULL - 40,
                          future_exog=fx)
    fc = gk._np(fit["forecast"]).astype(np.float64)
    se = gk._np(fit["forecast_se"]).astype(np.float64)
    z = NormalDist().inv_cdf(0.95)
    hist_rows = []
    groups = out.groupby(["Product", "SKU"], sort=True, observed=True)
    assert len(groups) == 8
    for g, (_, grp) in enumerate(groups):
        assert len(grp) == T_FULL + H
        assert grp["Date"].is_monotonic_increasing
        hist, fut = grp.iloc[:T_FULL], grp.iloc[T_FULL:]
        assert (np.diff(grp["Date"].to_numpy()[-H - 1:])
                == np.timedelta64(7, "D")).all()
        assert fut["Demand"].isna().all() and hist["Demand"].notna().all()
        assert np.array_equal(fut["Demand_Fitted"].to_numpy(), fc[g])
        assert np.array_equal(fut["Demand_Lower"].to_numpy(),
                              fc[g] - z * se[g])
        assert np.array_equal(fut["Demand_Upper"].to_numpy(),
                              fc[g] + z * se[g])
        assert (fut["Demand_Lower"] < fut["Demand_Fitted"]).all()
        assert (fut["Demand_Fitted"] < fut["Demand_Upper"]).all()
        assert hist["Demand_Lower"].isna().all()
        assert hist["Demand_Upper"].isna().all()
        hist_rows.append(hist[list(base.columns)])
    pd.testing.assert_frame_equal(
        pd.concat(hist_rows).reset_index(drop=True),
        base.reset_index(drop=True), check_exact=True)
