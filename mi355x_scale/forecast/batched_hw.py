"""Batched Holt-Winters (ExponentialSmoothing) fit — numpy oracle + GPU
driver.

The reference walkthrough fits four Holt-Winters variants per series
(``group_apply/02_Fine_Grained_Demand_Forecasting.py:143-188``);
``holtwinters.py`` reproduces them one series at a time. Here a whole
``[G, T]`` panel is fitted at once with the same fixed-schedule search:

  grid    itertools.product(alpha, beta, gamma, phi) over
          GRID = [0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9] (beta only with a
          trend, gamma only with a season) and PHIS = [0.8, 0.9, 0.98]
          (only when damped); first strict SSE minimum wins
  refine  two rounds over the 3x3 (alpha, beta) +-0.05 neighbourhood of
          the incumbent, clipped to [0.01, 0.99] / [0, 0.99], strict ``<``
  final   one pass at the winner: fitted values, end state, forecast

``batched_hw_reference`` is the vectorised numpy implementation (arrays
``[G, C]``, one numpy step per ``t``) — in f64 it equals
``ExponentialSmoothing(...).fit()`` per series, and it is the numerics
oracle for ``ops/csrc/hwfit.hip``. ``batched_hw_fit_gpu`` runs the search
and the final pass on the GPU, one group per lane.

Two behaviours the scalar class leaves to Python NaN comparisons are
defined here: a non-finite candidate SSE counts as +inf, and a group whose
best SSE is not finite gets ``status 0`` and NaN outputs.
"""
from __future__ import annotations

import itertools
from typing import Optional

import numpy as np

from .batched import _to_yT

GRID = (0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9)
PHIS = (0.8, 0.9, 0.98)
REFINE_STEPS = (-0.05, 0.0, 0.05)
REFINE_ROUNDS = 2
MAX_SEASONAL_PERIODS = 64
OUTPUT_KEYS = ("params", "sse", "fitted", "level", "trend", "season",
               "forecast", "status")


def _validate(y, trend, seasonal, seasonal_periods):
    if trend not in (None, "add"):
        raise ValueError("trend must be None or 'add'")
    if seasonal not in (None, "add", "mul"):
        raise ValueError("seasonal must be None, 'add' or 'mul'")
    m = 0
    if seasonal:
        if not seasonal_periods:
            raise ValueError("seasonal requires seasonal_periods")
        m = int(seasonal_periods)
        if m < 2 or m > MAX_SEASONAL_PERIODS:
            raise ValueError(
                f"seasonal_periods must be in [2, {MAX_SEASONAL_PERIODS}]")
    if y.ndim != 2:
        raise ValueError("y must be [G, T]")
    if y.shape[1] < 2:
        raise ValueError("need T >= 2")
    return m


def candidate_table(trend, damped_trend, seasonal) -> np.ndarray:
    """The coarse grid as a [C, 4] f64 table of (alpha, beta, gamma, phi)
    rows in ``itertools.product`` order (the scalar class's visit order)."""
    a_c = GRID
    b_c = GRID if trend else (0.0,)
    g_c = GRID if seasonal else (0.0,)
    p_c = PHIS if damped_trend else (1.0,)
    return np.array(list(itertools.product(a_c, b_c, g_c, p_c)),
                    dtype=np.float64)


def _params_arg(params, G):
    p = np.asarray(params, dtype=np.float64)
    if p.shape == (4,):
        p = np.broadcast_to(p, (G, 4))
    if p.shape != (G, 4):
        raise ValueError("params must be [G, 4] or one 4-tuple "
                         "(alpha, beta, gamma, phi)")
    return np.ascontiguousarray(p)


def _recursion(y, alpha, beta, gamma, phi, m, trend, seasonal,
               return_state=False):
    """One-step-ahead recursion for ``y [G,T]`` at parameters ``[G,C]``
    (or ``[1,C]``, broadcast over groups). Same operations in the same
    order as ``holtwinters._hw_sse``; everything runs in ``y.dtype``."""
    dt = y.dtype
    G, n = y.shape
    alpha, beta, gamma, phi = (np.asarray(p, dtype=dt)
                               for p in (alpha, beta, gamma, phi))
    C = alpha.shape[1]
    one = dt.type(1.0)
    tiny = dt.type(1e-9)
    if seasonal and n >= 2 * m:
        s0 = y[:, :m].mean(axis=1)
        b0 = ((y[:, m:2 * m].mean(axis=1) - s0) / dt.type(m) if trend
              else np.zeros(G, dtype=dt))
        j = np.arange(m, dtype=dt)
        base = s0[:, None] + b0[:, None] * (j - dt.type((m - 1) / 2.0))
        if seasonal == "mul":
            seas0 = y[:, :m] / np.maximum(base, tiny)
        else:
            seas0 = y[:, :m] - base
        lvl0 = s0
        mm = m
    else:
        lvl0 = y[:, 0]
        b0 = (y[:, 1] - y[:, 0]) if trend else np.zeros(G, dtype=dt)
        mm = m or 1
        seas0 = np.full((G, mm), 1.0 if seasonal == "mul" else 0.0,
                        dtype=dt)
    lvl = np.broadcast_to(lvl0[:, None], (G, C)).astype(dt)
    b = np.broadcast_to(b0[:, None], (G, C)).astype(dt)
    seas = np.broadcast_to(seas0[:, None, :], (G, C, mm)).astype(dt)
    sse = np.zeros((G, C), dtype=dt)
    fitted = np.empty((G, C, n), dtype=dt) if return_state else None
    with np.errstate(all="ignore"):
        for t in range(n):
            yt = y[:, t:t + 1]
            si = seas[:, :, t % mm].copy()
            if seasonal == "mul":
                yhat = (lvl + phi * b) * si
            else:
                yhat = lvl + phi * b + si
            if return_state:
                fitted[:, :, t] = yhat
            err = yt - yhat
            sse = sse + err * err
            prev = lvl
            if seasonal == "mul":
                des = yt / np.maximum(si, tiny)
            else:
                des = yt - si
            lvl = alpha * des + (one - alpha) * (prev + phi * b)
            if trend:
                b = beta * (lvl - prev) + (one - beta) * phi * b
            if seasonal == "mul":
                seas[:, :, t % mm] = (gamma * (yt / np.maximum(lvl, tiny))
                                      + (one - gamma) * si)
            elif seasonal:
                seas[:, :, t % mm] = gamma * (yt - lvl) + (one - gamma) * si
    if return_state:
        return sse, fitted, lvl, b, seas
    return sse


def _search(y, m, trend, damped_trend, seasonal):
    """Grid + refinement; returns (params [G,4] f64, best sse [G])."""
    G = y.shape[0]
    rows = np.arange(G)
    table = candidate_table(trend, damped_trend, seasonal)
    sse = _recursion(y, *(table[None, :, k] for k in range(4)),
                     m, trend, seasonal)
    sse = np.where(np.isfinite(sse), sse, np.inf)
    ci = np.argmin(sse, axis=1)          # first occurrence of the minimum
    best = sse[rows, ci]
    par = table[ci].copy()
    for _ in range(REFINE_ROUNDS):
        a0, b0 = par[:, 0].copy(), par[:, 1].copy()
        aa = np.stack([np.clip(a0 + da, 0.01, 0.99)
                       for da in REFINE_STEPS for _db in REFINE_STEPS], 1)
        bb = np.stack([np.clip(b0 + db, 0.0, 0.99)
                       for _da in REFINE_STEPS for db in REFINE_STEPS], 1)
        gg = np.repeat(par[:, 2:3], 9, axis=1)
        pp = np.repeat(par[:, 3:4], 9, axis=1)
        s = _recursion(y, aa, bb, gg, pp, m, trend, seasonal)
        s = np.where(np.isfinite(s), s, np.inf)
        for r in range(9):
            better = s[:, r] < best
            best = np.where(better, s[:, r], best)
            par[better, 0] = aa[better, r]
            par[better, 1] = bb[better, r]
    return par, best


def _forecast(level, trend_state, seas, phi, n, steps, trend, seasonal):
    """``HoltWintersResults.forecast`` for every group: [G, steps]."""
    G, mm = seas.shape
    out = np.empty((G, steps), dtype=level.dtype)
    with np.errstate(all="ignore"):
        for h in range(1, steps + 1):
            damp = np.where(phi == 1.0, phi * h,
                            phi * (1 - phi ** h) / (1 - phi))
            base = level + (damp * trend_state if trend else 0.0)
            si = seas[:, (n + h - 1) % mm]
            out[:, h - 1] = base * si if seasonal == "mul" else base + si
    return out


def batched_hw_reference(y, trend: Optional[str] = None,
                         damped_trend: bool = False,
                         seasonal: Optional[str] = None,
                         seasonal_periods: Optional[int] = None,
                         params=None, forecast_steps: int = 0,
                         dtype=np.float64) -> dict:
    """Holt-Winters fit of every row of ``y [G,T]`` — the CPU oracle.

    ``params=None`` runs the full search; ``params`` as ``[G,4]`` (or one
    4-tuple for all groups) of (alpha, beta, gamma, phi) skips it and runs
    the final pass at exactly those values. ``dtype`` is the arithmetic
    precision (f32 emulates the GPU kernel on the CPU).

    Returns a dict of numpy arrays: ``params [G,4]``, ``sse [G]``,
    ``fitted [G,T]``, ``level [G]``, ``trend [G]``, ``season [G,m]``
    (``m = 1`` without a season), ``forecast [G,forecast_steps]``,
    ``status [G]`` (u8; 0 = non-finite fit, outputs NaN).
    """
    dt = np.dtype(dtype)
    y = np.ascontiguousarray(np.asarray(y, dtype=dt))
    m = _validate(y, trend, seasonal, seasonal_periods)
    G, T = y.shape
    if params is None:
        par, _ = _search(y, m, trend, damped_trend, seasonal)
    else:
        par = _params_arg(params, G).copy()
    sse, fitted, lvl, b, seas = _recursion(
        y, *(par[:, k:k + 1] for k in range(4)), m, trend, seasonal,
        return_state=True)
    sse, fitted, lvl, b, seas = (sse[:, 0], fitted[:, 0], lvl[:, 0],
                                 b[:, 0], seas[:, 0])
    fc = _forecast(lvl, b, seas, par[:, 3].astype(dt), T,
                   int(forecast_steps), trend, seasonal)
    ok = np.isfinite(sse)
    bad = ~ok
    par = par.copy()
    out = {"params": par, "sse": sse, "fitted": fitted, "level": lvl,
           "trend": b, "season": seas, "forecast": fc}
    for v in out.values():
        v[bad] = np.nan
    out["status"] = ok.astype(np.uint8)
    return out


def batched_hw_fit_gpu(y, trend: Optional[str] = None,
                       damped_trend: bool = False,
                       seasonal: Optional[str] = None,
                       seasonal_periods: Optional[int] = None,
                       params=None, forecast_steps: int = 0,
                       device="cuda", search_waves: int = 0) -> dict:
    """Holt-Winters fit of every row of ``y [G,T]`` on the GPU.

    Same arguments and dict keys as ``batched_hw_reference``; the values
    are torch tensors on ``device``, ``[G, .]``-major (f32, ``status``
    u8). ``params=None`` runs ``hwfit_search`` then ``hwfit_final``;
    given ``params`` only ``hwfit_final`` runs. The search scores its
    candidates in f32; the final pass computes in f64 and rounds its
    outputs to f32.

    ``search_waves`` is the number of waves per block the candidate list
    is split across (0 = as many as the LDS budget allows, at most 16).
    The result does not depend on it.
    """
    import torch
    from ..ops import require_ext, _C
    require_ext()
    y_np = y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)
    m = _validate(y_np, trend, seasonal, seasonal_periods)
    G, T = y_np.shape
    H = int(forecast_steps)
    if H < 0:
        raise ValueError("forecast_steps must be >= 0")
    y32 = np.asarray(y_np, dtype=np.float32)
    if not y32.flags.writeable:
        y32 = y32.copy()      # torch will not wrap a read-only array
    yT = _to_yT(y32, device)
    has_trend = trend is not None
    seas_mode = {None: 0, "add": 1, "mul": 2}[seasonal]
    mm = m or 1
    f32 = dict(dtype=torch.float32, device=device)
    if params is None:
        table = torch.tensor(candidate_table(trend, damped_trend, seasonal),
                             **f32).contiguous()
        par = torch.empty((G, 4), **f32)
        s_sse = torch.empty((G,), **f32)
        s_status = torch.empty((G,), dtype=torch.uint8, device=device)
        _C.hwfit_search(yT, table, par, s_sse, s_status, has_trend,
                        seas_mode, mm, int(search_waves))
        par_in = par
    else:
        par_in = torch.tensor(_params_arg(params, G), **f32).contiguous()
    fitted = torch.empty((T, G), **f32)
    forecast = torch.empty((H, G), **f32)
    level = torch.empty((G,), **f32)
    trend_o = torch.empty((G,), **f32)
    season = torch.empty((mm, G), **f32)
    sse = torch.empty((G,), **f32)
    status = torch.empty((G,), dtype=torch.uint8, device=device)
    _C.hwfit_final(yT, par_in, fitted, forecast, level, trend_o, season,
                   sse, status, has_trend, seas_mode, mm)
    if params is not None:
        # supplied parameters of a failed group read NaN like its outputs
        par_in = torch.where(status[:, None] != 0, par_in,
                             torch.full_like(par_in, float("nan")))
    return {
        "params": par_in, "sse": sse, "fitted": fitted.t().contiguous(),
        "level": level, "trend": trend_o,
        "season": season.t().contiguous(),
        "forecast": forecast.t().contiguous(), "status": status,
    }
