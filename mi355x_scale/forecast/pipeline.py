"""W1 per-SKU demand-forecast pipeline.

Native equivalent of the reference's notebook functions
(``group_apply/02_Fine_Grained_Demand_Forecasting.py``):

  * ``add_exo_variables``      (ref :343-358) — covid/christmas/new_year
    exogenous indicator columns from the Date column.
  * ``split_train_score_data`` (ref :372-380) — last ``forecast_horizon``
    weeks held out for scoring.
  * ``evaluate_model``         (ref :264-282) — fit candidate (p,d,q),
    MSE on the held-out window.
  * ``build_tune_and_score_model`` (ref :417-494) — per-group: sort by
    date, split, nested sequential TPE over (p,d,q) ∈ [0,4]×[0,2]×[0,4]
    with ``max_evals=10`` (ref :461-469), refit best on train+score,
    one-step-ahead fit over the full range, return the forecast frame.

Used two ways: through the ``groupby`` engine (pandas path, config 1) and
as the semantics reference for the batched GPU fit (``batched.py``).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import pandas as pd

from ..tune import Trials, fmin, hp, scope, tpe
from .sarimax import SARIMAX

FORECAST_HORIZON = 40  # weeks, ref :341
EXO_COLS = ["covid", "christmas", "new_year"]

TUNING_SCHEMA = ("Product string, SKU string, Date date, Demand float, "
                 "Demand_Fitted float")

SEARCH_SPACE = {
    "p": scope.int(hp.quniform("p", 0, 4, 1)),
    "d": scope.int(hp.quniform("d", 0, 2, 1)),
    "q": scope.int(hp.quniform("q", 0, 4, 1)),
}


def add_exo_variables(pdf: pd.DataFrame) -> pd.DataFrame:
    """Compute the three exogenous indicators from Date (ref :343-358)."""
    out = pdf.copy()
    date = pd.to_datetime(out["Date"])
    covid_start = pd.Timestamp("2020-03-01")
    weeks_since = ((date - covid_start).dt.days // 7)
    in_covid = (weeks_since >= 0) & (weeks_since < 16)
    out["covid"] = np.where(in_covid,
                            np.exp(-0.25 * weeks_since.clip(lower=0)), 0.0)
    out["christmas"] = ((date.dt.month == 12) & (date.dt.day >= 18)).astype(float)
    out["new_year"] = ((date.dt.month == 1) & (date.dt.day <= 7)).astype(float)
    return out


def split_train_score_data(pdf: pd.DataFrame,
                           horizon: int = FORECAST_HORIZON
                           ) -> Tuple[pd.DataFrame, pd.DataFrame]:
    """Last ``horizon`` rows are the score window (ref :372-380)."""
    return pdf.iloc[:-horizon], pdf.iloc[-horizon:]


def evaluate_model(params: Dict, train: pd.DataFrame, score: pd.DataFrame,
                   exo_cols=EXO_COLS) -> Dict:
    """Fit (p,d,q) on train, forecast the score window, return MSE loss
    (ref evaluate_model :435-459)."""
    from ..tune import STATUS_FAIL, STATUS_OK
    p, d, q = int(params["p"]), int(params["d"]), int(params["q"])
    try:
        res = SARIMAX(train["Demand"].to_numpy(),
                      exog=train[exo_cols].to_numpy(),
                      order=(p, d, q)).fit(disp=False)
        fc = res.forecast(len(score), exog=score[exo_cols].to_numpy())
        mse = float(np.mean((score["Demand"].to_numpy() - fc) ** 2))
        if not np.isfinite(mse):
            return {"loss": None, "status": STATUS_FAIL}
        return {"loss": mse, "status": STATUS_OK}
    except Exception:
        return {"loss": None, "status": STATUS_FAIL}


def _check_forecast_args(forecast_steps, interval) -> int:
    """Validate the two forecast keywords; returns the horizon H."""
    H = int(forecast_steps)
    if H < 0:
        raise ValueError(f"forecast_steps must be >= 0, got {forecast_steps}")
    if interval is not None and not 0.0 < float(interval) < 1.0:
        raise ValueError(f"interval must be in (0, 1), got {interval}")
    return H


def _future_dates(dates, H: int) -> pd.DatetimeIndex:
    """H dates past the last one, at the spacing of the last two."""
    d = pd.DatetimeIndex(pd.to_datetime(dates))
    return pd.DatetimeIndex(d[-1] + (d[-1] - d[-2]) * np.arange(1, H + 1))


def _interval_z(interval: float) -> float:
    """Two-sided normal quantile: the interval is forecast -/+ z * se."""
    from statistics import NormalDist
    return NormalDist().inv_cdf(0.5 + float(interval) / 2.0)


def build_tune_and_score_model(sku_pdf: pd.DataFrame,
                               horizon: int = FORECAST_HORIZON,
                               max_evals: int = 10,
                               seed: int = 123,
                               forecast_steps: int = 0,
                               interval: Optional[float] = None
                               ) -> pd.DataFrame:
    """The applyInPandas group function (ref :417-494): returns a frame
    matching TUNING_SCHEMA with one-step-ahead fitted demand. With
    ``forecast_steps > 0`` that many future rows follow (dates continue at
    the spacing of the last two, Demand is NaN, Demand_Fitted holds the
    forecast); with ``interval`` in (0,1) the columns Demand_Lower /
    Demand_Upper hold forecast -/+ z * se on the future rows and NaN on
    the history rows."""
    H = _check_forecast_args(forecast_steps, interval)
    pdf = sku_pdf.sort_values("Date").reset_index(drop=True)
    train, score = split_train_score_data(pdf, horizon)

    trials = Trials()
    fmin(lambda prm: evaluate_model(prm, train, score),
         SEARCH_SPACE, algo=tpe.suggest, max_evals=max_evals,
         trials=trials, rstate=np.random.default_rng(seed))
    bt = trials.best_trial["misc"]["vals"]
    p, d, q = int(bt["p"][0]), int(bt["d"][0]), int(bt["q"][0])

    # final refit on the whole series (ref :472-481)
    res = SARIMAX(pdf["Demand"].to_numpy(),
                  exog=pdf[EXO_COLS].to_numpy(),
                  order=(p, d, q)).fit(disp=False)
    T = len(pdf)
    dates = pd.to_datetime(pdf["Date"])
    demand = pdf["Demand"].astype(float)
    product, sku = pdf["Product"], pdf["SKU"]
    if H > 0:
        fdates = _future_dates(dates, H)
        future = add_exo_variables(
            pd.DataFrame({"Date": fdates}))[EXO_COLS].to_numpy()
        fitted = res.predict(0, T - 1 + H, exog=future)
        dates = pd.concat([dates, pd.Series(fdates)], ignore_index=True)
        demand = pd.concat([demand, pd.Series(np.full(H, np.nan))],
                           ignore_index=True)
        product = pd.Series([product.iloc[0]] * (T + H))
        sku = pd.Series([sku.iloc[0]] * (T + H))
    else:
        fitted = res.predict(0, T - 1)
    out = pd.DataFrame({
        "Product": product,
        "SKU": sku,
        "Date": dates,
        "Demand": demand,
        "Demand_Fitted": fitted,
    })
    if interval is not None:
        half = np.full(T + H, np.nan)
        if H > 0:
            half[T:] = _interval_z(interval) * res.forecast_se(H)
        out["Demand_Lower"] = out["Demand_Fitted"] - half
        out["Demand_Upper"] = out["Demand_Fitted"] + half
    return out


def _forecast_schema(interval) -> str:
    if interval is None:
        return TUNING_SCHEMA
    return TUNING_SCHEMA + ", Demand_Lower float, Demand_Upper float"


DEFAULT_GPU_ORDERS = [(0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 1, 1),
                      (1, 1, 1), (2, 1, 0), (2, 0, 1), (0, 2, 1),
                      (2, 1, 2), (4, 1, 2)]


def run_fine_grained_forecast_gpu(demand_df: pd.DataFrame,
                                  orders=None,
                                  horizon: int = FORECAST_HORIZON,
                                  forecast_steps: int = 0,
                                  interval: Optional[float] = None
                                  ) -> pd.DataFrame:
    """W1 on the batched CDNA4 kernel: same input/output frames as
    ``run_fine_grained_forecast`` but every group is fitted on the GPU
    (candidate grid -> best-per-group -> final fit), ~10^6 groups/sec.
    ``forecast_steps`` and ``interval`` as in
    ``build_tune_and_score_model``: future rows from the forecast kernel,
    their exogenous indicators from ``add_exo_variables`` on the future
    dates.
    """
    from ..groupby.gather import long_from_panel, panel_from_long
    from .batched import batched_fit_gpu
    H = _check_forecast_args(forecast_steps, interval)
    # C++ group gather (the Spark-shuffle replacement): factorize + scatter
    y, gindex, dates = panel_from_long(demand_df, ["Product", "SKU"],
                                       "Date", "Demand")
    # exog indicators are a pure function of the week — compute on the T
    # unique dates, not by enriching/scanning the full long frame
    exog = add_exo_variables(
        pd.DataFrame({"Date": pd.to_datetime(dates)}))[EXO_COLS].to_numpy()
    T = y.shape[1]
    future_exog = None
    if H > 0:
        fdates = _future_dates(dates, H)
        future_exog = add_exo_variables(
            pd.DataFrame({"Date": fdates}))[EXO_COLS].to_numpy()
    out = batched_fit_gpu(y, exog, orders or DEFAULT_GPU_ORDERS,
                          train_len=T - horizon, future_exog=future_exog)
    demand = y.astype(np.float64)
    fitted = out["fitted"].cpu().numpy().astype(np.float64)
    cols = ["Product", "SKU", "Date", "Demand", "Demand_Fitted"]
    if H > 0:
        G = len(demand)
        dates = pd.DatetimeIndex(pd.to_datetime(dates)).append(
            fdates).to_numpy()
        demand = np.concatenate([demand, np.full((G, H), np.nan)], axis=1)
        fitted = np.concatenate(
            [fitted, out["forecast"].cpu().numpy().astype(np.float64)],
            axis=1)
    values = [("Demand", demand), ("Demand_Fitted", fitted)]
    if interval is not None:
        half = np.full(fitted.shape, np.nan)
        if H > 0:
            half[:, T:] = _interval_z(interval) * out[
                "forecast_se"].cpu().numpy().astype(np.float64)
        values += [("Demand_Lower", fitted - half),
                   ("Demand_Upper", fitted + half)]
        cols += ["Demand_Lower", "Demand_Upper"]
    res = long_from_panel(demand, gindex, dates, ["Product", "SKU"], "Date",
                          values)
    if not np.issubdtype(res["Date"].dtype, np.datetime64):
        # tiled tvals are already datetime64 for datetime inputs —
        # an unconditional to_datetime copied 15.7M timestamps (~0.11 s
        # of the 0.72 s end-to-end job) for nothing
        res["Date"] = pd.to_datetime(res["Date"])
    return res[cols]


def run_holtwinters_forecast_gpu(demand_df: pd.DataFrame,
                                 trend: Optional[str] = "add",
                                 damped_trend: bool = False,
                                 seasonal: Optional[str] = None,
                                 seasonal_periods: Optional[int] = None,
                                 forecast_steps: int = 0) -> pd.DataFrame:
    """Holt-Winters for every (Product, SKU) group on the batched GPU fit
    (the reference's single-series walkthrough, ref :143-188, at panel
    scale). Returns the TUNING_SCHEMA columns with one-step-ahead fitted
    demand; with ``forecast_steps > 0`` each group gets that many future
    rows appended (dates continue at the spacing of the last two, Demand
    is NaN, Demand_Fitted holds the forecast).
    """
    from ..groupby.gather import long_from_panel, panel_from_long
    from .batched_hw import batched_hw_fit_gpu
    y, gindex, dates = panel_from_long(demand_df, ["Product", "SKU"],
                                       "Date", "Demand")
    H = int(forecast_steps)
    out = batched_hw_fit_gpu(y, trend=trend, damped_trend=damped_trend,
                             seasonal=seasonal,
                             seasonal_periods=seasonal_periods,
                             forecast_steps=H)
    demand = y.astype(np.float64)
    fitted = out["fitted"].cpu().numpy().astype(np.float64)
    if H > 0:
        d = pd.DatetimeIndex(pd.to_datetime(dates))
        future = d[-1] + (d[-1] - d[-2]) * np.arange(1, H + 1)
        dates = d.append(pd.DatetimeIndex(future)).to_numpy()
        demand = np.concatenate(
            [demand, np.full((len(demand), H), np.nan)], axis=1)
        fitted = np.concatenate(
            [fitted, out["forecast"].cpu().numpy().astype(np.float64)],
            axis=1)
    res = long_from_panel(demand, gindex, dates, ["Product", "SKU"], "Date",
                          [("Demand", demand), ("Demand_Fitted", fitted)])
    if not np.issubdtype(res["Date"].dtype, np.datetime64):
        res["Date"] = pd.to_datetime(res["Date"])
    return res[["Product", "SKU", "Date", "Demand", "Demand_Fitted"]]


def _shard_of(product: str, sku: str, num_shards: int) -> int:
    """Deterministic group→shard assignment (stable across processes —
    md5, not the salted builtin hash)."""
    import hashlib
    h = hashlib.md5(f"{product}\x1f{sku}".encode()).digest()
    return int.from_bytes(h[:4], "little") % num_shards


def run_fine_grained_forecast_sharded(
    demand_df: pd.DataFrame,
    out_dir: str,
    num_shards: int = 16,
    engine: str = "auto",
    resume: bool = True,
    cur_rank: int = 0,
    world_size: int = 1,
    horizon: int = FORECAST_HORIZON,
    orders=None,
    max_evals: int = 10,
    forecast_steps: int = 0,
    interval: Optional[float] = None,
) -> list:
    """W1 with restartable per-group-shard Parquet output.

    The reference persists the forecast frame to storage
    (``group_apply/02_Fine_Grained_Demand_Forecasting.py:544-552``,
    Delta write) so a failed job keeps its finished work; SURVEY §5.4
    calls the group-shard output "naturally restartable". Here: groups
    are hashed into ``num_shards`` deterministic shards; each shard's
    forecast frame is written as ``shard-NNNNN.parquet`` via tmp-file +
    atomic rename, so a file's existence means it is complete. A rerun
    (``resume=True``) skips finished shards without refitting them and
    produces byte-identical output. Multi-worker: rank r owns shards
    r, r+world_size, ... (the reader-sharding convention).

    ``forecast_steps`` / ``interval`` are passed to the engine (future
    rows and interval columns in every shard).

    Returns the ordered list of shard paths.
    """
    import os

    _check_forecast_args(forecast_steps, interval)

    os.makedirs(out_dir, exist_ok=True)
    if engine == "auto":
        try:
            import torch
            engine = "gpu" if torch.cuda.is_available() else "pandas"
        except Exception:
            engine = "pandas"

    keys = demand_df[["Product", "SKU"]].drop_duplicates()
    shard_ids = {
        (r.Product, r.SKU): _shard_of(r.Product, r.SKU, num_shards)
        for r in keys.itertuples(index=False)
    }
    shard_col = pd.Series(
        [shard_ids[k] for k in zip(demand_df["Product"],
                                   demand_df["SKU"])],
        index=demand_df.index)

    paths = []
    for s in range(num_shards):
        path = os.path.join(out_dir, f"shard-{s:05d}.parquet")
        paths.append(path)
        if s % world_size != cur_rank:
            continue
        if resume and os.path.exists(path):
            continue
        part = demand_df[shard_col == s]
        if len(part) == 0:
            frame = pd.DataFrame({
                "Product": pd.Series(dtype=str),
                "SKU": pd.Series(dtype=str),
                "Date": pd.Series(dtype="datetime64[ns]"),
                "Demand": pd.Series(dtype=float),
                "Demand_Fitted": pd.Series(dtype=float),
            })
            if interval is not None:
                frame["Demand_Lower"] = pd.Series(dtype=float)
                frame["Demand_Upper"] = pd.Series(dtype=float)
        elif engine == "gpu":
            frame = run_fine_grained_forecast_gpu(
                part, orders=orders, horizon=horizon,
                forecast_steps=forecast_steps, interval=interval)
        else:
            frame = run_fine_grained_forecast(
                part, max_evals=max_evals, horizon=horizon,
                forecast_steps=forecast_steps, interval=interval)
        # deterministic row order -> byte-identical reruns
        frame = frame.sort_values(["Product", "SKU", "Date"]
                                  ).reset_index(drop=True)
        tmp = f"{path}.tmp.{os.getpid()}"
        frame.to_parquet(tmp, index=False)
        os.replace(tmp, path)  # atomic: no partially-written shard files
    return paths


def read_forecast_shards(out_dir: str) -> pd.DataFrame:
    """Read back a sharded forecast output directory (finished shards
    only — ``.tmp`` files from a killed run are ignored)."""
    import glob
    import os
    parts = sorted(glob.glob(os.path.join(out_dir, "shard-*.parquet")))
    frames = [pd.read_parquet(p) for p in parts]
    if not frames:
        return pd.DataFrame(columns=["Product", "SKU", "Date", "Demand",
                                     "Demand_Fitted"])
    return pd.concat(frames, ignore_index=True)


def run_fine_grained_forecast(demand_df: pd.DataFrame,
                              num_workers: Optional[int] = None,
                              max_evals: int = 10,
                              horizon: int = FORECAST_HORIZON,
                              forecast_steps: int = 0,
                              interval: Optional[float] = None
                              ) -> pd.DataFrame:
    """The whole W1 job: enrich → group → tune+score per SKU (the
    reference's :520-528 chain) on the local process pool.
    ``forecast_steps`` / ``interval`` as in ``build_tune_and_score_model``.
    """
    from ..groupby import LocalFrame
    _check_forecast_args(forecast_steps, interval)
    if not set(EXO_COLS) <= set(demand_df.columns):
        demand_df = add_exo_variables(demand_df)
    n_groups = demand_df.groupby(["Product", "SKU"]).ngroups
    frame = LocalFrame(demand_df, num_workers=num_workers)
    return (frame.repartition(n_groups, "Product", "SKU")
                 .groupBy("Product", "SKU")
                 .applyInPandas(
                     lambda g: build_tune_and_score_model(
                         g, horizon=horizon, max_evals=max_evals,
                         forecast_steps=forecast_steps, interval=interval),
                     _forecast_schema(interval)))
