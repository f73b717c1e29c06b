"""Batched per-group ARIMAX fitting — algorithm reference + GPU driver.

This is the N2 component: the reference fits one
statsmodels SARIMAX per Spark task per SKU
(``group_apply/02_Fine_Grained_Demand_Forecasting.py:441-450,472-481``);
here thousands of groups are fitted per kernel launch on one MI355X.

The fixed-schedule estimator (identical to ``sarimax.py`` per group, with
Yule-Walker/Levinson for the long-AR stage):

  stage 0  w = diff^d(y_train), centered; exog differenced+centered and
           its OLS pseudo-inverse P_d precomputed ON HOST (shared by all
           groups — the exog design matrix is date-only in W1)
  stage 1  beta = P_d @ w_c   (per group: a matvec; across groups: a
           GEMM);  u = w_c - Xc @ beta
  stage 2  long-AR via Yule-Walker autocovariances + Levinson-Durbin,
           innovations eps by recursion  (q>0 only)
  stage 3  OLS of u_t on [u lags (p), eps lags (q)] over t = m..n-1 —
           exact lag-matrix normal equations, ridge, Cholesky solve,
           stationarity/invertibility shrinkage
  stage 4  recompute eps under (phi, theta); redo stage 3 once
  stage 5  H-step validation forecast, integrated back to y-units; MSE

``batched_fit_reference`` is the vectorized-f64 numpy implementation —
the numerics oracle for the HIP kernel (``ops/csrc/groupfit.hip``), which
runs one group per lane, 64 groups per wave, series slabs in LDS,
time-major [T, G] global layout for coalescing.

Out-of-sample: ``forecast_from_params_reference`` /
``batched_forecast_reference`` define the H-step forecast, the innovation
variance and the psi-weight standard errors; ``batched_forecast_gpu``
(``groupfit_forecast_kernel``) computes them for a whole panel from the
stored ``params`` / ``best_order``, and ``batched_fit_gpu(...,
future_exog=F)`` fits and forecasts in one call.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAXP = 4
MAXQ = 4
MAXD = 2
LONG_AR_EXTRA = 3
RIDGE = 1e-6
SHRINK = 0.98


# --------------------------------------------------------------------------
# host-side shared precomputation
# --------------------------------------------------------------------------
@dataclass
class ExogDesign:
    """Per-d differenced/centered exog design + train pseudo-inverse."""
    d: int
    Xc_full: np.ndarray   # [T-d, KX] centered with TRAIN-window means
    P: np.ndarray         # [KX, n] with n = S-d (train rows)
    xmean: np.ndarray     # [KX]


def make_exog_designs(exog: np.ndarray, train_len: int,
                      ds: Sequence[int] = (0, 1, 2)) -> List[ExogDesign]:
    out = []
    X = np.asarray(exog, dtype=np.float64)
    for d in ds:
        Xd = X.copy()
        for _ in range(d):
            Xd = np.diff(Xd, axis=0)
        n = train_len - d
        xm = Xd[:n].mean(axis=0)
        Xc = Xd - xm
        XtX = Xc[:n].T @ Xc[:n]
        XtX[np.diag_indices_from(XtX)] += RIDGE * max(1.0, np.trace(XtX) / len(XtX))
        P = np.linalg.solve(XtX, Xc[:n].T)
        out.append(ExogDesign(d=d, Xc_full=Xc, P=P, xmean=xm))
    return out


def _levinson(r: np.ndarray, M: int, dtype=np.float64) -> np.ndarray:
    """Levinson-Durbin: AR(M) coefficients from autocovariances r[0..M]."""
    dt = np.dtype(dtype).type
    a = np.zeros(M, dtype=dtype)
    e = r[0] if r[0] > 0 else dt(1.0)
    for k in range(1, M + 1):
        acc = r[k] - np.dot(a[:k - 1], r[k - 1:0:-1])
        lam = acc / e
        prev = a[:k - 1].copy()
        a[k - 1] = lam
        a[:k - 1] = prev - lam * prev[::-1]
        e *= (dt(1.0) - lam * lam)
        if e <= 0:
            e = dt(1e-12)
    return a


def _fit_arma_one(
        u: np.ndarray, p: int, q: int, refine: int = 1, dtype=np.float64,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Stages 2-4 for one group, every intermediate in ``dtype`` (``u``
    must already have it). Returns (phi, theta, eps)."""
    dt = np.dtype(dtype).type
    n = len(u)
    if p + q == 0:
        return np.zeros(0, dtype=dtype), np.zeros(0, dtype=dtype), u.copy()
    if q > 0:
        M = min(max(p, q) + LONG_AR_EXTRA, max(1, n // 4))
        r = np.array([np.dot(u[k:], u[:n - k]) / dt(n)
                      for k in range(M + 1)], dtype=dtype)
        a = _levinson(r, M, dtype)
        eps = u.copy()
        for i in range(1, M + 1):
            eps[i:] -= a[i - 1] * u[:-i]
        # pre-sample lags treated as zero ⇒ first M values keep partial sums
    else:
        eps = u.copy()
    m = max(p, q)
    phi = np.zeros(p, dtype=dtype)
    theta = np.zeros(q, dtype=dtype)
    for _ in range(1 + refine):
        K = p + q
        Z = np.empty((n - m, K), dtype=dtype)
        for i in range(p):
            Z[:, i] = u[m - 1 - i:n - 1 - i]
        for j in range(q):
            Z[:, p + j] = eps[m - 1 - j:n - 1 - j]
        A = Z.T @ Z
        A[np.diag_indices_from(A)] += dt(RIDGE) * max(dt(1.0),
                                                      np.trace(A) / dt(K))
        b = Z.T @ u[m:]
        c = np.linalg.solve(A, b)
        phi, theta = c[:p], c[p:]
        sp = np.abs(phi).sum()
        if sp > dt(SHRINK):
            phi *= dt(SHRINK) / sp
        st = np.abs(theta).sum()
        if st > dt(SHRINK):
            theta *= dt(SHRINK) / st
        new_eps = np.zeros(n, dtype=dtype)
        for t in range(n):
            acc = u[t]
            for i in range(p):
                if t - 1 - i >= 0:
                    acc -= phi[i] * u[t - 1 - i]
            for j in range(q):
                if t - 1 - j >= 0:
                    acc -= theta[j] * new_eps[t - 1 - j]
            new_eps[t] = acc
        eps = new_eps
        if q == 0:
            break
    return phi, theta, eps


def _forecast_y(y: np.ndarray, S: int, H: int, d: int, wm: float,
                reg_future: np.ndarray, phi: np.ndarray, theta: np.ndarray,
                u: np.ndarray, eps: np.ndarray,
                dtype=np.float64) -> np.ndarray:
    """H-step forecast in y-units from the end of the train window."""
    dt = np.dtype(dtype).type
    p, q = len(phi), len(theta)
    u_h = list(u)
    e_h = list(eps)
    w_pred = np.empty(H, dtype=dtype)
    for h in range(H):
        acc = dt(0.0)
        for i in range(p):
            k = len(u_h) - 1 - i
            if k >= 0:
                acc += phi[i] * u_h[k]
        for j in range(q):
            k = len(e_h) - 1 - j
            if k >= 0:
                acc += theta[j] * e_h[k]
        w_pred[h] = wm + reg_future[h] + acc
        u_h.append(acc)
        e_h.append(dt(0.0))
    if d == 0:
        return w_pred
    if d == 1:
        return y[S - 1] + np.cumsum(w_pred)
    out = np.empty(H, dtype=dtype)
    y1, y2 = y[S - 1], y[S - 2]
    for h in range(H):
        nxt = w_pred[h] + dt(2.0) * y1 - y2
        out[h] = nxt
        y2, y1 = y1, nxt
    return out


def batched_fit_reference(
    y: np.ndarray,                  # [G, T]
    exog: np.ndarray,               # [T, KX] (shared across groups)
    orders: Sequence[Tuple[int, int, int]],
    train_len: int,
    designs: Optional[List[ExogDesign]] = None,
    dtype=np.float64,
) -> np.ndarray:
    """Validation MSE per (group, candidate): returns [G, C] in ``dtype``.
    The numerics oracle for the HIP kernel (same algorithm, f64). With
    ``dtype=np.float32`` it is the kernel's arithmetic emulated on the
    host: the designs are still computed in f64 and then rounded, as the
    GPU driver uploads them; everything else runs in f32."""
    y = np.asarray(y, dtype=dtype)
    G, T = y.shape
    S = train_len
    H = T - S
    if designs is None:
        designs = make_exog_designs(exog, S)
    by_d = {dz.d: _design_as(dz, dtype) for dz in designs}
    mse = np.full((G, len(orders)), np.inf, dtype=dtype)
    for ci, (p, d, q) in enumerate(orders):
        dz = by_d[d]
        n = S - d
        for g in range(G):
            yg = y[g]
            w = yg[:S].copy()
            for _ in range(d):
                w = np.diff(w)
            wm = w.mean()
            wc = w - wm
            beta = dz.P @ wc
            u = wc - dz.Xc_full[:n] @ beta
            phi, theta, eps = _fit_arma_one(u, p, q, dtype=dtype)
            reg_future = dz.Xc_full[n:n + H] @ beta
            fc = _forecast_y(yg, S, H, d, wm, reg_future, phi, theta, u, eps,
                             dtype)
            mse[g, ci] = np.mean((yg[S:] - fc) ** 2)
    return mse


def _design_as(dz: ExogDesign, dtype) -> ExogDesign:
    """The design rounded to ``dtype`` (the f64 one itself for f64)."""
    if np.dtype(dtype) == np.float64:
        return dz
    return ExogDesign(d=dz.d, Xc_full=dz.Xc_full.astype(dtype),
                      P=dz.P.astype(dtype), xmean=dz.xmean.astype(dtype))


def _designs_to_gpu(designs: List[ExogDesign], device):
    import torch
    xs, ps = [], []
    for dz in sorted(designs, key=lambda z: z.d):
        xs.append(torch.tensor(dz.Xc_full, dtype=torch.float32,
                               device=device).contiguous())
        ps.append(torch.tensor(dz.P, dtype=torch.float32,
                               device=device).contiguous())
    return xs, ps


def _to_yT(y, device):
    import torch
    y_t = torch.as_tensor(np.ascontiguousarray(y), dtype=torch.float32)
    if torch.device(device).type == "cuda":
        # upload [G,T] row-major, transpose to time-major ON DEVICE — the
        # host-side .t().contiguous() was ~2/3 of the whole-job wall time
        # at 100k groups (63 MB single-thread CPU transpose)
        return y_t.to(device).t().contiguous()
    return y_t.t().contiguous().to(device)


def _mfma_projection(yT, ps, train_len: int, device):
    """Stage-1 via the MFMA design-matrix GEMM for each d: Wc/wm from the
    diff+center kernel, beta = P_d @ Wc on the f32 matrix cores."""
    import torch
    from ..ops import _C
    T, G = yT.shape
    betas, wms = [], []
    for d in range(3):
        n = train_len - d
        wc = torch.empty((n, G), dtype=torch.float32, device=device)
        wm = torch.empty((G,), dtype=torch.float32, device=device)
        _C.diff_center(yT, wc, wm, train_len, d)
        beta = torch.empty((ps[d].shape[0], G), dtype=torch.float32,
                           device=device)
        _C.exog_project_mfma(ps[d], wc, beta)
        betas.append(beta)
        wms.append(wm)
    return betas, wms


def batched_eval_gpu(y, exog, orders, train_len: int, device="cuda",
                     yT=None, use_mfma: bool = True):
    """GPU candidate evaluation: returns (mse [G,C] torch.f32, status
    [G,C] torch.u8). ``y`` is [G,T] (numpy or torch)."""
    import torch
    from ..ops import require_ext, _C
    require_ext()
    if yT is None:
        yT = _to_yT(y, device)
    T, G = yT.shape
    designs = make_exog_designs(exog, train_len)
    xs, ps = _designs_to_gpu(designs, device)
    if use_mfma:
        betas, wms = _mfma_projection(yT, ps, train_len, device)
    else:
        empty = torch.empty(0, dtype=torch.float32, device=device)
        betas, wms = [empty] * 3, [empty] * 3
    orders_t = torch.tensor(list(orders), dtype=torch.int32,
                            device=device).reshape(-1, 3).contiguous()
    C = orders_t.shape[0]
    mse = torch.empty((C, G), dtype=torch.float32, device=device)
    status = torch.empty((C, G), dtype=torch.uint8, device=device)
    _C.groupfit_eval(yT, xs[0], xs[1], xs[2], ps[0], ps[1], ps[2],
                     orders_t, mse, status, train_len,
                     betas[0], betas[1], betas[2],
                     wms[0], wms[1], wms[2])
    return mse.t().contiguous(), status.t().contiguous()


def _check_future_exog(exog, future_exog, T: int) -> int:
    """Host-side shape checks shared by the forecast entry points; returns
    the horizon H."""
    ex, fx = np.shape(exog), np.shape(future_exog)
    if len(ex) != 2 or ex[0] != T:
        raise ValueError(f"exog must have T = {T} rows, got shape {ex}")
    if len(fx) != 2 or fx[1] != ex[1]:
        raise ValueError(f"future_exog must be [H, {ex[1]}] like exog, "
                         f"got shape {fx}")
    if fx[0] < 1:
        raise ValueError("future_exog needs at least one row (H >= 1)")
    return int(fx[0])


def _forecast_launch(yT, xs, best_order, params, H: int):
    """``groupfit_forecast`` on device tensors; ``xs`` are the stacked
    designs. Returns forecast/forecast_se [G,H], sigma2/status [G]."""
    import torch
    from ..ops import _C
    T, G = yT.shape
    dev = yT.device
    forecast = torch.empty((H, G), dtype=torch.float32, device=dev)
    forecast_se = torch.empty((H, G), dtype=torch.float32, device=dev)
    sigma2 = torch.empty((G,), dtype=torch.float32, device=dev)
    status = torch.empty((G,), dtype=torch.uint8, device=dev)
    _C.groupfit_forecast(yT, xs[0], xs[1], xs[2], best_order, params,
                         forecast, forecast_se, sigma2, status)
    return {"forecast": forecast.t().contiguous(),
            "forecast_se": forecast_se.t().contiguous(),
            "sigma2": sigma2, "status": status}


def batched_forecast_gpu(y, exog, future_exog, best_order, params,
                         device="cuda"):
    """Out-of-sample forecast from STORED coefficients: ``params``
    [G,1+KX+8] and ``best_order`` [G,3] as ``batched_fit_gpu`` returned
    them for the same ``y`` [G,T] and ``exog`` [T,KX]. No fitting: one
    streaming pass rebuilds the end-of-series state, then
    ``H = len(future_exog)`` steps. Returns a dict with ``forecast``
    [G,H], ``forecast_se`` [G,H], ``sigma2`` [G] and ``status`` [G] (1 iff
    every output of the group is finite)."""
    ys = np.shape(y)
    if len(ys) != 2:
        raise ValueError(f"y must be [G, T], got shape {ys}")
    G, T = ys
    H = _check_future_exog(exog, future_exog, T)
    KX = np.shape(exog)[1]
    if tuple(np.shape(params)) != (G, 1 + KX + 8):
        raise ValueError(f"params must be [{G}, {1 + KX + 8}], got shape "
                         f"{tuple(np.shape(params))}")
    if tuple(np.shape(best_order)) != (G, 3):
        raise ValueError(f"best_order must be [{G}, 3], got shape "
                         f"{tuple(np.shape(best_order))}")
    import torch
    from ..ops import require_ext
    require_ext()
    yT = _to_yT(y, device)
    xs, _ = _designs_to_gpu(stacked_exog_designs(exog, future_exog, T),
                            device)
    best_order = torch.as_tensor(best_order).to(
        device=device, dtype=torch.int32).contiguous()
    params = torch.as_tensor(params).to(
        device=device, dtype=torch.float32).contiguous()
    return _forecast_launch(yT, xs, best_order, params, H)


def batched_fit_gpu(y, exog, orders, train_len: int, device="cuda",
                    use_mfma: bool = True, future_exog=None):
    """Full W1 GPU pipeline: evaluate candidates, pick the best per group,
    final-fit on the whole series. Returns a dict with ``best_order``
    [G,3], ``mse`` [G,C], ``fitted`` [G,T], ``params`` [G,1+KX+8],
    ``status`` [G] (all torch tensors on ``device``). With ``future_exog``
    [H,KX] the final fit is followed by an H-step forecast from its
    coefficients: ``forecast`` [G,H], ``forecast_se`` [G,H], ``sigma2``
    [G] and ``forecast_status`` [G] are added, the other keys unchanged."""
    import torch
    from ..ops import require_ext, _C
    if future_exog is not None:
        H = _check_future_exog(exog, future_exog, np.shape(y)[1])
    require_ext()
    yT = _to_yT(y, device)
    T, G = yT.shape
    mse, status = batched_eval_gpu(y, exog, orders, train_len, device,
                                   yT=yT, use_mfma=use_mfma)
    orders_t = torch.tensor(list(orders), dtype=torch.int32, device=device
                            ).reshape(-1, 3)
    best_ci = mse.argmin(dim=1)                        # [G]
    best_order = orders_t[best_ci].contiguous()        # [G,3]
    if future_exog is None:
        designs = make_exog_designs(exog, T)           # full-series designs
    else:
        # same history rows and P, bit for bit, plus the H future rows
        designs = stacked_exog_designs(exog, future_exog, T)
    xs, ps = _designs_to_gpu(designs, device)
    KX = xs[0].shape[1]
    if use_mfma:
        # stage 1 for the final fit on the matrix cores too (full-series
        # design, train_len = T)
        betas, wms = _mfma_projection(yT, ps, T, device)
    else:
        empty = torch.empty(0, dtype=torch.float32, device=device)
        betas, wms = [empty] * 3, [empty] * 3
    fitted = torch.empty((T, G), dtype=torch.float32, device=device)
    params = torch.empty((G, 1 + KX + 8), dtype=torch.float32,
                         device=device)
    fstatus = torch.empty((G,), dtype=torch.uint8, device=device)
    _C.groupfit_final(yT, xs[0], xs[1], xs[2], ps[0], ps[1], ps[2],
                      best_order, fitted, params, fstatus,
                      betas[0], betas[1], betas[2],
                      wms[0], wms[1], wms[2])
    out = {
        "best_order": best_order, "mse": mse, "eval_status": status,
        "fitted": fitted.t().contiguous(), "params": params,
        "status": fstatus,
    }
    if future_exog is not None:
        fc = _forecast_launch(yT, xs, best_order, params, H)
        out["forecast_status"] = fc.pop("status")
        out.update(fc)
    return out


def fitted_values_reference(y: np.ndarray, exog: np.ndarray,
                            order: Tuple[int, int, int], train_len: int,
                            designs=None, dtype=np.float64) -> np.ndarray:
    """One-step-ahead fitted values over the full series for one group
    (used by the final-fit path; full-series design, S=T). ``dtype`` as
    in ``batched_fit_reference``."""
    p, d, q = order
    dt = np.dtype(dtype).type
    y = np.asarray(y, dtype=dtype)
    T = len(y)
    designs = designs or make_exog_designs(exog, T)
    dz = _design_as([z for z in designs if z.d == d][0], dtype)
    n = T - d
    w = y.copy()
    for _ in range(d):
        w = np.diff(w)
    wm = w.mean()
    wc = w - wm
    beta = dz.P @ wc
    u = wc - dz.Xc_full[:n] @ beta
    phi, theta, eps = _fit_arma_one(u, p, q, dtype=dtype)
    what = wm + dz.Xc_full[:n] @ beta
    for t in range(n):
        acc = dt(0.0)
        for i in range(p):
            if t - 1 - i >= 0:
                acc += phi[i] * u[t - 1 - i]
        for j in range(q):
            if t - 1 - j >= 0:
                acc += theta[j] * eps[t - 1 - j]
        what[t] += acc
    fit = np.empty(T, dtype=dtype)
    fit[:d] = y[:d]
    if d == 0:
        fit = what
    elif d == 1:
        fit[1:] = y[:-1] + what
    else:
        fit[2:] = dt(2.0) * y[1:-1] - y[:-2] + what
    return fit


# --------------------------------------------------------------------------
# out-of-sample forecast with standard errors
# --------------------------------------------------------------------------
def stacked_exog_designs(exog: np.ndarray, future_exog: np.ndarray,
                         train_len: int) -> List[ExogDesign]:
    """Designs over history + future rows: ``n = train_len - d`` history
    rows followed by the ``H`` future rows, differenced against the tail
    of the history and centered with the history means. The first ``n``
    rows and ``P`` are those of ``make_exog_designs(exog, train_len)``."""
    return make_exog_designs(
        np.vstack([np.asarray(exog, dtype=np.float64),
                   np.asarray(future_exog, dtype=np.float64)]), train_len)


def psi_weights_reference(phi: np.ndarray, theta: np.ndarray, d: int,
                          steps: int, dtype=np.float64) -> np.ndarray:
    """psi_0..psi_{steps-1} of the ARIMA(p,d,q) process: with
    ``1 - sum a_k B^k = (1 - sum phi_i B^i)(1 - B)^d``, psi_0 = 1 and
    ``psi_j = theta_j [j <= q] + sum_{k=1}^{min(j,p+d)} a_k psi_{j-k}``."""
    dt = np.dtype(dtype).type
    phi = np.asarray(phi, dtype=dtype)
    theta = np.asarray(theta, dtype=dtype)
    p, q = len(phi), len(theta)
    c = np.zeros(p + d + 1, dtype=dtype)      # 1 - sum a_k B^k
    c[0] = dt(1.0)
    c[1:p + 1] = -phi
    for _ in range(d):                        # times (1 - B)
        c[1:] = c[1:] - c[:-1]
    a = -c[1:]
    psi = np.zeros(steps, dtype=dtype)
    for j in range(steps):
        if j == 0:
            psi[0] = dt(1.0)
            continue
        acc = theta[j - 1] if j <= q else dt(0.0)
        for k in range(1, min(j, p + d) + 1):
            acc += a[k - 1] * psi[j - k]
        psi[j] = acc
    return psi


def forecast_from_params_reference(
        y: np.ndarray, design_d: ExogDesign, order: Tuple[int, int, int],
        wm, beta: np.ndarray, phi4: np.ndarray, theta4: np.ndarray, H: int,
        dtype=np.float64) -> Tuple[np.ndarray, np.ndarray, float]:
    """H-step forecast of one group with the coefficients GIVEN:
    ``(forecast [H], forecast_se [H], sigma2)``. ``design_d`` is the
    stacked design of the order's ``d`` (``T - d`` history rows, then H
    future rows); ``phi4``/``theta4`` are zero past p/q. The residual
    recursion is the fitted-value pass of ``groupfit_final``; the
    regression coefficients count as fixed in the standard error."""
    p, d, q = order
    dt = np.dtype(dtype).type
    y = np.asarray(y, dtype=dtype)
    T = len(y)
    n = T - d
    dz = _design_as(design_d, dtype)
    if dz.Xc_full.shape[0] != n + H:
        raise ValueError(f"design has {dz.Xc_full.shape[0]} rows, "
                         f"need {n} + {H}")
    wm = dt(wm)
    beta = np.asarray(beta, dtype=dtype)
    phi4 = np.asarray(phi4, dtype=dtype)
    theta4 = np.asarray(theta4, dtype=dtype)
    w = y.copy()
    for _ in range(d):
        w = np.diff(w)
    u = (w - wm) - dz.Xc_full[:n] @ beta
    e = np.zeros(n, dtype=dtype)
    m = max(p, q)
    sse = dt(0.0)
    for td in range(n):
        acc = dt(0.0)
        for i in range(min(4, td)):
            acc += phi4[i] * u[td - 1 - i] + theta4[i] * e[td - 1 - i]
        e[td] = u[td] - acc
        if td >= m:
            sse += e[td] * e[td]
    sigma2 = sse / dt(n - m)
    reg_future = dz.Xc_full[n:n + H] @ beta
    fc = _forecast_y(y, T, H, d, wm, reg_future, phi4[:p], theta4[:q], u, e,
                     dtype)
    psi = psi_weights_reference(phi4[:p], theta4[:q], d, H, dtype)
    se = np.sqrt(sigma2 * np.cumsum(psi * psi, dtype=dtype))
    return fc, se, sigma2


def batched_forecast_reference(
        y: np.ndarray, exog: np.ndarray, future_exog: np.ndarray,
        orders_per_group, dtype=np.float64,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Fit every group on its whole series (as ``fitted_values_reference``
    does) and forecast ``len(future_exog)`` steps past it. One order for
    all groups, or one per group. Returns ``forecast [G,H]``,
    ``forecast_se [G,H]`` and ``sigma2 [G]`` in ``dtype``."""
    y = np.asarray(y, dtype=dtype)
    G, T = y.shape
    H = len(future_exog)
    if np.ndim(orders_per_group) == 1:
        orders_per_group = [tuple(orders_per_group)] * G
    by_d = {dz.d: dz for dz in stacked_exog_designs(exog, future_exog, T)}
    fc = np.empty((G, H), dtype=dtype)
    se = np.empty((G, H), dtype=dtype)
    s2 = np.empty(G, dtype=dtype)
    for g in range(G):
        p, d, q = (int(v) for v in orders_per_group[g])
        dz = _design_as(by_d[d], dtype)
        n = T - d
        w = y[g].copy()
        for _ in range(d):
            w = np.diff(w)
        wm = w.mean()
        wc = w - wm
        beta = dz.P @ wc
        u = wc - dz.Xc_full[:n] @ beta
        phi, theta, _ = _fit_arma_one(u, p, q, dtype=dtype)
        phi4 = np.zeros(4, dtype=dtype)
        theta4 = np.zeros(4, dtype=dtype)
        phi4[:p] = phi
        theta4[:q] = theta
        fc[g], se[g], s2[g] = forecast_from_params_reference(
            y[g], by_d[d], (p, d, q), wm, beta, phi4, theta4, H, dtype)
    return fc, se, s2
