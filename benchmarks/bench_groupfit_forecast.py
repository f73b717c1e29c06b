"""Batched ARIMAX fit with an out-of-sample forecast: 100k store-SKU groups
x 157 weeks on one MI355X. Metric: groups/sec for the whole job
(``batched_fit_gpu``: upload + candidate grid + final fit) with a 40-step
forecast and standard errors, against the same job without it.

    python benchmarks/bench_groupfit_forecast.py

The two variants are timed in alternating runs. ``groupfit_forecast`` and
``groupfit_final`` are also timed alone by device events, on the same
panel, orders and coefficients. The GPU work runs in a child process under
its own time limit, and nothing more is started after it fails. One JSON
line is printed.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FORECAST_STEPS = 40


def future_exog(weeks: int, steps: int) -> np.ndarray:
    """The exogenous indicators of the ``steps`` weeks after the panel."""
    import pandas as pd
    from mi355x_scale.data.generator import _week_dates
    from mi355x_scale.forecast.pipeline import (EXO_COLS, _future_dates,
                                                add_exo_variables)
    dates = _future_dates(_week_dates(weeks).to_numpy(), steps)
    return add_exo_variables(
        pd.DataFrame({"Date": dates}))[EXO_COLS].to_numpy()


def worker(groups: int, weeks: int, train_len: int, repeats: int) -> dict:
    import torch
    from bench_groupfit import synth_groups
    from mi355x_scale.forecast.batched import (_designs_to_gpu,
                                               _mfma_projection, _to_yT,
                                               batched_fit_gpu,
                                               stacked_exog_designs)
    from mi355x_scale.forecast.pipeline import DEFAULT_GPU_ORDERS
    from mi355x_scale.ops import _C, require_ext
    require_ext()
    if not torch.cuda.is_available():
        raise SystemExit("bench_groupfit_forecast needs a GPU")
    orders = DEFAULT_GPU_ORDERS
    y, exog = synth_groups(groups, weeks)
    fx = future_exog(weeks, FORECAST_STEPS)
    batched_fit_gpu(y[:1024], exog, orders, train_len, future_exog=fx)
    torch.cuda.synchronize()
    times = {"fit": [], "fit_forecast": []}
    for _ in range(repeats):            # alternating runs
        for name, kw in (("fit", {}), ("fit_forecast", {"future_exog": fx})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = batched_fit_gpu(y, exog, orders, train_len, **kw)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    ok = float(out["forecast_status"].float().mean().item())

    # the two kernels alone, by device events, on the job's own buffers
    yT = _to_yT(y, "cuda")
    xs, ps = _designs_to_gpu(stacked_exog_designs(exog, fx, weeks), "cuda")
    betas, wms = _mfma_projection(yT, ps, weeks, "cuda")
    best, params = out["best_order"], out["params"]
    fitted = torch.empty((weeks, groups), dtype=torch.float32, device="cuda")
    fstatus = torch.empty((groups,), dtype=torch.uint8, device="cuda")
    par2 = torch.empty_like(params)
    fc = torch.empty((FORECAST_STEPS, groups), dtype=torch.float32,
                     device="cuda")
    se = torch.empty_like(fc)
    s2 = torch.empty((groups,), dtype=torch.float32, device="cuda")
    st = torch.empty((groups,), dtype=torch.uint8, device="cuda")

    def run_final():
        _C.groupfit_final(yT, xs[0], xs[1], xs[2], ps[0], ps[1], ps[2],
                          best, fitted, par2, fstatus,
                          betas[0], betas[1], betas[2],
                          wms[0], wms[1], wms[2])

    def run_forecast():
        _C.groupfit_forecast(yT, xs[0], xs[1], xs[2], best, params,
                             fc, se, s2, st)

    kernel_ms = {}
    for name, fn in (("groupfit_final", run_final),
                     ("groupfit_forecast", run_forecast)):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        kernel_ms[name] = min(ms)
    counts = torch.bincount(
        (best[:, 0] * 100 + best[:, 1] * 10 + best[:, 2]).long())
    mix = {f"{k // 100},{k // 10 % 10},{k % 10}": int(c)
           for k, c in enumerate(counts.tolist()) if c}
    return {"fit_ms": [t * 1e3 for t in times["fit"]],
            "fit_forecast_ms": [t * 1e3 for t in times["fit_forecast"]],
            "kernel_ms": kernel_ms, "order_mix": mix, "ok_fraction": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--weeks", type=int, default=157)
    ap.add_argument("--train-len", type=int, default=117)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=240.0,
                    help="seconds allowed to the GPU run")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()

    if args.worker:
        print(json.dumps(worker(args.groups, args.weeks, args.train_len,
                                args.repeats)))
        return 0

    cmd = [sys.executable, os.path.abspath(__file__), "--worker",
           "--groups", str(args.groups), "--weeks", str(args.weeks),
           "--train-len", str(args.train_len),
           "--repeats", str(args.repeats)]
    try:
        cp = subprocess.run(cmd, capture_output=True, text=True,
                            timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "no result within "
                                   f"{args.step_timeout:.0f} s"}))
        return 1
    if cp.returncode != 0:
        sys.stderr.write(cp.stderr[-2000:])
        print(json.dumps({"error": f"worker: exit {cp.returncode}"}))
        return 1
    res = json.loads(cp.stdout.strip().splitlines()[-1])
    dt = min(res["fit_forecast_ms"]) / 1e3
    print(json.dumps({
        "metric": "groups/sec",
        "value": args.groups / dt,
        "unit": "groups/s",
        "n_gpus": 1,
        "steps": args.repeats,
        "warmup": 1,
        "ms_per_step": dt * 1e3,
        "higher_is_better": True,
        "dtype": "fp32",
        "data": "synthetic",
        "config": {
            "model": "ARIMAX grid 10 candidates + final fit + "
                     f"{FORECAST_STEPS}-step forecast with standard errors",
            "groups": args.groups, "weeks": args.weeks,
            "train_len": args.train_len,
            "without_forecast_groups_per_s":
                args.groups / (min(res["fit_ms"]) / 1e3),
            **res,
        },
    }))
    return 0


if __name__ == "__main__":
    sys.exit(main())
