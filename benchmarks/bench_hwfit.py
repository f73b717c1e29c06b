"""Batched Holt-Winters fit: 100k store-SKU groups x 157 weeks on one
MI355X. Metric: groups/sec for the whole fit (upload + grid/refinement
search + final pass with a 40-step forecast).

    python benchmarks/bench_hwfit.py

Two models are timed: trend + additive season m=52 (343 grid candidates)
and damped trend + multiplicative season m=4 (1,029 candidates). Each
runs in a child process of its own under its own time limit, and nothing
more is started after a child fails. The numpy oracle is timed on a
256-group sample for comparison. One JSON line is printed.
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

MODELS = {
    "trend_add52": dict(trend="add", seasonal="add", seasonal_periods=52),
    "damped_mul4": dict(trend="add", damped_trend=True, seasonal="mul",
                        seasonal_periods=4),
}
FORECAST_STEPS = 40


def worker(model: str, groups: int, weeks: int, repeats: int) -> dict:
    import torch
    from bench_groupfit import synth_groups
    from mi355x_scale.forecast.batched import _to_yT
    from mi355x_scale.forecast.batched_hw import (batched_hw_fit_gpu,
                                                  candidate_table)
    from mi355x_scale.ops import _C, require_ext
    require_ext()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hwfit needs a GPU")
    kw = MODELS[model]
    y, _ = synth_groups(groups, weeks)
    out = batched_hw_fit_gpu(y[:1024], forecast_steps=FORECAST_STEPS, **kw)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = batched_hw_fit_gpu(y, forecast_steps=FORECAST_STEPS, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    ok = float(out["status"].float().mean().item())

    # the search kernel alone, by device events
    yT = _to_yT(y, "cuda")
    table = torch.tensor(candidate_table(kw.get("trend"),
                                         kw.get("damped_trend", False),
                                         kw.get("seasonal")),
                         dtype=torch.float32, device="cuda")
    par = torch.empty((groups, 4), dtype=torch.float32, device="cuda")
    sse = torch.empty((groups,), dtype=torch.float32, device="cuda")
    st = torch.empty((groups,), dtype=torch.uint8, device="cuda")
    seas = {None: 0, "add": 1, "mul": 2}[kw.get("seasonal")]
    kms = []
    waves = 0
    for _ in range(repeats):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        waves = _C.hwfit_search(yT, table, par, sse, st,
                                kw.get("trend") is not None, seas,
                                kw["seasonal_periods"], 0)
        e1.record()
        torch.cuda.synchronize()
        kms.append(e0.elapsed_time(e1))
    dt = min(times)
    return {"model": model, "groups_per_s": groups / dt,
            "ms_per_fit": dt * 1e3, "ms_all": [t * 1e3 for t in times],
            "search_kernel_ms": min(kms), "search_waves": int(waves),
            "candidates": int(table.shape[0]) + 18, "ok_fraction": ok}


def oracle_rate(model: str, groups: int, weeks: int) -> float:
    from bench_groupfit import synth_groups
    from mi355x_scale.forecast.batched_hw import batched_hw_reference
    y, _ = synth_groups(groups, weeks)
    t0 = time.perf_counter()
    batched_hw_reference(y, forecast_steps=FORECAST_STEPS, **MODELS[model])
    return groups / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--weeks", type=int, default=157)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--oracle-groups", type=int, default=256)
    ap.add_argument("--step-timeout", type=float, default=240.0,
                    help="seconds allowed to each model's GPU run")
    ap.add_argument("--worker", choices=sorted(MODELS), default=None)
    args = ap.parse_args()

    if args.worker:
        print(json.dumps(worker(args.worker, args.groups, args.weeks,
                                args.repeats)))
        return 0

    results = {}
    for model in MODELS:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", model,
               "--groups", str(args.groups), "--weeks", str(args.weeks),
               "--repeats", str(args.repeats)]
        try:
            cp = subprocess.run(cmd, capture_output=True, text=True,
                                timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"error": f"{model}: no result within "
                                       f"{args.step_timeout:.0f} s"}))
            return 1
        if cp.returncode != 0:
            sys.stderr.write(cp.stderr[-2000:])
            print(json.dumps({"error": f"{model}: exit {cp.returncode}"}))
            return 1
        results[model] = json.loads(cp.stdout.strip().splitlines()[-1])

    oracle = {m: oracle_rate(m, args.oracle_groups, args.weeks)
              for m in MODELS}
    main_model = "trend_add52"
    print(json.dumps({
        "metric": "groups/sec",
        "value": results[main_model]["groups_per_s"],
        "unit": "groups/s",
        "n_gpus": 1,
        "steps": args.repeats,
        "warmup": 1,
        "ms_per_step": results[main_model]["ms_per_fit"],
        "higher_is_better": True,
        "dtype": "fp32",
        "data": "synthetic",
        "config": {
            "model": "Holt-Winters grid + 2x9 refinement search + final "
                     f"pass, {FORECAST_STEPS}-step forecast",
            "groups": args.groups, "weeks": args.weeks,
            "models": results,
            "oracle_groups": args.oracle_groups,
            "oracle_groups_per_s": oracle,
        },
    }))
    return 0


if __name__ == "__main__":
    sys.exit(main())
