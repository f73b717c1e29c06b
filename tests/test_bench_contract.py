"""bench.py driver-contract rehearsal (the round-end SCALE run shape).

The driver launches `python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...` and
parses ONE JSON line from rank 0. Rehearse that exact shape at N=2 on
CPU (gloo; bench.py's CPU smoke config) so contract regressions surface
here instead of in the driver's multi-GPU window.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(extra, env_extra=None, timeout=420):
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    # these are CPU rehearsals (they assert the CPU smoke config): hide any
    # GPU from the child so they mean the same on a GPU box
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    if env_extra:
        env.update(env_extra)
    res = subprocess.run(extra, capture_output=True, text=True,
                         timeout=timeout, cwd=REPO, env=env)
    lines = [ln for ln in res.stdout.splitlines()
             if ln.startswith("{") and '"metric"' in ln]
    assert lines, (f"no JSON line. rc={res.returncode}\n"
                   f"stdout:\n{res.stdout[-1500:]}\n"
                   f"stderr:\n{res.stderr[-1500:]}")
    return json.loads(lines[-1])


def _check_contract(out, n_gpus):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in out, f"missing {key}"
    assert out["n_gpus"] == n_gpus
    assert out["metric"] == "samples/sec"
    assert out["value"] > 0
    assert out["data"] == "synthetic"
    assert out["scaling"] == "weak"
    assert out["config"]["model"] == "resnet18"
    assert out["config"]["global_batch"] == 8 * n_gpus  # CPU smoke batch


def test_bench_single_process_contract():
    out = _run_bench([sys.executable, "bench.py", "--steps", "2",
                      "--warmup", "1"])
    _check_contract(out, 1)


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's loss and the updated
    weights as float32 .npy, and two runs with the same arguments see the
    same inputs, so (on CPU, same thread count) the dumps are bit-identical.
    The second run adds --full, which must be accepted and, in the CPU
    config, changes no input."""
    import numpy as np
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = _run_bench([sys.executable, "bench.py", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(d)] + extra)
        _check_contract(out, 1)
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        files = sorted(p.name for p in d.iterdir())
        assert files == ["loss.npy", "params.npy"]
        dumps.append({p.stem: np.load(p) for p in d.iterdir()})
    a, b = dumps
    total = 0
    for k in a:
        assert a[k].dtype == np.float32
        assert np.isfinite(a[k]).all()
        assert np.array_equal(a[k], b[k]), k
        total += a[k].nbytes
    assert total <= 64 * 1024 * 1024
    assert a["loss"].shape == (1,)
    # resnet18: 11,689,512 trainable weights, dumped whole
    assert a["params"].shape == (11_689_512,)


@pytest.mark.timeout(600)
def test_bench_torchrun_ws2_contract():
    """The driver's exact launch shape at N=2 (gloo on CPU)."""
    out = _run_bench([
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
        "--master-port", "29377", "bench.py", "--gpus", "2",
        "--steps", "2", "--warmup", "1",
    ], env_extra={"MI355X_BACKEND": "gloo"})
    _check_contract(out, 2)
