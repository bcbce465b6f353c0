"""bench.py driver-contract tests: single-process CPU run and the torchrun
multi-rank launch (gloo on CPU — the same code path RCCL takes on GPUs)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_env():
    """Environment that hides every GPU from the child processes: these
    launches test the CPU/gloo path, also on a machine that has GPUs (and
    fewer of them than ranks). torch on ROCm honours HIP_VISIBLE_DEVICES,
    CUDA_VISIBLE_DEVICES alone does not hide the devices there; an invalid
    ordinal ends the visible-device list."""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="-1",
               HIP_VISIBLE_DEVICES="-1")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    return env


BENCH_ARGS = ["--steps", "2", "--warmup", "1", "--batch", "2",
              "--trajectory", "4", "--lstm", "16", "--pool", "2"]


def _check_line(line: str, n_gpus: int):
    out = json.loads(line)
    assert out["metric"].startswith("learner env-frames/sec")
    assert out["n_gpus"] == n_gpus
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True
    assert out["scaling"] == "weak"
    assert out["data"] == "synthetic"
    assert out["config"]["global_batch"] == 2 * n_gpus
    assert out["config"]["parallelism"] == f"dp{n_gpus}"
    return out


def test_bench_single_process():
    r = subprocess.run([sys.executable, "bench.py"] + BENCH_ARGS,
                       capture_output=True, text=True, cwd=REPO,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_line(r.stdout.strip().splitlines()[-1], 1)


def _dump_twice(tmp_path, env=None):
    """Two bench runs with the same arguments (the second with --full),
    each dumping its outputs; returns the two {file: array} dicts."""
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        r = subprocess.run(
            [sys.executable, "bench.py"] + BENCH_ARGS + extra
            + ["--dump-outputs", str(d)],
            capture_output=True, text=True, cwd=REPO, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        _check_line(r.stdout.strip().splitlines()[-1], 1)
        files = sorted(p.name for p in d.iterdir())
        assert files == ["baseline_loss.npy", "entropy.npy", "grads.npy",
                         "params.npy", "pi_loss.npy"]
        arrs = {f: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 for a in arrs.values())
        assert all(np.isfinite(a).all() for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
        assert arrs["params.npy"].size > 1000
        assert np.abs(arrs["grads.npy"]).max() > 0
        dumps.append(arrs)
    return dumps


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float32 .npy
    (<= 64 MB in all), bit-identical on the CPU path for two runs with the
    same arguments; --full is accepted and leaves the result line alone."""
    a, b = _dump_twice(tmp_path, _cpu_env())
    for f in a:
        np.testing.assert_array_equal(a[f], b[f])


@pytest.mark.gpu
def test_bench_dump_outputs_reproducible_gpu(tmp_path):
    """Same on the graphed GPU path. The dumped step runs from the
    restored, bit-identical initial weights on a fixed batch, so neither the
    machine-dependent number of clock-priming updates nor noise amplified by
    earlier updates may show; what is left is one step's atomic
    accumulation-order noise: a gradient element may flip by one bf16 ulp
    (2^-8 relative, bounded here against the array's largest magnitude),
    and one RMSProp update moves a parameter by at most
    lr/sqrt(1-rho) = 6e-4/0.1, of which a 1-ulp gradient flip perturbs
    2^-7 relative. The losses come from bf16 logits/values, so they are
    held to one bf16 ulp."""
    a, b = _dump_twice(tmp_path)
    g_tol = 2.0 ** -8 * np.abs(a["grads.npy"]).max()
    p_tol = (6e-4 / 0.1) * 2.0 ** -7
    np.testing.assert_allclose(a["grads.npy"], b["grads.npy"],
                               rtol=0, atol=g_tol)
    np.testing.assert_allclose(a["params.npy"], b["params.npy"],
                               rtol=0, atol=p_tol)
    for f in ("pi_loss.npy", "baseline_loss.npy", "entropy.npy"):
        np.testing.assert_allclose(a[f], b[f], rtol=2.0 ** -8)


@pytest.mark.parametrize("algo,extra", [
    ("apex", ["--batch", "4"]),
    ("r2d2", ["--batch", "2", "--seq-len", "6", "--burn-in", "2"]),
])
def test_bench_algo_flags(algo, extra):
    """--algo apex/r2d2 (BASELINE configs #3/#4) emit well-formed contract
    lines; CPU fallback exercises the same sample->train->priority-update
    loop against the float64 Memory."""
    r = subprocess.run(
        [sys.executable, "bench.py", "--algo", algo, "--steps", "2",
         "--warmup", "1"] + extra,
        capture_output=True, text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert algo in out["metric"].lower().replace("-", "")
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["data"] == "synthetic"
    if algo == "r2d2":
        assert out["config"]["seq_len"] == 6
        assert out["config"]["burn_in"] == 2


def test_bench_torchrun_two_ranks():
    """Exactly the driver's multi-GPU launch shape, on CPU/gloo."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29511", "bench.py"] + BENCH_ARGS,
        capture_output=True, text=True, cwd=REPO, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    json_lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1, "exactly one JSON line from rank 0"
    out = _check_line(json_lines[-1], 2)
    # whole-job aggregate: 2 ranks x 2 batch x 4 steps... value is frames/s;
    # just confirm the frames accounting doubled via global_batch above
    assert out["config"]["frames_per_step_per_rank"] == 8


def test_bench_torchrun_four_ranks():
    """The driver's N=4 launch shape (gloo on CPU): rank logic, pool
    seeding, MAX-over-ranks timing and the single rank-0 JSON line must
    hold beyond 2 ranks."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
         "--master-port", "29513", "bench.py"] + BENCH_ARGS,
        capture_output=True, text=True, cwd=REPO, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    json_lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1
    out = _check_line(json_lines[-1], 4)
    assert out["config"]["global_batch"] == 8
