"""GPU: bench.py's own rank launcher, and its plain / --full / --dump-outputs runs.  `python bench.py --gpus 2` (no WORLD_SIZE
in the environment) must start two ranks itself and print ONE JSON line with n_gpus == 2; with APTAI_BENCH_BACKEND=gloo both
ranks share the one card of the test box (the RCCL branch needs two cards and is what the driver's 8-GPU run exercises).  Also
rehearsed: a hipGraph capture that fails on ONE rank only must switch EVERY rank to the eager loop (different collective
sequences would hang)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env, *flags, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(APTAI_BENCH_BACKEND="gloo", **extra_env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--batch", "2", "--seconds", "1", "--no-cpu-baseline", *flags], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), p.stderr


def test_bench_launches_its_own_ranks():
    res, err = _run({})
    assert res["n_gpus"] == 2 and res["config"]["ranks"] == 2 and res["config"]["global_batch"] == 4
    assert res["config"]["execution"].startswith("hipGraph")
    assert res["value"] > 0 and res["scaling"] == "weak"
    assert "gloo" in res["config"]["collective"]


def test_capture_failure_on_one_rank_moves_every_rank_to_eager():
    res, err = _run({"APTAI_GRAPH_FAIL_CAPTURE": "rank1"})
    assert res["n_gpus"] == 2 and res["config"]["execution"] == "eager autograd loop"
    assert "ALL ranks run the eager loop" in err


def _run_one(out_dir, *flags, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "2", "--seconds", "1", "--dump-outputs", str(out_dir), *flags], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_what_full_computes(tmp_path):
    """A plain run prints the headline fields only; --full adds the roofline and leaves the timed steps' results unchanged:
    the arrays --dump-outputs writes are equal between the two runs (seeded inputs and weights, deterministic kernels)."""
    import numpy as np
    plain = _run_one(tmp_path / "plain")
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["higher_is_better"] is True
    assert plain["dtype"] == "bf16" and plain["unit"] == "utterances/sec"
    assert not {"roofline", "cpu_baseline", "ema_rmse_vs_ref", "index_exact"} & set(plain)
    full = _run_one(tmp_path / "full", "--full", "--no-cpu-baseline")
    assert full["roofline"]["launches"] > 0 and full["roofline"]["achieved"] > 0
    names = sorted(os.listdir(tmp_path / "plain"))
    assert {"loss.npy", "tvs_pred.npy", "phn_fc_pred.npy", "params.npy", "grads.npy"} <= set(names)
    assert names == sorted(os.listdir(tmp_path / "full"))
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "plain" / "loss.npy")) == pytest.approx(plain["loss"], abs=1e-5)
