"""bench.py on the device, at a small size: a plain run times its steps and prints the
headline line without the legs that take runs of their own, --full adds them, and
--dump-outputs writes what the last timed solve returned -- the same arrays from run to
run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BENCH = os.path.join(REPO, "bench.py")
WALKS = 2000
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--walks", str(WALKS)]
HEADLINE = {"metric": "walk-steps/sec", "unit": "walk-steps/s", "higher_is_better": True, "dtype": "f32"}


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, BENCH, *SMALL, *extra], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs_reproducibly(gpu_available, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench("--dump-outputs", str(a))
    _bench("--dump-outputs", str(b))
    for k, v in HEADLINE.items():
        assert d[k] == v
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = walk-steps / s of the timed region, ms_per_step = that region / steps
    assert d["value"] == pytest.approx(2 * d["config"]["walk_steps_per_solve"] / (2e-3 * d["ms_per_step"]), rel=1e-3)
    # the legs that take runs of their own are not in a plain line
    assert d["cpu_baseline"] is None and "rho_a" not in d and "first_solve_ms" not in d["cold"]
    assert sorted(os.listdir(a)) == ["point_sums.npy", "u.npy"]
    u, sums = np.load(a / "u.npy"), np.load(a / "point_sums.npy")
    assert u.dtype == np.float32 and u.shape == (48, 1)
    assert sums.dtype == np.float64 and sums.shape == (48, 3)
    assert np.array_equal(u[:, 0], (sums[:, 0] / WALKS).astype(np.float32))
    assert sums[:, 2].sum() > 0
    assert d["u_checksum"] == pytest.approx(float(np.sum(sums[:, 0] / WALKS)), rel=1e-12)
    assert np.array_equal(u, np.load(b / "u.npy")) and np.array_equal(sums, np.load(b / "point_sums.npy"))


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(gpu_available):
    d = _bench("--full", "--cpu-seconds", "0.2")
    for k, v in HEADLINE.items():
        assert d[k] == v
    assert d["cpu_baseline"]["value"] > 0
    assert d["cold"]["first_solve_ms"] > 0
    assert d["rho_a"]["vs_reference_replay"]["steps_identical"] is True
