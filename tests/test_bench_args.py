"""bench.py's arguments (no GPU): a plain run keeps only the timed steps -- the legs that
take runs of their own are off unless --full asks for them, where --no-cpu, --no-rho and
--no-bruteforce still drop single legs."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_extra_legs(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_cpu and a.no_rho and a.no_bruteforce


def test_full_run_keeps_every_leg_unless_dropped(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    assert not (a.no_cpu or a.no_rho or a.no_bruteforce)
    a = _parse(bench, monkeypatch, "--full", "--no-cpu")
    assert a.no_cpu and not a.no_rho


def test_dump_outputs_writes_float_arrays(bench, tmp_path):
    import numpy as np

    bench.dump_outputs(str(tmp_path / "d"), {"u": np.ones((3, 1), np.float32), "n": np.arange(3)})
    assert np.load(tmp_path / "d" / "u.npy").dtype == np.float32
    assert np.load(tmp_path / "d" / "n.npy").dtype == np.float64
