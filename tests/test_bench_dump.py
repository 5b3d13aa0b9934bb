"""bench.py --dump-outputs on the host side: the arrays are written whole while they fit the budget, beyond it the largest are
cut to the same seeded sample of entries on every run, and the files never exceed 64 MB in all."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _on_disk(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_outputs_within_the_budget_are_written_whole(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(1)
    arrays = {"loss": np.float32(2.5).reshape(()), "total_energy": rng.random((256, 1)).astype(np.float32),
              "parameters": rng.random(1000).astype(np.float32), "probe": rng.random(7)}
    shapes = bench.write_outputs(arrays, str(tmp_path))
    assert shapes == {k: list(v.shape) for k, v in arrays.items()}
    for k, v in arrays.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == v.dtype and np.array_equal(got, v), k


def test_outputs_beyond_the_budget_are_a_fixed_sample_under_64_mb(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(2)
    arrays = {"loss": np.float32(1.0).reshape(()), "parameters": rng.random(9_000_000).astype(np.float32),
              "gradients": rng.random(8_000_000).astype(np.float32), "ema_parameters": rng.random(3_000_000).astype(np.float32)}
    a, b = tmp_path / "a", tmp_path / "b"
    shapes = bench.write_outputs(arrays, str(a))
    assert bench.write_outputs(arrays, str(b)) == shapes
    assert _on_disk(a) <= 64_000_000
    assert shapes["loss"] == [] and shapes["ema_parameters"] == [3_000_000]      # the small ones stay whole
    for k in arrays:
        x, y = np.load(a / f"{k}.npy"), np.load(b / f"{k}.npy")
        assert np.array_equal(x, y), k
        assert np.isin(x, arrays[k]).all(), k                                   # entries of the array, not new values
