"""bench.py --dump-outputs: the writer of the last timed step's outputs (no GPU: CPU tensors stand in for the step's)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_writes_every_tensor_as_float32_or_float64(tmp_path):
    import bench
    out = {"depth": torch.arange(12, dtype=torch.float32).view(1, 3, 4), "norm_curv": torch.ones(1, 1, 3, 4, dtype=torch.float16),
           "stage1": {"depth": torch.zeros(2, 2)}, "loss": torch.tensor([0.25], dtype=torch.float64), "note": "not an array"}
    shapes = bench.dump_outputs(out, str(tmp_path))
    assert set(shapes) == {"depth", "norm_curv", "stage1.depth", "loss"}
    assert sorted(os.listdir(tmp_path)) == ["depth.npy", "loss.npy", "norm_curv.npy", "stage1.depth.npy"]
    d = np.load(tmp_path / "depth.npy")
    assert d.dtype == np.float32 and d.shape == (1, 3, 4) and np.array_equal(d.reshape(-1), np.arange(12, dtype=np.float32))
    assert np.load(tmp_path / "norm_curv.npy").dtype == np.float32
    assert np.load(tmp_path / "loss.npy").dtype == np.float64


def test_dump_over_budget_keeps_a_fixed_seeded_sample(tmp_path):
    import bench
    big = torch.arange(100_000, dtype=torch.float32)
    out = {"big": big, "small": torch.ones(10)}
    budget = 40_000
    bench.dump_outputs(out, str(tmp_path / "a"), budget=budget)
    bench.dump_outputs(out, str(tmp_path / "b"), budget=budget)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b)                                   # same positions on every run
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, big.numpy()))   # a sample of the elements, ascending
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))   # minus the .npy headers
    assert total <= budget
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), np.ones(10, dtype=np.float32))
