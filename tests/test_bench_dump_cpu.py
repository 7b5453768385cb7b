"""bench.py --dump-outputs: the files it writes from the last timed step's outputs (names, dtype, the 64 MB budget and its seeded sample).
The outputs themselves come from the GPU path; here the writer gets host tensors of the same kinds."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_are_written_whole(tmp_path):
    g = torch.Generator().manual_seed(0)
    outputs = {"loss": torch.tensor([2.5]), "grad.a.b": torch.randn(3, 5, generator=g), "param.a.b": torch.randn(3, 5, generator=g)}
    bench.dump_outputs(str(tmp_path), outputs)
    assert sorted(os.listdir(tmp_path)) == ["grad.a.b.npy", "loss.npy", "param.a.b.npy"]
    for k, t in outputs.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy())


def test_large_outputs_keep_a_fixed_sample_inside_the_budget(tmp_path):
    g = torch.Generator().manual_seed(1)
    outputs = {"loss": torch.tensor([1.0]), "grad.w": torch.randn(12_000_000, generator=g), "param.w": torch.randn(6_000_000, generator=g)}
    bench.dump_outputs(str(tmp_path / "a"), outputs)
    bench.dump_outputs(str(tmp_path / "b"), outputs)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    for k, t in outputs.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)  # the same positions on every run
        assert np.isin(a, t.numpy()).all()  # elements of the output, not something derived from it
    assert np.load(tmp_path / "a" / "grad.w.npy").size > np.load(tmp_path / "a" / "param.w.npy").size > 1_000_000
