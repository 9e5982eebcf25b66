"""CPU tier: bench.py --dump-outputs writes the timed frame as float64 .npy, a frame over the size cap as a fixed, seeded row sample."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("rl_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_the_whole_frame(tmp_path):
    frame = torch.rand(108, 192, 3, dtype=torch.float64)
    _bench().dump_outputs(str(tmp_path / "out"), frame)
    assert sorted(os.listdir(tmp_path / "out")) == ["frame.npy"]
    got = np.load(tmp_path / "out" / "frame.npy")
    assert got.dtype == np.float64 and np.array_equal(got, frame.numpy())


def test_dump_of_a_large_frame_is_a_seeded_row_sample_under_64_mb(tmp_path):
    bench = _bench()
    frame = torch.rand(2160, 3840, 3, dtype=torch.float64)
    runs = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        bench.dump_outputs(str(d), frame)
        assert sum(os.path.getsize(d / n) for n in os.listdir(d)) <= 64_000_000
        rows, got = np.load(d / "frame_rows.npy"), np.load(d / "frame.npy")
        assert rows.dtype == np.float64 and np.array_equal(got, frame.numpy()[rows.astype(np.int64)])
        runs.append(rows)
    assert np.array_equal(runs[0], runs[1])
