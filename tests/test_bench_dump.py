"""bench.py --dump-outputs, host side: the arrays of one step are written as float32 .npy files; above
the size budget every array keeps the same seeded sample of env rows, identical from run to run.
A plain run (no --full) switches off everything but the main line."""
import os
import sys

import numpy as np
import torch

import bench


def _outputs(E):
    g = torch.Generator().manual_seed(3)
    obs = torch.rand((E, 1, 57), generator=g)
    return {"obs": obs, "reward": torch.rand(E, generator=g), "terminated": torch.rand(E, generator=g) < 0.1,
            "truncated": torch.rand(E, generator=g) < 0.2, "terminal_observation": obs * 2}


def test_dump_writes_float32_arrays(tmp_path):
    out = _outputs(33)
    bench.dump_outputs(str(tmp_path / "d"), out, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f"{k}.npy" for k in out)
    for k, v in out.items():
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        np.testing.assert_array_equal(a, v.float().numpy())


def test_dump_samples_rows_above_the_budget(tmp_path, monkeypatch):
    E = 1000
    out = _outputs(E)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100_000)
    bench.dump_outputs(str(tmp_path / "a"), out, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), out, 0, 1)
    rows = np.load(tmp_path / "a" / "envs.npy")
    assert 0 < len(rows) < E and np.all(np.diff(rows) > 0)
    total = 0
    for k, v in out.items():
        a = np.load(tmp_path / "a" / f"{k}.npy")
        total += a.nbytes
        np.testing.assert_array_equal(a, v.float().numpy()[rows.astype(np.int64)])
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / f"{k}.npy"))
    assert total + rows.nbytes <= 100_000


def test_plain_run_times_the_main_line_only(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert not a.full and a.no_configs and a.no_cpu_baseline and a.no_sweep and a.no_allgather and a.graph_only
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    a = bench.parse()
    assert a.full and not (a.no_configs or a.no_cpu_baseline or a.no_sweep or a.no_allgather or a.graph_only)
