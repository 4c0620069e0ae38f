"""bench.py's --full / --dump-outputs plumbing on CPU: the options, the seeded
sample positions and the layout of the dumped arrays (torch CPU tensors stand
in for the device buffers; no kernel runs)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_is_the_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")


def test_dump_positions_are_fixed_and_in_range():
    import bench
    assert np.array_equal(bench.dump_positions(10, count=16), np.arange(10))
    p = bench.dump_positions(1 << 40, count=1000)
    assert p.dtype == np.int64 and p.shape == (1000,) and p.min() >= 0 and p.max() < (1 << 40)
    assert np.all(np.diff(p) >= 0)
    assert np.array_equal(p, bench.dump_positions(1 << 40, count=1000))
    # the default sample keeps a dump (two sampled outputs and their edges, float32) under 64 MB
    n_max = 64
    assert 4 * (2 * bench.DUMP_SAMPLES + 2 * bench.DUMP_EDGE * (n_max + 1)) <= 64 * 10**6


def test_dump_outputs_layout(tmp_path, monkeypatch):
    import torch

    import bench
    n, objects, L, Ls, size = 3, 4, 10, 16, 7
    rng = np.random.default_rng(1)
    reps = torch.from_numpy(rng.integers(0, 256, (n, objects * Ls), dtype=np.uint8))
    restored = torch.from_numpy(rng.integers(0, 256, objects * size + 5, dtype=np.uint8))  # (longer than the batch)
    logical = reps.view(n, objects, Ls)[:, :, :L].numpy()
    names = bench.dump_outputs(torch, str(tmp_path / "out"), reps, restored, n, objects, L, Ls, size)
    got = {nm: np.load(tmp_path / "out" / f"{nm}.npy") for nm in names}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["replicas"], logical.reshape(-1).astype(np.float32))  # the stride padding is left out
    assert np.array_equal(got["restored"], restored.numpy()[:objects * size].astype(np.float32))
    assert np.array_equal(got["replicas_edges"][:, :L], logical[:, 0, :])
    assert np.array_equal(got["replicas_edges"][:, L:], logical[:, objects - 1, :])
    # a sampled dump takes the same bytes of the same arrays
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 20)
    bench.dump_outputs(torch, str(tmp_path / "s"), reps, restored, n, objects, L, Ls, size, rank=1)
    p = bench.dump_positions(n * objects * L)
    assert np.array_equal(np.load(tmp_path / "s" / "replicas_rank1.npy"), logical.reshape(-1)[p].astype(np.float32))
    p = bench.dump_positions(objects * size)
    assert np.array_equal(np.load(tmp_path / "s" / "restored_rank1.npy"), restored.numpy()[p].astype(np.float32))
