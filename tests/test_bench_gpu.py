"""A plain bench.py run end to end on the GPU, at a small shape: the result
line's keys, --steps, that the legs beside the metric stay off without --full,
and --dump-outputs checked byte for byte against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ctypes as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_what_the_oracle_computes(gpu, tmp_path):
    # --no-jit: the repair runs the ahead-of-time kernel, so the run compiles
    # nothing (tests/test_jit_gpu.py covers the run-time compiled kernels)
    k, m, objects, size = 16, 4, 3, 1 << 20
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--objects", str(objects), "--object-mib", "1", "--no-jit", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert (res["steps"], res["warmup"], res["full"], res["unit"], res["dtype"]) == (3, 1, False, "GiB/s", "u16")
    assert res["higher_is_better"] is True and res["value"] > 0 and res["ms_per_step"] > 0
    # value = object bytes of a step over ms_per_step (both rounded to 3 decimals in the line)
    rounding = 0.0005 / res["ms_per_step"] + 0.0005 / res["value"]
    assert res["value"] == pytest.approx(objects * size / 2**30 / (res["ms_per_step"] * 1e-3), rel=1e-6 + 1.01 * rounding)
    for leg in ("restore_aot", "regenerate_ms", "sha256_replicas_GiBps", "align16", "c4", "live_shape", "cpu_baseline"):
        assert res[leg] is None, leg
    n = k + m
    L = O.replica_size(2, k, size)
    data = [O.splitmix(0x7664730000000000 + o, size) for o in range(objects)]
    want = np.stack([np.stack([O.encode(k, rep, d) for d in data]) for rep in range(n)])  # [n][objects][L]
    got = {nm: np.load(out / f"{nm}.npy") for nm in res["dumped_outputs"]}
    assert all(g.dtype == np.float32 for g in got.values())
    assert sum(g.nbytes for g in got.values()) <= 64 * 10**6
    assert np.array_equal(got["replicas"], want.reshape(-1).astype(np.float32))
    assert np.array_equal(got["restored"], np.concatenate(data).astype(np.float32))
    e = got["replicas_edges"].shape[1] // 2
    assert np.array_equal(got["replicas_edges"], np.concatenate([want[:, 0, :e], want[:, -1, L - e:]], axis=1))
    e = got["restored_edges"].size // 2
    assert np.array_equal(got["restored_edges"], np.concatenate([data[0][:e], data[-1][size - e:]]))
