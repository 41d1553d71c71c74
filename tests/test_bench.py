"""bench.py's own contract: `--dump-outputs DIR` (what the timed path computed, a fixed seeded
sample of a large output, 64 MB at most) and a plain run that times the headline alone."""

import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump(tmp_path, arrays):
    import torch
    import bench
    bench.dump_outputs(SimpleNamespace(dump_outputs=str(tmp_path)), SimpleNamespace(rank=0, torch=torch),
                       arrays)
    return {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones(tmp_path):
    """On the host: an array up to 8 MiB is written whole; a larger one as 32 MiB of whole rows
    plus 2^20 single elements, at positions fixed by the seed (two runs, two identical sets of
    files), 64 MB at most in all; complex outputs as real pairs."""
    import torch
    nrow, ncol = 300, 1 << 14
    big = torch.arange(nrow * ncol, dtype=torch.float64).reshape(nrow, ncol)
    small = torch.randn(4, 5, dtype=torch.complex128)
    got = _dump(tmp_path / "a", {"big": big, "small": small, "count": [17]})
    assert sorted(got) == ["big_points", "big_rows", "count", "small"]
    assert got["count"].dtype == np.float64 and got["count"].tolist() == [17.0]
    assert np.array_equal(got["small"], torch.view_as_real(small).numpy())
    rows = got["big_rows"]
    assert rows.dtype == np.float64 and rows.shape == (256, ncol)        # 32 MiB of whole rows
    idx = (rows[:, 0] // ncol).astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(rows, big.numpy()[idx])
    pts = got["big_points"]
    assert pts.shape == (1 << 20,) and np.all(np.diff(pts) >= 0) and pts[-1] < nrow * ncol
    assert sum(v.nbytes for v in got.values()) <= 64_000_000
    again = _dump(tmp_path / "b", {"big": big, "small": small, "count": [17]})
    assert all(np.array_equal(got[k], again[k]) for k in got)


@pytest.mark.gpu
def test_plain_bench_times_the_headline_and_dumps_its_outputs(tmp_path):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR`: the result line with `ms_per_step` for
    exactly the steps asked for and nothing of `--full` (no cpu_baseline, no steady_state); the
    output chunk of the last timed step sampled as float64, finite, under 64 MB."""
    out_dir = tmp_path / "out"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in line
    assert "cpu_baseline" not in line and "steady_state" not in line
    files = sorted(os.listdir(out_dir))
    assert files == ["chain_output_points.npy", "chain_output_rows.npy"], files
    rows, pts = (np.load(out_dir / f) for f in ("chain_output_rows.npy", "chain_output_points.npy"))
    assert rows.dtype == pts.dtype == np.float64
    assert rows.shape == (4, 1 << 20) and pts.shape == (1 << 20,)
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(pts)) and np.any(rows != 0)
    assert rows.nbytes + pts.nbytes <= 64_000_000
