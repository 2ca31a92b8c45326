"""bench.py --dump-outputs on the device: the timed step's outputs, identical from run to run with the same arguments (seeded
inputs and weights), and the line reports the --steps it was asked for."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_bench_dumps_the_same_outputs_twice(dev, tmp_path, monkeypatch):
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    for run in ("a", "b"):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rc = bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "tiny", "--batch", "2", "--no-cpu-baseline",
                             "--no-parity", "--no-b1", "--dump-outputs", str(tmp_path / run)])
        assert rc == 0
        lines = [l for l in buf.getvalue().splitlines() if l.strip()]
        line = json.loads(lines[-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["outputs_finite"] is True
    names = sorted(os.listdir(tmp_path / "a"))
    assert {"output_ids.npy", "pred_masks_left.npy", "pred_masks_right.npy", "taxonomies.npy"} <= set(names)
    assert names == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "output_ids.npy").shape[0] == 2
