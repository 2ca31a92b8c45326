"""bench.py with and without --full on the device: a plain run calls evaluate() exactly warm-up + K times and measures or checks
nothing else; --full adds the roofline, batch-1, CPU baseline and parity objects after the timed steps, and its gate passes."""
import contextlib
import io
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "tiny", "--batch", "2"]


def _run(bench, argv, monkeypatch):
    """bench.main(argv) with evaluate() calls counted: (exit code, the one stdout line, evaluate() calls)."""
    from haff.lisa import LisaMI355
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    calls = []
    evaluate = LisaMI355.evaluate

    def counted(self, *a, **kw):
        calls.append(1)
        return evaluate(self, *a, **kw)
    monkeypatch.setattr(LisaMI355, "evaluate", counted)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = bench.main(argv)
    lines = [l for l in buf.getvalue().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return rc, json.loads(lines[0]), len(calls)


def test_plain_run_times_the_steps_and_nothing_else(dev, tmp_path, monkeypatch):
    import bench

    def refused(*a, **kw):
        raise AssertionError("a plain bench run must not measure or check beyond the headline")
    for name in ("gemm_roofline", "train_gemm_roofline", "parity_vs_oracle", "parity_full_frame", "cpu_baseline", "cpu_full_frame",
                 "cpu_train_baseline", "GemmMeter"):
        monkeypatch.setattr(bench, name, refused)
    rc, line, n_eval = _run(bench, ARGS + ["--dump-outputs", str(tmp_path / "out")], monkeypatch)
    assert rc == 0 and n_eval == 1 + 2
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["roofline"] is None and line["cpu_baseline"] is None
    for k in ("parity", "latency_batch1_ms", "decode_step_batch1"):
        assert k not in line, k
    assert os.path.exists(tmp_path / "out" / "output_ids.npy")


def test_full_run_adds_every_measurement_and_passes_its_gate(dev, monkeypatch):
    import bench
    rc, line, n_eval = _run(bench, ARGS + ["--full"], monkeypatch)
    assert rc == 0 and n_eval > 1 + 2
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    rf = line["roofline"]
    assert rf["bound"] == "mfma" and rf["launches_per_step"] > 0 and 0 < rf["frac"] < 1
    assert line["latency_batch1_ms"] > 0 and line["decode_step_batch1"]["ms"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "frames/s"
    p = line["parity"]
    assert p["timed_mode"] == "bf16" and p["token_ids_equal"] is True and p["gate_failed"] == []
