"""bench.py's stdout contract: ONE compact JSON line the driver can parse — round 5's line had grown to 20.7 KB
and BENCH_r05.json recorded `parsed: null`. compact_line() is a pure function of the full line object; the fixtures are full line
objects of round 5's tree kept under profiles/."""
import io
import json
import os
import sys
import contextlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _fixture(name):
    with open(os.path.join(ROOT, "profiles", name)) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", ["r5_final_bench7b_b64_benchline.json", "r5_final_bench13b_b8_benchline.json",
                                  "r5_final_train7b_b8_benchline.json"])
def test_compact_line_fits_the_budget_and_keeps_the_contract(name):
    full = _fixture(name)
    if full.get("parity"):
        full["parity"].setdefault("timed_mode", "fp32" if full["dtype"] == "f32" else "bf16")
    assert len(json.dumps(full)) > bench.LINE_BUDGET_BYTES      # the fixture IS one of the lines that were too long
    line = bench.compact_line(full)
    text = json.dumps(line)
    assert len(text) <= bench.LINE_BUDGET_BYTES, len(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == pytest.approx(full["value"], rel=1e-3) and line["config"]["workload"]
    rf = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["frac"] == pytest.approx(full["roofline"]["achieved"] / full["roofline"]["peak"], rel=1e-3)
    if full.get("cpu_baseline"):
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in line["cpu_baseline"], k
    if full.get("parity"):
        p = line["parity"]
        assert p["timed_mode"] in ("bf16", "fp32", "bf16_fp32_stream", "bf16_fp32_stream_f32neck")
        assert 0.9 < p["mask_iou_min"] <= 1.0 and isinstance(p["gate_failed"], list)
        want = full["parity"]["full_frame"][p["timed_mode"]]["mask_iou_min"]
        assert p["mask_iou_min"] == pytest.approx(want, abs=1e-5)        # the IoU printed belongs to the mode that was timed
        assert p["meets_iou_0.999"] == (want >= 0.999)


def test_compact_line_survives_absurdly_long_free_text():
    full = _fixture("r5_final_bench7b_b64_benchline.json")
    full["config"]["workload"] = "w" * 5000
    full["cpu_baseline"]["sample"] = "s" * 5000
    full["roofline"]["kernel"] = "k" * 5000
    assert len(json.dumps(bench.compact_line(full))) <= bench.LINE_BUDGET_BYTES
    # even a config object stuffed with junk cannot keep the line from being printed within the budget
    full["config"].update({"junk%d" % i: "x" * 200 for i in range(40)})
    line = bench.compact_line(full)
    assert len(json.dumps(line)) <= bench.LINE_BUDGET_BYTES and line["value"] == full["value"] and "frac" in line["roofline"]


def test_stub_run_prints_exactly_one_line_within_the_budget(tmp_path, monkeypatch):
    env_keys = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")
    for k in env_keys:
        monkeypatch.delenv(k, raising=False)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--stub-step-ms", "5", "--batch", "3"])
    lines = [l for l in buf.getvalue().splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) <= bench.LINE_BUDGET_BYTES
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["steps"] == 2 and line["config"]["stub"] is True and line["cpu_baseline"] is None
    detail = os.path.join(ROOT, line["detail"])
    assert os.path.exists(detail) and json.load(open(detail))["steps"] == 2


def _fake_evaluate_out(seed):
    """evaluate()'s return value at 3 frames of 640^2: ids, per-frame left / right masks and taxonomies of one [SEG] each."""
    import torch
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 32000, (3, 9), generator=g)
    masks = lambda: [torch.randn((1, 640, 640), generator=g) for _ in range(3)]   # noqa: E731
    return ids, masks(), masks(), [torch.randn((1, 4), generator=g) for _ in range(3)]


def test_dump_outputs_writes_every_output_within_the_budget(tmp_path):
    """--dump-outputs: float32 / float64 .npy files of what evaluate() returned; an array over DUMP_SAMPLE elements (the masks: 3 x
    640^2) is a fixed sample of its flat elements with the positions beside it; the same outputs give the same files."""
    import numpy as np
    import torch
    out = _fake_evaluate_out(0)
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["output_ids.npy", "pred_masks_left.npy", "pred_masks_left_index.npy", "pred_masks_right.npy",
                     "pred_masks_right_index.npy", "taxonomies.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / "b" / n)), n
    assert got["output_ids"].dtype == np.float64 and np.array_equal(got["output_ids"], out[0].numpy())
    assert got["taxonomies"].dtype == np.float32 and np.array_equal(got["taxonomies"], torch.cat(out[3]).numpy())
    for side, masks in (("left", out[1]), ("right", out[2])):
        v, idx = got[f"pred_masks_{side}"], got[f"pred_masks_{side}_index"]
        assert v.dtype == np.float32 and idx.dtype == np.float64 and 0.6 * bench.DUMP_SAMPLE < v.size <= bench.DUMP_SAMPLE
        flat = torch.cat(masks).reshape(-1).numpy()
        assert idx[-1] < flat.size and np.all(np.diff(idx) > 0) and np.array_equal(v, flat[idx.astype(np.int64)])
    bench.dump_outputs(_fake_evaluate_out(1), str(tmp_path / "c"))      # other outputs: same positions, other values
    assert np.array_equal(np.load(tmp_path / "c" / "pred_masks_left_index.npy"), got["pred_masks_left_index"])
    assert not np.array_equal(np.load(tmp_path / "c" / "pred_masks_left.npy"), got["pred_masks_left"])


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--stub-step-ms", "5", "--dump-outputs", "x"],
                                  ["--mode", "train", "--dump-outputs", "x"]])
def test_bench_refuses_arguments_it_cannot_honour(argv, monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "1"] + argv)
    assert "bench.py:" in str(e.value)
