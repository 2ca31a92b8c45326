"""inference.py --score_hausdorff_device (haff.scoring.BenchmarkScorer(hausdorff="device"), csrc/contour_hausdorff.hip) against the
host route --score_hausdorff, on the two leaf folders and the forced-[SEG] tiny model of
tests/test_score_cli_gpu.py::test_score_hausdorff_equals_the_reference_walk."""
import os
import shutil
import threading

import pytest

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")
FIELDS = ("count", "failed", "iou", "iocm", "hd", "directed_hd")
_HOST = {}                     # the host route's report of the two-leaf tree, computed by the first test that needs it


@pytest.fixture
def forced(monkeypatch):
    """Random-init models never emit [SEG]; force one so the mask branch of the CLI runs."""
    import torch
    import haff  # noqa: F401
    from haff import lisa
    orig = lisa.LisaMI355.evaluate

    def evaluate(self, *a, **kw):
        B = a[2].shape[0]
        kw["forced_answer"] = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]]).expand(B, -1)
        kw["max_new_tokens"] = 3
        return orig(self, *a, **kw)
    monkeypatch.setattr(lisa.LisaMI355, "evaluate", evaluate)


@pytest.fixture
def scorers(monkeypatch):
    """Every BenchmarkScorer the CLI builds, with `extra` keywords added to its constructor."""
    from haff import scoring
    made, extra = [], {}

    class Recorded(scoring.BenchmarkScorer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **extra))
            made.append(self)
    monkeypatch.setattr(scoring, "BenchmarkScorer", Recorded)
    return made, extra


def _bench(tmp_path):
    bench = tmp_path / "bench"
    for sub, leaf in (("P14_05", "0001413"), ("8f91bc0d-9ce7-4b31-aba7-dd59791917df", "00000029")):
        shutil.copytree(os.path.join(SAMPLE, sub, leaf), bench / sub / leaf)
    return str(bench)


def _run(argv_tail, bench, vis):
    from haff import inference
    return inference.main(["--synthetic", "tiny", "--benchmark-dir", bench, "--vis_save_path", vis, "--image_size", "224",
                           "--batch-size", "3"] + argv_tail)


def _host_report(bench, tmp_path):
    if "rep" not in _HOST:
        _HOST["rep"] = _run(["--score", "--score_hausdorff"], bench, str(tmp_path / "host" / "th"))
    return _HOST["rep"]


def _same(got, want):
    assert [r["threshold"] for r in got["per_threshold"]] == [r["threshold"] for r in want["per_threshold"]]
    for g, w in zip(got["per_threshold"], want["per_threshold"]):
        for k in FIELDS:
            assert g[k] == w[k], (g["threshold"], k, g[k], w[k])
    assert {k: got["best"][k] for k in FIELDS + ("threshold",)} == {k: want["best"][k] for k in FIELDS + ("threshold",)}
    assert got["mean_average_precision"] == want["mean_average_precision"]


def test_device_route_reports_what_the_host_route_reports(dev, tmp_path, forced, scorers, capsys):
    bench = _bench(tmp_path)
    want = _host_report(bench, tmp_path)
    made, _ = scorers
    del made[:]
    capsys.readouterr()
    rep = _run(["--score_only", "--score_hausdorff_device"], bench, str(tmp_path / "none" / "th"))
    text = capsys.readouterr().out
    _same(rep, want)
    assert not os.path.exists(tmp_path / "none")                                             # no file
    assert not [t for t in threading.enumerate() if t.name.startswith("haff-hausdorff")]     # no thread
    assert len(made) == 1 and made[0].hausdorff_device and made[0]._pool is None and made[0].host_walks == 0
    assert rep["best"]["hd"] is not None and rep["best"]["hd"] > 0
    assert f"Hausdorff-Distance: {rep['best']['hd']}" in text and f"Directed Hausdorff-Distance: {rep['best']['directed_hd']}" in text
    assert f"mean average precision: {rep['mean_average_precision']}" in text


def test_a_tiny_vertex_capacity_falls_back_to_the_host_walk(dev, tmp_path, forced, scorers):
    bench = _bench(tmp_path)
    want = _host_report(bench, tmp_path)
    made, extra = scorers
    del made[:]
    extra["max_vertices"] = 3
    rep = _run(["--score_only", "--score_hausdorff_device"], bench, str(tmp_path / "none" / "th"))
    _same(rep, want)
    assert len(made) == 1 and made[0].max_vertices == 3 and made[0].host_walks > 0
    assert not [t for t in threading.enumerate() if t.name.startswith("haff-hausdorff")]
