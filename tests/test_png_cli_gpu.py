"""inference.py --device_png and robot_demo.py --device_png against their default routes, with the tiny synthetic model and a forced
[SEG] answer (as tests/test_score_cli_gpu.py runs it): the same files under the same names, every mask pixel-equal and mode L, the
same --score report, no plane encoded on the host."""
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")


def _force(monkeypatch, batched):
    """Random-init models never emit [SEG]; force one so the mask branch of the CLI runs."""
    import torch
    import haff  # noqa: F401
    from haff import lisa
    orig = lisa.LisaMI355.evaluate

    def evaluate(self, *a, **kw):
        answer = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]])
        kw["forced_answer"] = answer.expand(a[2].shape[0], -1) if batched else answer
        kw["max_new_tokens"] = 3
        return orig(self, *a, **kw)
    monkeypatch.setattr(lisa.LisaMI355, "evaluate", evaluate)


def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _image(data):
    from PIL import Image
    return Image.open(io.BytesIO(data))


@pytest.mark.timeout(600)
def test_inference_device_png_equals_the_default_route(dev, tmp_path, monkeypatch, capsys):
    from haff import inference, png
    _force(monkeypatch, batched=True)
    encoders = []
    made = png.PngEncoder

    def counted():
        encoders.append(made())
        return encoders[-1]
    monkeypatch.setattr(png, "PngEncoder", counted)

    def run(tail, vis):
        return inference.main(["--synthetic", "tiny", "--benchmark-dir", SAMPLE, "--vis_save_path", str(tmp_path / vis / "th"),
                               "--image_size", "224", "--batch-size", "3", "--score"] + tail)
    want_report = run([], "plain")
    want_text = capsys.readouterr().out
    got_report = run(["--device_png"], "device")
    got_text = capsys.readouterr().out
    assert len(encoders) == 1 and encoders[0].host_encodes == 0      # every frame is 855 x 855 or smaller
    want, got = _files(tmp_path / "plain"), _files(tmp_path / "device")
    assert len(want) >= 20 and sorted(got) == sorted(want)
    on = 0
    for k in want:
        a, b = _image(want[k]), _image(got[k])
        assert a.mode == b.mode == "L" and a.size == b.size, k
        assert np.array_equal(np.asarray(a), np.asarray(b)), k
        assert got[k][:8] == b"\x89PNG\r\n\x1a\n" and got[k].count(b"IDAT") == 1
        on += int(np.asarray(b).any())
    assert on > 0                                                     # not vacuous: some written mask has pixels on
    assert got != want                                                # and the files do come from another encoder
    saved = [line.replace(str(tmp_path / "plain"), "").replace(str(tmp_path / "device"), "")
             for text in (want_text, got_text) for line in text.splitlines() if line.endswith("has been saved.")]
    assert len(saved) == 2 * len(want) and saved[:len(want)] == saved[len(want):]   # same lines, same order
    assert [r["count"] for r in got_report["per_threshold"]] == [4] * 5
    assert [r["threshold"] for r in got_report["per_threshold"]] == [r["threshold"] for r in want_report["per_threshold"]]
    for g, w in zip(got_report["per_threshold"], want_report["per_threshold"]):
        for k in ("count", "failed", "iou", "iocm", "hd", "directed_hd"):
            assert g[k] == w[k], (g["threshold"], k, g[k], w[k])
    assert got_report["best"]["threshold"] == want_report["best"]["threshold"]
    assert got_report["mean_average_precision"] == want_report["mean_average_precision"]


@pytest.mark.timeout(600)
def test_robot_demo_device_png_equals_the_default_route(dev, tmp_path, monkeypatch):
    from PIL import Image
    from haff import robot_demo
    _force(monkeypatch, batched=False)
    rng = np.random.default_rng(12)
    H, W, margins = 150, 224, (3, -2, 5, 1)
    Ho, Wo = H + margins[1] + margins[3], W + margins[0] + margins[2]
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks = {s: rng.integers(0, 256, (Ho, Wo), dtype=np.uint8) for s in ("left", "right")}
    trees = {}
    for route, flags in (("plain", []), ("device", ["--device_png"])):
        inp, out = tmp_path / route / "in", tmp_path / route / "out"
        inp.mkdir(parents=True)
        Image.fromarray(img).save(inp / "img.png")
        (inp / "prompt.txt").write_text("open the drawer\n")
        (inp / "margins.txt").write_text("3,-2,5,1\n")
        for s, m in masks.items():
            Image.fromarray(m).save(inp / f"mask_{s}.png")
        robot_demo.main(["--synthetic", "tiny", "--zed2_img_path", str(inp), "--vis_save_path", str(out), "--force_both",
                         "--image_size", "224", "--poll-interval", "0"] + flags, max_requests=1)
        trees[route] = _files(out)
    want, got = trees["plain"], trees["device"]
    assert sorted(got) == sorted(want) == ["aff_left.png", "aff_left_heat.png", "aff_right.png", "aff_right_heat.png", "cropped_img.png"]
    for k in want:
        if k in ("aff_left.png", "aff_right.png"):
            a, b = _image(want[k]), _image(got[k])
            assert a.mode == b.mode == "L" and b.size == (Wo, Ho) and np.array_equal(np.asarray(a), np.asarray(b)), k
            assert got[k] != want[k], k
        else:
            assert got[k] == want[k], k
    assert any(np.asarray(_image(got[k])).any() for k in ("aff_left.png", "aff_right.png"))
