"""--precision fp16 through the reference's CLIs (synthetic tiny model: the bf16 weight values of the same seed, so both
precisions run one model; byte tokenizer; a forced [SEG] answer so the mask branch runs)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _png(path, h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(path)


def _force_seg(monkeypatch, lisa, first):
    orig = lisa.LisaMI355.evaluate

    def forced(self, *a, **kw):
        import torch
        kw["forced_answer"] = torch.tensor([[first, self.cfg.seg_token_idx, self.cfg.eos_token_id]])
        kw["max_new_tokens"] = 3
        return orig(self, *a, **kw)
    monkeypatch.setattr(lisa.LisaMI355, "evaluate", forced)


def test_inference_cli_fp16_matches_bf16_planes(dev, tmp_path, monkeypatch):
    import haff  # noqa: F401
    from haff import inference, lisa
    from PIL import Image
    bench = tmp_path / "bench" / "kitchen"
    for i, (h, w) in enumerate(((150, 224), (224, 180))):
        d = bench / f"clip{i}"
        d.mkdir(parents=True)
        _png(d / "inpainting.png", h, w, i)
        (d / "annotation.json").write_text(json.dumps({"narration": "open drawer"}))
    _force_seg(monkeypatch, lisa, 5)
    planes = {}
    for prec in ("bf16", "fp16"):
        out = tmp_path / f"vis_{prec}_"
        inference.main(["--synthetic", "tiny", "--precision", prec, "--benchmark-dir", str(tmp_path / "bench"), "--vis_save_path",
                        str(out), "--image_size", "224"])
        found = {}
        for th in (0.1, 0.2, 0.3, 0.5, 0.7):
            for i in range(2):
                for side in ("left", "right"):
                    p = f"{out}{th}/kitchen/clip{i}/aff_{side}.png"
                    if os.path.exists(p):
                        found[(th, i, side)] = np.asarray(Image.open(p))
        planes[prec] = found
    assert planes["fp16"] and set(planes["fp16"]) == set(planes["bf16"])
    for key, a in planes["fp16"].items():
        b = planes["bf16"][key]
        agree = float((a == b).mean())
        print(f"{key}: fp16 / bf16 planes agree on {agree:.5f} of the pixels")
        assert a.shape == b.shape and agree >= 0.99, (key, agree)


def test_chat_cli_fp16_roundtrip(dev, tmp_path, monkeypatch, capsys):
    import haff  # noqa: F401
    from haff import chat, lisa
    img = tmp_path / "mug.png"
    _png(img, 224, 200, 1)
    _force_seg(monkeypatch, lisa, 7)
    answers = iter(["Where would you hold the mug?", str(img)])
    chat.main(["--synthetic", "tiny", "--precision", "fp16", "--vis_save_path", str(tmp_path / "vis"), "--image_size", "224"],
              input_fn=lambda _: next(answers), max_turns=1)
    text = capsys.readouterr().out
    assert "text_output:" in text and "[SEG]" in text
    for name in ("mug_mask_left0.jpg", "mug_mask_right0.jpg", "mug_masked_img_0.jpg"):
        assert os.path.exists(tmp_path / "vis" / name)
