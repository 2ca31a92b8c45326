"""robot_demo.py's device kernels (haff_robot_heatmap, haff_robot_mask) against the CPU restatement (tests/robot_ref.py), byte for
byte, and one request of the CLI end to end on the synthetic tiny model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/robot_ref.py
import robot_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 700), (224, 224), (720, 1280), (1024, 1024)]


def _fields(shape, rng):
    """the logit fields: random, a huge range, plateaus, values on (and one ulp around) integers after scaling"""
    H, W = shape
    yield "random", (rng.standard_normal(shape) * 6).astype(np.float32)
    yield "huge", (rng.standard_normal(shape) * 1e37).astype(np.float32)
    coarse = rng.integers(-3, 4, (H // 8 + 1, W // 8 + 1)).astype(np.float32) * 7.5
    yield "plateaus", np.ascontiguousarray(np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:H, :W])
    # min -5, max 250: scale 1, shift 5, so x + 5 hits every integer; one ulp below truncates one lower
    k = rng.integers(-5, 251, shape).astype(np.float32)
    side = rng.integers(-1, 2, shape)
    x = np.where(side < 0, np.nextafter(k, np.float32(-np.inf)), np.where(side > 0, np.nextafter(k, np.float32(np.inf)), k))
    x = np.clip(x, np.float32(-5), np.float32(250)).astype(np.float32)
    x.flat[0], x.flat[-1] = -5, 250
    yield "integers", x
    # a random range with values at the float32 preimages of integers (and their neighbours)
    mn, mx = np.float32(-3.7), np.float32(11.2)
    scale = 255.0 / (float(mx) - float(mn))
    sf, sh = np.float32(scale), np.float32(-float(mn) * scale)
    pre = ((rng.integers(0, 256, shape) - np.float64(sh)) / np.float64(sf)).astype(np.float32)
    pre = np.where(side < 0, np.nextafter(pre, np.float32(-np.inf)), np.where(side > 0, np.nextafter(pre, np.float32(np.inf)), pre))
    pre = np.clip(pre, mn, mx).astype(np.float32)
    pre.flat[0], pre.flat[-1] = mn, mx
    yield "preimages", pre


@pytest.mark.timeout(900)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_heatmap_and_mask_kernels_equal_the_restatement(dev, shape):
    import torch
    import haff
    from haff import ops, postprocess
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    H, W = shape
    fields = list(_fields(shape, rng))
    jet = torch.from_numpy(postprocess.jet_table()).to(dev)
    margin_sets = [(0, 0, 0, 0), (3, 2, 1, 4), (-1, 0, -2, 1), (5, -1, 0, 7)]
    for i, (name, x) in enumerate(fields):
        y = fields[(i + 1) % len(fields)][1]
        logits = torch.from_numpy(np.stack([x, y])).to(dev)
        heat = ops.robot_heatmap(logits, jet).cpu().numpy()
        for k, plane in enumerate((x, y)):
            ref = R.heatmap(plane)
            assert np.array_equal(heat[k], ref), (shape, name, k, int((heat[k] != ref).sum()))
        margins = margin_sets[i % len(margin_sets)]
        Ho, Wo = H + margins[1] + margins[3], W + margins[0] + margins[2]
        if Ho <= 0 or Wo <= 0:
            margins, Ho, Wo = (1, 1, 1, 1), H + 2, W + 2
        m = rng.integers(0, 256, (Ho, Wo), dtype=np.uint8)
        md = torch.from_numpy(m).to(dev)
        th = (-5, 0, 1, 3)[i % 4] if name != "integers" else 0
        got_heat, got = postprocess.robot_planes(logits, th, margins, [md, md])
        assert np.array_equal(got_heat.cpu().numpy(), heat)
        for k, plane in enumerate((x, y)):
            ref = R.pad_and_mask(plane, th, margins, m)
            assert np.array_equal(got[k].cpu().numpy(), ref), (shape, name, margins, th, k)
        # no mask: no AND (a mask of 255 everywhere in the restatement)
        nomask = ops.robot_mask(logits[0], -1.0, margins, None).cpu().numpy()
        assert np.array_equal(nomask, R.pad_and_mask(x, -1, margins, np.full((Ho, Wo), 255, np.uint8)))
    # a constant plane: JET[0] everywhere
    heat = ops.robot_heatmap(torch.full((1, H, W), 2.5, device=dev), jet).cpu().numpy()
    assert (heat == postprocess.jet_table()[0]).all()
    # a mask of another size is refused
    with pytest.raises(haff.HaffLibraryError):
        ops.robot_mask(logits[0], 0.0, (1, 1, 1, 1), torch.zeros((H + 2, W + 3), dtype=torch.uint8, device=dev))


@pytest.mark.timeout(600)
def test_robot_demo_end_to_end(dev, tmp_path, monkeypatch, capsys):
    import torch
    from PIL import Image
    import haff  # noqa: F401
    from haff import lisa, robot_demo
    rng = np.random.default_rng(12)
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    H, W = 150, 224
    margins = (3, -2, 5, 1)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    Image.fromarray(img).save(inp / "img.png")
    (inp / "prompt.txt").write_text("open the drawer\n")
    (inp / "margins.txt").write_text("3,-2,5,1\n")
    Ho, Wo = H + margins[1] + margins[3], W + margins[0] + margins[2]
    masks = {s: rng.integers(0, 256, (Ho, Wo), dtype=np.uint8) for s in ("left", "right")}
    for s, m in masks.items():
        Image.fromarray(m).save(inp / f"mask_{s}.png")
    captured = []
    orig = lisa.LisaMI355.evaluate

    def forced(self, *a, **kw):   # random-init models never emit [SEG]: force one so the mask branch runs
        kw["forced_answer"] = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]])
        kw["max_new_tokens"] = 3
        res = orig(self, *a, **kw)
        captured.append(res)
        return res
    monkeypatch.setattr(lisa.LisaMI355, "evaluate", forced)
    robot_demo.main(["--synthetic", "tiny", "--zed2_img_path", str(inp), "--vis_save_path", str(out), "--force_both",
                     "--image_size", "224", "--poll-interval", "0"], max_requests=1)
    text = capsys.readouterr().out
    assert len(captured) == 1
    _, left, right, tax = captured[0]
    assert tax[0].numel() != 0
    for side, pm in (("left", left), ("right", right)):
        x = pm[0][0].float().cpu().numpy()
        assert x.shape == (H, W)
        assert np.array_equal(np.asarray(Image.open(out / f"aff_{side}_heat.png")), R.heatmap(x)), side
        assert np.array_equal(np.asarray(Image.open(out / f"aff_{side}.png")), R.pad_and_mask(x, -5, margins, masks[side])), side
        assert f"aff_{side}.png has been saved." in text
    assert np.array_equal(np.asarray(Image.open(out / "cropped_img.png")), img)
    assert sorted(os.listdir(inp)) == ["mask_left.png", "mask_right.png"]
