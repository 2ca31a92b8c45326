"""tests/overlay_ref.py pinned on hand-derived values, evaluation.create_overlay (the host route of --visualize) pinned against it,
the captions' positions, the panel files, and the CLI flags of both routes. CPU only."""
import os

import numpy as np
import pytest

import haff  # noqa: F401
from haff import evaluation as ev

import overlay_ref as O
import score_ref as R

SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")
BAND_CAP = 1e-4            # tests/test_score_ref_cpu.py: the share of target pixels the near-tie band holds on the sample's planes


def test_blend_bytes_by_hand():
    """(frame byte, first layer byte, second layer byte) -> output, each worked by hand with alpha = (0.5, 1), beta = (0.5, 0.5)."""
    def two(v, first, second):
        return O.blend_byte(O.blend_byte(v, 0.5, first, 0.5, 0.0), 1.0, second, 0.5, 0.0)
    assert two(1, 0, 0) == 0            # 0.5 -> 0 (half to even), 0 + 0 -> 0
    assert two(3, 0, 0) == 2            # 1.5 -> 2
    assert two(0, 255, 0) == 128        # 127.5 -> 128
    assert two(1, 0, 255) == 128        # 0.5 -> 0, then rint(0 + 127.5) = 128
    assert two(255, 255, 0) == 255      # 127.5 + 127.5 = 255 exactly
    assert two(255, 0, 255) == 255      # 127.5 -> 128, 128 + 127.5 = 255.5 -> 256: saturates
    assert two(254, 0, 0) == 127 and two(2, 0, 0) == 1 and two(5, 0, 0) == 2          # 2.5 -> 2
    # the channels of a pixel under both hands: red from the left layer, green from the right one, blue from neither
    frame = np.full((1, 1, 3), 255, np.uint8)
    on = np.ones((1, 1), bool)
    assert O.overlay(frame, on, on).tolist() == [[[255, 255, 128]]]
    assert O.overlay(frame, on, None).tolist() == [[[255, 128, 128]]]
    assert O.overlay(frame, None, on).tolist() == [[[128, 255, 128]]]
    assert O.overlay(frame, None, None).tolist() == [[[128, 128, 128]]]               # both blends always run: the frame is halved
    assert O.overlay(np.array([[[1, 3, 0]]], np.uint8), None, None).tolist() == [[[0, 2, 0]]]


def test_blend_table_is_the_scalar_rule_for_every_byte():
    for c in range(3):
        t = O.blend_table(c)
        for v in (0, 1, 2, 3, 127, 128, 254, 255):
            for left in (0, 1):
                for right in (0, 1):
                    t1 = O.blend_byte(v, 0.5, O.COLORS[0][c] * left, 0.5, 0.0)
                    assert t[v, left, right] == O.blend_byte(t1, 1.0, O.COLORS[1][c] * right, 0.5, 0.0)
    # with create_overlay's weights every product and sum is exact in fp32: the double-precision value gives the same byte
    for v in range(256):
        for b in (0, 255):
            exact = v * 0.5 + b * 0.5
            assert O.blend_byte(v, 0.5, b, 0.5, 0.0) == min(255, round(exact))


def test_nearest_index_is_opencvs_double_rule():
    cols = O.nearest_index(34, 6)
    assert cols[17] == 2                                       # 17 * (1 / (34 / 6)) = 2.9999999999999996, not the rational 3
    assert cols[:6] == [0, 0, 0, 0, 0, 0] and cols[-1] == 5 and len(cols) == 34
    assert O.nearest_index(7, 7) == list(range(7))
    assert O.nearest_index(3, 9) == [0, 3, 6] and O.nearest_index(256, 855)[-1] == 851
    from haff import cvlite
    for n_dst, n_src in ((34, 6), (29, 7), (256, 855), (855, 256), (7, 13), (1, 5), (5, 1)):
        assert cvlite.nearest_indices(n_dst, n_src).tolist() == O.nearest_index(n_dst, n_src)
    img = np.arange(6, dtype=np.uint8)[None, :]
    assert cvlite.resize_nearest(img, (34, 1))[0].tolist() == cols


@pytest.mark.parametrize("hw", [(1, 1), (7, 34), (16, 64), (33, 29)])
def test_create_overlay_equals_the_restatement_on_identity_sizes(hw):
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    frame = rng.integers(0, 256, hw + (3,)).astype(np.uint8)
    frame.reshape(-1)[:8] = [0, 1, 2, 3, 254, 255, 127, 128][:frame.size]
    left, right = rng.random(hw) < 0.5, rng.random(hw) < 0.5
    assert np.array_equal(ev.create_overlay(frame, left, right), O.overlay(frame, left, right))
    assert np.array_equal(ev.create_overlay(frame, None, right), O.overlay(frame, None, right))
    assert np.array_equal(ev.create_overlay(frame, left, np.zeros((0, 0))), O.overlay(frame, left, None))


def test_create_overlay_resizes_by_the_nearest_rule():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (34, 29, 3)).astype(np.uint8)
    left, right = rng.random((6, 7)) < 0.5, rng.random((6, 7)) < 0.5
    assert np.array_equal(ev.create_overlay(frame, left, right), O.overlay(frame, left, right))
    frame = rng.integers(0, 256, (7, 34, 3)).astype(np.uint8)
    left, right = rng.random((13, 6)) < 0.5, rng.random((13, 6)) < 0.5
    assert np.array_equal(ev.create_overlay(frame, left, right), O.overlay(frame, left, right))


def test_sample_overlays_differ_only_inside_the_near_tie_band():
    """The sample's object masks as 256 x 256 predictions, taken to 855 x 855 by evaluation's fp32 resize and by the exact rule, drawn
    over the 256 x 256 frame: the two overlays may differ only where the frame pixel reads a target pixel of the near-tie band."""
    from PIL import Image
    seen = 0
    for sub in sorted(os.listdir(SAMPLE)):
        if not os.path.isdir(os.path.join(SAMPLE, sub)):
            continue
        for leaf in sorted(os.listdir(os.path.join(SAMPLE, sub))):
            frame = np.asarray(Image.open(os.path.join(SAMPLE, sub, leaf, "inpainting.png")).convert("RGB"))
            assert frame.shape == (256, 256, 3)
            small, theirs, ours, band = {}, {}, {}, np.zeros((855, 855), bool)
            for side in ("left", "right"):
                p = os.path.join(SAMPLE, sub, leaf, f"obj_{side}.png")
                if not os.path.exists(p):
                    theirs[side] = ours[side] = None
                    continue
                small[side] = R.resample_on(np.asarray(Image.open(p).convert("L")) > 0, (256, 256))
                theirs[side] = ev._resize_bilinear(small[side].astype(np.uint8) * 255, (855, 855)) > 0
                ours[side] = R.resample_on(small[side], (855, 855))
                ties = R.near_tie(small[side], (855, 855))
                assert ties.sum() <= BAND_CAP * ties.size
                assert np.array_equal(theirs[side][~ties], ours[side][~ties])
                band |= ties
                seen += 1
            a = ev.create_overlay(frame, theirs["left"], theirs["right"])
            b = O.overlay(frame, ours["left"], ours["right"])
            rows, cols = np.asarray(O.nearest_index(256, 855)), np.asarray(O.nearest_index(256, 855))
            differ = (a != b).any(axis=2)
            assert not differ[~band[rows][:, cols]].any()
            assert differ.sum() <= 2 * BAND_CAP * 855 * 855
            assert (a != np.asarray(frame)).any()                # something was drawn
    assert seen == 6


def test_caption_positions_and_panel_files(tmp_path):
    from PIL import Image, ImageFont
    font = ImageFont.load_default()
    wf = 120
    texts = ev.panel_captions("vid/0001", "Aff-Ex", 0.123449, wf)
    assert [t for t, _ in texts] == ["vid/0001", "Aff-Ex", "IoU: 0.1234"] and [x for _, x in texts] == [-wf, -2 * wf, 10]
    black = np.zeros((40, 2 * wf, 3), np.uint8)
    img = np.asarray(ev.draw_captions(black, texts))
    assert img.shape == black.shape and img.any()
    lit = np.flatnonzero(img.any(axis=(0, 2)))
    # the three texts start at x = 10, Wf - tw - 10 and 2 Wf - tw - 10 (tw = font.getbbox(text)[2]) and end before the panel's edge
    tw = [font.getbbox(t)[2] for t, _ in texts]
    starts = [wf - tw[0] - 10, 2 * wf - tw[1] - 10, 10]
    for s, w in zip(starts, tw):
        inside = lit[(lit >= s) & (lit <= s + w)]
        assert inside.size and not img[:10].any()
    assert lit.min() >= 10 and lit.max() <= 2 * wf - 10 and not np.any((lit > wf - 10) & (lit < 2 * wf - tw[1] - 10))
    assert np.array_equal(np.asarray(ev.draw_captions(black, [])), black)
    # the files of :272-301
    bench, pred = np.full((40, wf, 3), 10, np.uint8), np.full((40, wf, 3), 200, np.uint8)
    p = ev.write_panel(str(tmp_path), "vid", "0001", "Aff-Ex", 0.5, bench, pred)
    assert p == str(tmp_path / "vid_0001_concatenated.png")
    got = np.asarray(Image.open(p))
    assert got.shape == (40, 2 * wf, 3) and np.array_equal(got[30:], np.concatenate([bench, pred], axis=1)[30:])
    assert ev.write_panel(str(tmp_path), "vid", "0002", ".", 0.2, None, pred) is None            # not above 0.2
    assert ev.write_panel(str(tmp_path), "vid", "0002", ".", 0.2, None, pred, keep_all=True) == str(tmp_path / "vid_0002.png")
    p = ev.write_panel(str(tmp_path), "vid", "0003", ".", 0.21, None, pred)
    assert np.array_equal(np.asarray(Image.open(p)), pred)                                       # the prediction overlay alone, no text
    assert sorted(os.listdir(tmp_path)) == ["vid_0001_concatenated.png", "vid_0002.png", "vid_0003.png"]


def _write(path, plane_bool):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(plane_bool.astype(np.uint8) * 255).save(path)


def test_evaluation_visualize_on_the_sample(tmp_path):
    """evaluation.py --visualize over the sample's object masks written as predictions at 855 x 855 (no resize, so no band): every
    panel is the restatement's two overlays side by side under draw_captions, and its IoU is evaluate_folders' for the frame."""
    from PIL import Image
    pred = tmp_path / "pred"
    labels = []
    for sub in sorted(os.listdir(SAMPLE)):
        if not os.path.isdir(os.path.join(SAMPLE, sub)):
            continue
        for leaf in sorted(os.listdir(os.path.join(SAMPLE, sub))):
            labels.append((sub, leaf))
            for side in ("left", "right"):
                op = os.path.join(SAMPLE, sub, leaf, f"obj_{side}.png")
                if os.path.exists(op):
                    _write(str(pred / sub / leaf / f"aff_{side}.png"), np.asarray(Image.open(op).convert("L")) > 0)
    out = tmp_path / "panels"
    done = ev.main(["--benchmark_folder", SAMPLE, "--comparison_folder", str(pred), "--visualize", "--visualize-dir", str(out),
                    "--num-examples", "3"])
    assert [d[0] for d in done] == [f"{s}/{l}" for s, l in labels[:3]]           # sorted order, the first three
    assert sorted(os.listdir(out)) == sorted(f"{s}_{l}_concatenated.png" for s, l in labels[:3])
    for (sub, leaf), (_, iou, path) in zip(labels, done):
        res = ev.score_frame(os.path.join(SAMPLE, sub, leaf), str(pred / sub / leaf), (855, 855))
        assert iou == res[0]
        frame = np.asarray(Image.open(os.path.join(SAMPLE, sub, leaf, "inpainting.png")).convert("RGB"))
        planes = {}
        for who, root in (("gt", os.path.join(SAMPLE, sub, leaf)), ("pr", str(pred / sub / leaf))):
            for side in ("left", "right"):
                p = os.path.join(root, f"aff_{side}.png")
                planes[who, side] = np.asarray(Image.open(p).convert("L")) > 0 if os.path.exists(p) else None
        canvas = np.concatenate([O.overlay(frame, planes["gt", "left"], planes["gt", "right"]),
                                 O.overlay(frame, planes["pr", "left"], planes["pr", "right"])], axis=1)
        want = np.asarray(ev.draw_captions(canvas, ev.panel_captions(f"{sub}/{leaf}", "Aff-Ex", iou, frame.shape[1])))
        assert np.array_equal(np.asarray(Image.open(path)), want)
    # --files_folder: only the listed frames; the caption "." writes the prediction overlay alone, every listed frame kept
    listing = tmp_path / "listing"
    os.makedirs(listing)
    for sub, leaf in (labels[0], labels[2]):
        open(listing / f"{sub}_{leaf}.png", "w").close()
    out2 = tmp_path / "panels2"
    done = ev.main(["--benchmark_folder", SAMPLE, "--comparison_folder", str(pred), "--visualize", "--visualize-dir", str(out2),
                    "--caption", ".", "--files_folder", str(listing)])
    assert sorted(os.listdir(out2)) == sorted(f"{s}_{l}.png" for s, l in (labels[0], labels[2]))
    for flag in (["--map"], ["--only", "ego"], ["--intersection"]):
        with pytest.raises(SystemExit, match=flag[0]):
            ev.main(["--benchmark_folder", SAMPLE, "--comparison_folder", str(pred), "--visualize", "--visualize-dir", str(out)] + flag)


def test_inference_visualize_flags():
    from haff import inference
    a = inference.parse_args(["--benchmark-dir", "b", "--score_only"])
    assert a.visualize is None and a.visualize_threshold == 0.5 and a.visualize_caption == "Aff-Ex" and a.visualize_examples == 20
    a = inference.parse_args(["--benchmark-dir", "b", "--score", "--visualize", "d", "--visualize_threshold", "0.7",
                              "--visualize_caption", ".", "--visualize_examples", "0"])
    assert (a.visualize, a.visualize_threshold, a.visualize_caption, a.visualize_examples) == ("d", 0.7, ".", 0)
    for bad in (["--benchmark-dir", "b", "--visualize", "d"], ["--benchmark-dir", "b", "--score", "--visualize_threshold", "0.5"],
                ["--benchmark-dir", "b", "--score", "--visualize_caption", "x"], ["--benchmark-dir", "b", "--score", "--visualize_examples", "3"],
                ["--benchmark-dir", "b", "--score", "--visualize", "d", "--visualize_threshold", "0.55"],
                ["--benchmark-dir", "b", "--score", "--visualize", "d", "--visualize_examples", "-1"]):
        with pytest.raises(SystemExit):
            inference.parse_args(bad)


def test_pack_vis_layout():
    """The record as include/haff_hip.h lays it out, from tensors that only have to answer data_ptr / shape / stride."""
    import torch
    from haff import scoring

    class Fake:
        def __init__(self, ptr, shape, dtype, stride=None):
            self._ptr, self.shape, self.dtype, self._stride, self.is_cuda = ptr, torch.Size(shape), dtype, stride, True

        def data_ptr(self):
            return self._ptr

        def is_contiguous(self):
            return True

        def dim(self):
            return len(self.shape)

        def stride(self, k):
            return self._stride[k]

    rgb = Fake(0x1000, (7, 34, 3), torch.uint8)
    row, col = Fake(0x2000, (7,), torch.int32), Fake(0x3000, (34,), torch.int32)
    out0, out1 = Fake(0x4000, (7, 34, 3), torch.uint8, (204, 3, 1)), Fake(0x4000 + 102, (7, 34, 3), torch.uint8, (204, 3, 1))
    t = scoring.pack_vis([{"rgb": rgb, "row": row, "col": col, "out": (out0, out1), "t": 2},
                          {"rgb": rgb, "row": None, "col": None, "out": (None, out1), "t": 0, "alpha": (0.25, 0.75), "beta": (1.0, 2.0),
                           "gamma": 3.0, "colors": ((1, 2, 3), (4, 5, 6))}])
    assert t.shape == (2, 16) and t.dtype == np.int64
    assert t[0, :7].tolist() == [0x1000, 0x2000, 0x3000, 0x4000, 0x4000 + 102, 204, 204]
    ints, floats = t.view(np.int32).reshape(2, 32), t.view(np.float32).reshape(2, 32)
    assert ints[0, 14:17].tolist() == [7, 34, 2] and floats[0, 17:22].tolist() == [0.5, 1.0, 0.5, 0.5, 0.0]
    assert ints[0, 22:28].tolist() == [255, 0, 0, 0, 255, 0] and not ints[0, 28:].any()
    assert t[1, :7].tolist() == [0x1000, 0, 0, 0, 0x4000 + 102, 0, 204]
    assert floats[1, 17:22].tolist() == [0.25, 0.75, 1.0, 2.0, 3.0] and ints[1, 22:28].tolist() == [1, 2, 3, 4, 5, 6]
    # pack_frames records the frame's record number in the descriptor's first spare word
    frames = scoring.pack_frames([{"left": None, "right": None, "target_hw": (4, 4), "src_hw": (2, 2)},
                                  {"left": None, "right": None, "target_hw": (4, 4), "src_hw": (2, 2), "vis": 1}])
    assert frames.view(np.int32).reshape(2, 32)[:, 29].tolist() == [0, 1] and not frames.view(np.int32).reshape(2, 32)[:, 30:].any()
