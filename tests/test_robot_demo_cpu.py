"""robot_demo.py (the reference's 2Haff/robot_demo.py on the MI355X path), host side: the flags, properties of the CPU restatement
(tests/robot_ref.py), the two entry points' declarations and host-side refusals, and the file protocol with a stub model.
Nothing here computes on a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import haff
from haff import postprocess, robot_demo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/robot_ref.py
import robot_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("haff_robot_heatmap", "haff_robot_mask")

# 2Haff/robot_demo.py:22-55, by hand: dest -> default
REFERENCE_FLAGS = {
    "version": "aff_weights", "vis_save_path": "./robot_demo/out", "force_left": False, "force_right": False,
    "force_both": False, "precision": "bf16", "image_size": 1024, "model_max_length": 512, "lora_r": 8,
    "vision_tower": "openai/clip-vit-large-patch14", "local_rank": 0, "load_in_8bit": False, "load_in_4bit": False,
    "use_mm_start_end": True, "conv_type": "llava_v1", "zed2_img_path": "robot_demo/in", "th": -5,
}
REFERENCE_OPTIONS = {"--version", "--vis_save_path", "--force_left", "--force_right", "--force_both", "--precision",
                     "--image_size", "--model_max_length", "--lora_r", "--vision-tower", "--local-rank", "--load_in_8bit",
                     "--load_in_4bit", "--use_mm_start_end", "--conv_type", "--zed2_img_path", "--th"}
PORT_OPTIONS = {"--synthetic", "--sam-checkpoint", "--max-new-tokens", "--poll-interval"}


def test_flags_and_defaults_are_the_reference_ones():
    args = vars(robot_demo.parse_args([]))
    for dest, default in REFERENCE_FLAGS.items():
        assert args[dest] == default and type(args[dest]) is type(default), dest
    assert set(args) == set(REFERENCE_FLAGS) | {"synthetic", "sam_checkpoint", "max_new_tokens", "poll_interval"}
    assert args["max_new_tokens"] == 512            # robot_demo.py:261
    a = robot_demo.parse_args(["--th", "3", "--force_both", "--precision", "fp16", "--conv_type", "llava_llama_2"])
    assert a.th == 3 and a.force_both and a.precision == "fp16"
    for bad in (["--th", "0.5"], ["--precision", "int8"], ["--conv_type", "x"]):
        with pytest.raises(SystemExit):
            robot_demo.parse_args(bad)
    src = open(robot_demo.__file__).read()
    assert set(re.findall(r'add_argument\(\s*"(--[\w-]+)"', src)) == REFERENCE_OPTIONS | PORT_OPTIONS


@pytest.mark.parametrize("flag", ["--load_in_8bit", "--load_in_4bit"])
def test_quantised_loading_exits_as_in_inference(flag):
    args = robot_demo.parse_args([flag, "--synthetic", "tiny"])
    with pytest.raises(SystemExit, match="bitsandbytes"):
        robot_demo.build_model_and_tokenizer(args)


def test_jet_table_and_blur_coefficients():
    jet = postprocess.jet_table()
    assert jet.dtype == np.uint8 and jet.shape == (256, 3)
    assert np.array_equal(jet, R.jet_table())                     # two restatements of Octave's jet, written apart
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[255]) == (128, 0, 0)    # cv2: BGR (128,0,0) and (0,0,128)
    assert tuple(jet[128]) == (130, 255, 126)
    assert R.gaussian_coeffs() == (14, 62, 104, 62, 14)           # the constants of csrc/robot_post.hip
    assert sum(R.gaussian_coeffs()) == 256


def test_fma32_rounds_once():
    x = np.float32(1 + 2 ** -12)                   # x * x = 1 + 2^-11 + 2^-24: a float32 midpoint
    assert R.fma32(x, x, np.float32(0)) == np.float32(1 + 2 ** -11)                        # tie to even
    assert R.fma32(x, x, np.float32(2 ** -70)) == np.float32(1 + 2 ** -11 + 2 ** -23)     # lost in a double sum
    assert R.fma32(x, x, np.float32(-2 ** -70)) == np.float32(1 + 2 ** -11)


@pytest.mark.parametrize("margins", [(0, 0, 0, 0), (3, 2, 1, 4), (-2, -1, -3, -2), (-1, 3, 2, -4), (4, -2, -1, 0)])
def test_padding_follows_pil_paste(margins):
    rng = np.random.default_rng(sum(margins) + 20)
    left, top, right, bottom = margins
    x = rng.standard_normal((9, 11)).astype(np.float32) * 6
    Ho, Wo = 9 + top + bottom, 11 + left + right
    mask = rng.integers(0, 256, (Ho, Wo), dtype=np.uint8)
    got = R.pad_and_mask(x, -1, margins, mask)
    exp = np.zeros((Ho, Wo), np.uint8)
    for y in range(9):
        for xx in range(11):
            yy, xo = y + top, xx + left
            if 0 <= yy < Ho and 0 <= xo < Wo and x[y, xx] > -1 and mask[yy, xo] & 1:
                exp[yy, xo] = 255
    assert np.array_equal(got, exp)
    with pytest.raises(ValueError):
        R.pad_and_mask(x, -1, margins, mask[:, 1:])


def test_mask_and_keeps_odd_values_only():
    x = np.full((2, 6), 3.0, np.float32)
    m = np.array([[0, 1, 2, 3, 254, 255]] * 2, np.uint8)
    assert R.pad_and_mask(x, 0, (0, 0, 0, 0), m).tolist() == [[0, 255, 0, 255, 0, 255]] * 2


def test_threshold_of_one_or_more_clears_every_pixel():
    """`pred_mask[pred_mask > th] = 1` then `pred_mask[pred_mask <= th] = 0`: for th >= 1 the ones are cleared again"""
    x = np.linspace(-10, 10, 40, dtype=np.float32).reshape(4, 10)
    m = np.full((4, 10), 255, np.uint8)
    assert R.pad_and_mask(x, 0, (0, 0, 0, 0), m).any()
    for th in (1, 3):
        assert not R.pad_and_mask(x, th, (0, 0, 0, 0), m).any()


def test_missing_mask_falls_back_to_the_other_hand():
    ml, mr = np.zeros((2, 2), np.uint8), np.ones((2, 2), np.uint8)
    assert robot_demo.and_mask("left", ml, mr) is ml and robot_demo.and_mask("right", ml, mr) is mr
    assert robot_demo.and_mask("left", None, mr) is mr and robot_demo.and_mask("right", ml, None) is ml
    x = np.full((2, 2), 5.0, np.float32)
    assert np.array_equal(R.pad_and_mask(x, 0, (0, 0, 0, 0), None, mr), np.full((2, 2), 255, np.uint8))


def test_constant_plane_maps_to_jet_zero():
    jet0 = R.jet_table()[0]
    for shape in ((1, 1), (3, 7), (16, 5)):
        h = R.heatmap(np.full(shape, 7.25, np.float32))
        assert h.shape == shape + (3,) and (h == jet0).all()
    # a difference at or below DBL_EPSILON counts as constant too (scale 0)
    assert (R.normalize_u8(np.array([1.0, np.nextafter(np.float32(1.0), np.float32(2))], np.float32)) != 0).any()
    assert (R.normalize_u8(np.array([0.0, 1e-17], np.float32)) == 0).all()


def test_maximum_can_truncate_to_254():
    """fmaf(max, (float)scale, (float)shift) lands just below 255 for many (min, max): np.uint8 truncates it to 254"""
    rng = np.random.default_rng(1)
    seen = set()
    for _ in range(400):
        mn = rng.uniform(-50, 50)
        x = np.array([mn, mn + rng.uniform(0.1, 100)], np.float32)
        q = R.normalize_u8(x)
        assert q[0] == 0
        seen.add(int(q[1]))
    assert seen == {254, 255}


def test_blur_symmetry_and_constant_images():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    b = R.blur5(img)
    assert np.array_equal(R.blur5(img[:, ::-1]), b[:, ::-1])
    assert np.array_equal(R.blur5(img[::-1]), b[::-1])
    assert np.array_equal(R.blur5(img.transpose(1, 0, 2)), b.transpose(1, 0, 2))
    for shape in ((1, 1, 3), (2, 3, 3), (5, 5, 3)):
        for v in (0, 1, 128, 255):
            assert (R.blur5(np.full(shape, v, np.uint8)) == v).all()
    # one bright pixel spreads as the outer product of the coefficients
    dot = np.zeros((9, 9, 1), np.uint8)
    dot[4, 4] = 255
    c = np.array(R.gaussian_coeffs())
    assert np.array_equal(R.blur5(dot)[2:7, 2:7, 0], (np.outer(c, c) * 255 + 32768) >> 16)


def test_entry_points_declared_and_refuse_bad_shapes_on_the_host():
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    for name in ENTRY:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
        assert name in haff.EXPORTED_SYMBOLS
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    lib = haff.load_library()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    # mask: the padded size is 6 x 7 (4 x 5 + margins 1,1,1,1): a 6 x 6 or 7 x 7 mask is refused, as cv2.bitwise_and raises
    assert lib.haff_robot_mask(p, 4, 5, 1, 1, 1, 1, 0.0, p, 6, 6, 255, p, None) == -1
    assert lib.haff_robot_mask(p, 4, 5, 1, 1, 1, 1, 0.0, p, 7, 7, 255, p, None) == -1
    assert lib.haff_robot_mask(p, 4, 5, -3, 0, -2, 0, 0.0, None, 0, 0, 255, p, None) == -1     # empty padded plane
    assert lib.haff_robot_mask(p, 4, 5, 0, 0, 0, 0, 0.0, None, 0, 0, 256, p, None) == -1       # on_value
    assert lib.haff_robot_mask(p, 0, 5, 0, 0, 0, 0, 0.0, None, 0, 0, 255, p, None) == -1
    assert lib.haff_robot_mask(p, 4, 5, 0, 0, 0, 0, 0.0, None, 0, 0, 255, p + 1, None) == -1   # misaligned output
    # heatmap: empty planes, a missing table, a workspace below n * 512 floats
    assert lib.haff_robot_heatmap(p, 0, 4, 4, p, p, 512, p, None) == -1
    assert lib.haff_robot_heatmap(p, 1, 0, 4, p, p, 512, p, None) == -1
    assert lib.haff_robot_heatmap(p, 1, 4, 4, None, p, 512, p, None) == -1
    assert lib.haff_robot_heatmap(p, 2, 4, 4, p, p, 1023, p, None) == -1
    assert lib.haff_robot_heatmap(p + 2, 1, 4, 4, p, p, 512, p, None) == -1


# ---- the file protocol, with a stub model and the CPU restatement in place of the kernels ----

class _Stub:
    def __init__(self, seg=True):
        self.device = torch.device("cpu")
        self.seg = seg
        self.calls = []
        self.outputs = None

    def evaluate(self, images_clip, images, input_ids, resize_list, original_size_list, max_new_tokens=32, tokenizer=None,
                 frames_u8=None, **kw):
        self.calls.append({"ids": input_ids.clone(), "size": original_size_list[0], "max_new_tokens": max_new_tokens,
                           "frame": frames_u8.clone()})
        H, W = original_size_list[0]
        if not self.seg:
            e = torch.zeros((0, H, W))
            return input_ids, [e], [e.clone()], [torch.zeros((0, 4))]
        g = torch.Generator().manual_seed(len(self.calls))
        left, right = torch.randn((1, H, W), generator=g) * 8, torch.randn((1, H, W), generator=g) * 8 - 2
        self.outputs = (left[0].numpy(), right[0].numpy())
        return input_ids, [left], [right], [torch.tensor([[0.1, 0.6, 0.2, 0.1]])]


def _cpu_planes(logits, th, margins, and_masks, on_value=255):
    heat = np.stack([R.heatmap(x) for x in logits.numpy()])
    masks = np.stack([R.pad_and_mask(x, th, margins, m.numpy()) for x, m in zip(logits.numpy(), and_masks)])
    return torch.from_numpy(heat), torch.from_numpy(masks)


def _request(folder, rng, H=20, W=24, margins=(2, -1, 3, 4), masks=("left", "right"), prompt="pick up the cup\nsecond line"):
    folder.mkdir(parents=True, exist_ok=True)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    Image.fromarray(img).save(folder / "img.png")
    (folder / "prompt.txt").write_text(prompt)
    (folder / "margins.txt").write_text(",".join(str(m) for m in margins))
    Ho, Wo = H + margins[1] + margins[3], W + margins[0] + margins[2]
    planes = {}
    for side in masks:
        planes[side] = rng.integers(0, 256, (Ho, Wo), dtype=np.uint8)
        Image.fromarray(planes[side]).save(folder / f"mask_{side}.png")
    return img, planes


@pytest.fixture
def stub(monkeypatch):
    from haff import config as hcfg
    from haff.checkpoint import ByteTokenizer
    cfg = hcfg.tiny()
    holder = {"model": _Stub()}
    monkeypatch.setattr(robot_demo, "build_model_and_tokenizer",
                        lambda args: (holder["model"], ByteTokenizer(cfg), cfg, torch.float32))
    monkeypatch.setattr(postprocess, "robot_planes", _cpu_planes)
    holder["tokenizer"] = ByteTokenizer(cfg)
    return holder


@pytest.mark.parametrize("force,hands", [([], ()), (["--force_left"], ("left",)), (["--force_right"], ("right",)),
                                         (["--force_both"], ("left", "right")),
                                         (["--force_left", "--force_right"], ("left", "right"))])
def test_file_protocol(stub, tmp_path, capsys, force, hands):
    from haff import prompt as hprompt
    rng = np.random.default_rng(7)
    inp, out = tmp_path / "in", tmp_path / "out"
    img, masks = _request(inp, rng)
    robot_demo.main(["--zed2_img_path", str(inp), "--vis_save_path", str(out), "--poll-interval", "0"] + force, max_requests=1)
    text = capsys.readouterr().out
    assert text.startswith("Ready\n")
    expected = {"cropped_img.png"} | {f"aff_{h}.png" for h in hands} | {f"aff_{h}_heat.png" for h in hands}
    assert set(os.listdir(out)) == expected
    assert sorted(os.listdir(inp)) == ["mask_left.png", "mask_right.png"]       # inputs deleted, masks kept
    assert np.array_equal(np.asarray(Image.open(out / "cropped_img.png")), img)
    call = stub["model"].calls[0]
    assert call["size"] == (20, 24) and call["max_new_tokens"] == 512 and torch.equal(call["frame"][0], torch.from_numpy(img))
    ids = hprompt.tokenizer_image_token(hprompt.build_inference_prompt("pick up the cup\n"), stub["tokenizer"],
                                        return_tensors="pt")
    assert torch.equal(call["ids"][0], ids)                                     # the first line, newline included
    xs = dict(zip(("left", "right"), stub["model"].outputs))
    for h in hands:
        assert f"{out / ('aff_' + h + '.png')} has been saved." in text
        assert np.array_equal(np.asarray(Image.open(out / f"aff_{h}.png")), R.pad_and_mask(xs[h], -5, (2, -1, 3, 4), masks[h]))
        heat = Image.open(out / f"aff_{h}_heat.png")
        assert heat.mode == "RGB" and np.array_equal(np.asarray(heat), R.heatmap(xs[h]))
    assert text.count("has been saved.") == len(hands)


def test_file_protocol_missing_own_mask_and_threshold(stub, tmp_path):
    rng = np.random.default_rng(8)
    inp, out = tmp_path / "in", tmp_path / "out"
    _, masks = _request(inp, rng, margins=(0, 0, 0, 0), masks=("right",))
    robot_demo.main(["--zed2_img_path", str(inp), "--vis_save_path", str(out), "--poll-interval", "0", "--force_both",
                     "--th", "0"], max_requests=1)
    xl, xr = stub["model"].outputs
    assert np.array_equal(np.asarray(Image.open(out / "aff_left.png")), R.pad_and_mask(xl, 0, (0, 0, 0, 0), None, masks["right"]))
    assert np.array_equal(np.asarray(Image.open(out / "aff_right.png")), R.pad_and_mask(xr, 0, (0, 0, 0, 0), masks["right"]))
    assert os.listdir(inp) == ["mask_right.png"]


def test_file_protocol_without_seg(stub, tmp_path, capsys):
    stub["model"] = _Stub(seg=False)
    inp, out = tmp_path / "in", tmp_path / "out"
    img, _ = _request(inp, np.random.default_rng(9))
    robot_demo.main(["--zed2_img_path", str(inp), "--vis_save_path", str(out), "--poll-interval", "0", "--force_both"],
                    max_requests=1)
    assert "No taxonomy found!!" in capsys.readouterr().out
    assert os.listdir(out) == ["cropped_img.png"]
    assert sorted(os.listdir(inp)) == ["mask_left.png", "mask_right.png"]


def test_file_protocol_without_masks(stub, tmp_path, capsys):
    inp, out = tmp_path / "in", tmp_path / "out"
    _request(inp, np.random.default_rng(10), masks=())
    robot_demo.main(["--zed2_img_path", str(inp), "--vis_save_path", str(out), "--poll-interval", "0", "--force_both"],
                    max_requests=2)
    assert capsys.readouterr().out.count("Masks not found") == 2
    assert sorted(os.listdir(inp)) == ["img.png", "margins.txt", "prompt.txt"]    # nothing deleted, nothing evaluated
    assert os.listdir(out) == [] and stub["model"].calls == []
