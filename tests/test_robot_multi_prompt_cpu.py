"""robot_demo.py --multi_prompt, host side: the file protocol with a stub model and the CPU restatement (tests/robot_ref.py) in place of
the kernels. Every non-empty line of prompt.txt is one row of ONE evaluate(offset=[0, n]) call; line 0 writes the usual file names,
line i >= 1 the same set with _<i> in front of the extension; without the flag nothing changes. Nothing here computes on a GPU."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from haff import postprocess, robot_demo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/robot_ref.py
import robot_ref as R   # noqa: E402

MARGINS = (2, -1, 3, 4)


class _Stub:
    """evaluate() of a model that finds [SEG] in every row but `no_seg`: random planes per row, remembered for the comparison"""

    def __init__(self, no_seg=()):
        self.device = torch.device("cpu")
        self.calls, self.left, self.right, self.no_seg = [], [], [], set(no_seg)

    def evaluate(self, images_clip, images, input_ids, resize_list, original_size_list, max_new_tokens=32, tokenizer=None,
                 frames_u8=None, attention_mask=None, offset=None):
        self.calls.append({"ids": input_ids.clone(), "mask": attention_mask, "offset": offset, "frames": len(frames_u8),
                           "sizes": (list(resize_list), list(original_size_list))})
        H, W = original_size_list[0]
        g = torch.Generator().manual_seed(3)
        tax = []
        for b in range(input_ids.shape[0]):
            n = 0 if b in self.no_seg else 1
            self.left.append(torch.randn((n, H, W), generator=g) * 8)
            self.right.append(torch.randn((n, H, W), generator=g) * 8 - 2)
            tax.append(torch.full((n, 4), 0.25))
        return input_ids, self.left, self.right, tax


@pytest.fixture
def stub(monkeypatch):
    from haff import config as hcfg
    from haff.checkpoint import ByteTokenizer
    cfg = hcfg.tiny()
    holder = {"model": _Stub(), "tokenizer": ByteTokenizer(cfg), "cfg": cfg}
    monkeypatch.setattr(robot_demo, "build_model_and_tokenizer", lambda args: (holder["model"], holder["tokenizer"], cfg, torch.float32))
    monkeypatch.setattr(postprocess, "robot_planes", lambda logits, th, margins, and_masks: (
        torch.from_numpy(np.stack([R.heatmap(x) for x in logits.numpy()])),
        torch.from_numpy(np.stack([R.pad_and_mask(x, th, margins, m.numpy()) for x, m in zip(logits.numpy(), and_masks)]))))
    return holder


def _request(folder, prompt, H=20, W=24):
    rng = np.random.default_rng(7)
    folder.mkdir(parents=True, exist_ok=True)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    Image.fromarray(img).save(folder / "img.png")
    (folder / "prompt.txt").write_text(prompt)
    (folder / "margins.txt").write_text(",".join(str(m) for m in MARGINS))
    Ho, Wo = H + MARGINS[1] + MARGINS[3], W + MARGINS[0] + MARGINS[2]
    masks = {}
    for side in ("left", "right"):
        masks[side] = rng.integers(0, 256, (Ho, Wo), dtype=np.uint8)
        Image.fromarray(masks[side]).save(folder / f"mask_{side}.png")
    return img, masks


def _main(inp, out, *flags):
    robot_demo.main(["--zed2_img_path", str(inp), "--vis_save_path", str(out), "--poll-interval", "0", "--force_both", *flags],
                    max_requests=1)


def test_every_line_is_a_row_of_one_grouped_call(stub, tmp_path):
    from haff import prompt as hprompt
    inp, out = tmp_path / "in", tmp_path / "out"
    lines = ["pick up the cup", "open the drawer slowly", "cut"]
    img, masks = _request(inp, lines[0] + "\n\n" + lines[1] + "\n   \n" + lines[2])       # empty lines skipped, no newline at the end
    _main(inp, out, "--multi_prompt")
    model, cfg = stub["model"], stub["cfg"]
    assert len(model.calls) == 1
    call = model.calls[0]
    assert call["frames"] == 1 and len(call["sizes"][0]) == 1 and call["sizes"][1] == [(20, 24)]   # ONE frame, three rows
    assert call["offset"].dtype == torch.int64 and call["offset"].tolist() == [0, 3]
    rows = [hprompt.tokenizer_image_token(hprompt.build_inference_prompt(t), stub["tokenizer"], return_tensors="pt")
            for t in (lines[0] + "\n", lines[1] + "\n", lines[2])]                       # each line as the file holds it
    assert call["ids"].shape == (3, max(r.numel() for r in rows))
    for b, r in enumerate(rows):
        assert torch.equal(call["ids"][b, :r.numel()], r) and bool((call["ids"][b, r.numel():] == cfg.pad_token_id).all())
        assert call["mask"][b].tolist() == [True] * r.numel() + [False] * (call["ids"].shape[1] - r.numel())
    names = [f"{n}{s}.png" for s in ("", "_1", "_2") for n in ("aff_left", "aff_left_heat", "aff_right", "aff_right_heat", "cropped_img")]
    assert sorted(os.listdir(out)) == sorted(names)
    for i, s in enumerate(("", "_1", "_2")):
        for side, planes in (("left", model.left), ("right", model.right)):
            x = planes[i][0].numpy()
            assert np.array_equal(np.asarray(Image.open(out / f"aff_{side}{s}.png")), R.pad_and_mask(x, -5, MARGINS, masks[side]))
            assert np.array_equal(np.asarray(Image.open(out / f"aff_{side}_heat{s}.png")), R.heatmap(x))
        assert np.array_equal(np.asarray(Image.open(out / f"cropped_img{s}.png")), img)
    assert sorted(os.listdir(inp)) == ["mask_left.png", "mask_right.png"]


def test_a_line_without_seg_writes_only_its_frame(stub, tmp_path, capsys):
    stub["model"] = _Stub(no_seg=(1,))
    inp, out = tmp_path / "in", tmp_path / "out"
    _request(inp, "pick up the cup\nopen the drawer\n")
    _main(inp, out, "--multi_prompt")
    assert capsys.readouterr().out.count("No taxonomy found!!") == 1
    assert sorted(os.listdir(out)) == sorted(["aff_left.png", "aff_left_heat.png", "aff_right.png", "aff_right_heat.png",
                                              "cropped_img.png", "cropped_img_1.png"])


def test_one_line_with_the_flag_and_many_lines_without_it_are_the_plain_call(stub, tmp_path):
    for name, prompt, flags in (("a", "pick up the cup\n", ("--multi_prompt",)), ("b", "pick up the cup\nopen the drawer\n", ())):
        stub["model"] = _Stub()
        inp, out = tmp_path / (name + "_in"), tmp_path / (name + "_out")
        _request(inp, prompt)
        _main(inp, out, *flags)
        call = stub["model"].calls[0]
        assert call["ids"].shape[0] == 1 and call["offset"] is None and call["mask"] is None
        assert sorted(os.listdir(out)) == ["aff_left.png", "aff_left_heat.png", "aff_right.png", "aff_right_heat.png", "cropped_img.png"]


def test_the_flag_is_not_one_of_parse_args():
    """parse_args keeps the reference's flags plus the offline extras; --multi_prompt belongs to main()"""
    with pytest.raises(SystemExit):
        robot_demo.parse_args(["--multi_prompt"])
    assert robot_demo.MULTI_PROMPT_FLAG == "--multi_prompt"
