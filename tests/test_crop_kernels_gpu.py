"""csrc/frame_crop.hip against Pillow itself, to the byte: ops.crop_resample on frames (C = 3) and mask planes (C = 1), with and
without the mirror, on boxes that clamp at every border, pad either axis by an odd amount, scale up, scale down to the 17-tap
limit and span several tiles. Every case lies inside ops.crop_supported: nothing here takes a host route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pillow(image, box):
    """crop -> black square -> paste -> resize(BICUBIC), written for this test; image uint8 [H,W,3] or [H,W]."""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(image), "RGB" if image.ndim == 3 else "L")
    square = Image.new(im.mode, (box["S"], box["S"]))
    square.paste(im.crop((box["x0"], box["y0"], box["x0"] + box["cw"], box["y0"] + box["ch"])), (box["px"], box["py"]))
    return np.asarray(square.resize(im.size, Image.BICUBIC))


def _want(x, box, flip):
    """One sample [H,W,C] as the kernel is specified: mirror, then (with a box) the crop; C = 1 reads v != 0 as 255, writes != 0 as 1."""
    src = x[:, ::-1] if flip else x
    if x.shape[2] == 3:
        return _pillow(src, box) if box else np.ascontiguousarray(src)
    plane = (src[..., 0] != 0).astype(np.uint8)
    return ((_pillow(plane * 255, box) != 0) if box else plane).astype(np.uint8)[..., None]


def _box(x0, y0, cw, ch):
    S = max(cw, ch)
    return {"x0": x0, "y0": y0, "cw": cw, "ch": ch, "px": (S - cw) // 2, "py": (S - ch) // 2, "S": S}


def _blob(cx, cy, r, n, k):
    t = 2 * np.pi * np.arange(n) / n
    rad = r * (1 + 0.25 * np.sin(k * t))
    return np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], 1).astype(np.int32).tolist()


# name -> (H, W), obj_left, obj_right: the box is aff_dataset.crop_box's (margin 50), of the mirrored planes for the mirrored runs
CONTOUR_CASES = {
    "37x53 top-left corner": ((37, 53), [[[0, 0], [1, 0], [0, 1]]], []),                       # x0 = y0 = 0 by the clamp; cw = 51
    "37x53 bottom-right corner": ((37, 53), [], [[[52, 36], [51, 36], [52, 35]]]),             # x1 = W, y1 = H by the clamp; cw = 52
    "37x53 one pixel": ((37, 53), [[[20, 11]]], []),
    "64x80 cw < ch, odd S - cw": ((64, 80), [[[0, 0], [5, 0], [5, 63], [0, 63]]], []),         # 55 x 64
    "64x80 cw > ch, odd S - ch": ((64, 80), [[[0, 0], [10, 0], [10, 3], [0, 3]]], []),         # 60 x 53
    "64x80 full width": ((64, 80), [[[0, 20], [79, 20], [79, 24], [0, 24]]], []),              # S = W: identity across, 7 taps down
    "130x67 portrait": ((130, 67), [[[5, 100], [60, 110], [30, 129]]], []),                    # 67 x 80
    "256x456 both hands": ((256, 456), [_blob(150, 120, 30, 24, 3)], [_blob(300, 140, 25, 18, 4)]),
}
# name -> (H, W), the box as given (of the mirrored sample for the mirrored runs): what the 50 px margin cannot reach on small planes
BOX_CASES = {
    "64x80 threefold up-scale": ((64, 80), _box(10, 5, 21, 30)),
    "64x80 tiny box at the right border": ((64, 80), _box(59, 0, 21, 13)),
    "64x80 one source pixel": ((64, 80), _box(33, 17, 1, 1)),
    "24x96 fourfold down-scale, 17 taps": ((24, 96), _box(0, 3, 96, 20)),
    "70x300 several tiles, odd paddings": ((70, 300), _box(7, 2, 280, 67)),
}


def _case(name, flip):
    from haff import aff_dataset
    if name in BOX_CASES:
        return BOX_CASES[name]
    hw, left, right = CONTOUR_CASES[name]
    return hw, aff_dataset.crop_box(left, right, hw, flip=flip)


def test_the_named_cases_are_what_their_names_say():
    from haff import aff_dataset, ops
    geo = {n: aff_dataset.crop_box(c[1], c[2], c[0]) for n, c in CONTOUR_CASES.items()}
    b = geo["37x53 top-left corner"]
    assert (b["x0"], b["y0"], b["cw"], b["ch"]) == (0, 0, 51, 37)
    b = geo["37x53 bottom-right corner"]
    assert (b["x0"] + b["cw"], b["y0"] + b["ch"], b["x0"]) == (53, 37, 1)
    b = geo["64x80 cw < ch, odd S - cw"]
    assert b["cw"] < b["ch"] and (b["S"] - b["cw"]) % 2 == 1
    b = geo["64x80 cw > ch, odd S - ch"]
    assert b["cw"] > b["ch"] and (b["S"] - b["ch"]) % 2 == 1 and b["cw"] < 80
    b = geo["64x80 full width"]
    assert b["S"] == b["cw"] == 80 and ops.crop_table(80, 64).shape[1] - 2 == 7
    b = geo["130x67 portrait"]
    assert (b["cw"], b["ch"]) == (67, 80)
    b = geo["256x456 both hands"]
    assert b["cw"] > 250 and b["x0"] > 0 and b["x0"] + b["cw"] < 456 and b["y0"] > 0
    assert ops.crop_table(96, 24).shape[1] - 2 == 17
    for name in list(CONTOUR_CASES) + list(BOX_CASES):          # no case falls to the host route
        for flip in (False, True):
            hw, box = _case(name, flip)
            assert box is not None and ops.crop_supported(hw, box["S"]), name


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("name", list(CONTOUR_CASES) + list(BOX_CASES))
def test_crop_equals_pillow(dev, name, C, flip):
    from haff import ops
    (H, W), box = _case(name, flip)
    assert ops.crop_supported((H, W), box["S"])
    rng = np.random.default_rng(len(name) + 2 * C + flip)
    x = rng.integers(0, 256, (1, H, W, C), dtype=np.uint8)
    if C == 1:                                                  # a mask with holes and fragments; any non-zero byte counts
        x = np.where(rng.random((1, H, W, 1)) < 0.55, 0, x).astype(np.uint8)
    src = torch.from_numpy(x).to(dev)
    got = ops.crop_resample(src, [box], [flip])
    assert got.shape == src.shape and got.dtype == torch.uint8 and got.data_ptr() != src.data_ptr()
    assert torch.equal(src.cpu(), torch.from_numpy(x))           # out of place
    want = _want(x[0], box, flip)
    got = got.cpu().numpy()[0]
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} bytes differ"
    assert not np.array_equal(want, _want(x[0], None, flip))
    if C == 1:
        assert set(np.unique(got)) <= {0, 1}


def test_one_launch_mixes_cropped_mirrored_and_copied_samples(dev):
    from haff import ops
    H, W = 64, 80
    boxes = [_box(10, 5, 21, 30), _box(3, 0, 70, 64), None]
    flips = [False, True, False]
    rng = np.random.default_rng(9)
    for C in (3, 1):
        x = rng.integers(0, 256, (3, H, W, C), dtype=np.uint8)
        if C == 1:
            x = np.where(rng.random(x.shape) < 0.5, 0, x).astype(np.uint8)
        got = ops.crop_resample(torch.from_numpy(x).to(dev), boxes, flips).cpu().numpy()
        for b in range(3):
            assert np.array_equal(got[b], _want(x[b], boxes[b], flips[b])), (C, b)
    # a sample without a box is still mirrored where it drew the flip
    got = ops.crop_resample(torch.from_numpy(x).to(dev), [None, boxes[0], None], [True, False, False]).cpu().numpy()
    assert np.array_equal(got[0], _want(x[0], None, True)) and np.array_equal(got[2], _want(x[2], None, False))
    assert np.array_equal(got[1], _want(x[1], boxes[0], False))


def test_both_hands_planes_share_one_launch_as_the_ingest_calls_it(dev):
    """uint8 [2 B, H, W] filled planes viewed as [2 B, H, W, 1], each sample's box and flip given twice."""
    from haff import ops
    H, W = 130, 67
    box = _box(0, 50, 67, 80)
    planes = (np.random.default_rng(4).random((4, H, W)) < 0.3).astype(np.uint8)
    got = ops.crop_resample(torch.from_numpy(planes).to(dev)[..., None], [box, box, None, None], [True, True, False, False])[..., 0]
    assert got.is_contiguous() and got.shape == (4, H, W)
    for p in range(4):
        assert np.array_equal(got[p].cpu().numpy(), _want(planes[p][..., None], box if p < 2 else None, p < 2)[..., 0]), p


def test_over_limit_geometry_is_refused_on_the_host_without_a_launch(dev):
    from haff import ops
    from haff.lib import HaffLibraryError
    H, W = 15, 64                                               # S = 64 > 4 H: more than 17 taps down
    box = _box(0, 0, 64, 15)
    assert not ops.crop_supported((H, W), box["S"]) and ops.crop_supported((16, W), 64)
    src = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev)
    out = torch.full_like(src, 77)
    with pytest.raises(HaffLibraryError, match="-2"):
        ops.crop_resample(src, [box], [False], out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())                              # nothing ran
    assert not ops.crop_supported((4097, 4096), 100)            # the pixel limit of the other augmentation kernels
    bad = dict(box, x0=1)                                       # a box past the right border: a bad argument, not a host-route case
    with pytest.raises(HaffLibraryError, match="-1"):
        ops.crop_resample(torch.zeros((1, 16, W, 3), dtype=torch.uint8, device=dev), [dict(bad, ch=16, S=64, py=24)], [False], out=None)
