"""The object-crop augmentation (--aug_crop), the parts that need no GPU: the flag and its refusals, draw_crop, the box, the host route
of AffRecordsDataset (Pillow, the yardstick of the device route), the vectorised table builder and the C-ABI wiring of
csrc/frame_crop.hip."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import haff
from haff import aff_dataset, config as hcfg, cvlite, ops, preprocess, train_ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C-ABI wiring ----------------------------------------------------------------------------------------------------------
def test_crop_symbol_is_declared_exported_and_typed():
    from haff import lib as hlib
    name = "haff_crop_resample_u8"
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    m = re.search(r"^int %s\(([^;]*)\);" % name, text, flags=re.M | re.S)
    assert m, f"include/haff_hip.h does not declare {name}"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    proto = hlib._PROTOS[name]
    assert len(proto) == len(params) == 10
    for p, t in zip(params, proto):
        assert t is (hlib.c_void_p if "*" in p else hlib.c_long if p.startswith("long ") else hlib.c_int), (p, t)
    assert getattr(haff.load_library(), name).argtypes == proto
    assert "frame_crop.hip" in open(os.path.join(ROOT, "2handedafforder_amd", "csrc", "Makefile")).read()


def _box(x0, y0, cw, ch):
    S = max(cw, ch)
    return {"x0": x0, "y0": y0, "cw": cw, "ch": ch, "px": (S - cw) // 2, "py": (S - ch) // 2, "S": S}


def test_entry_point_refuses_bad_geometry_on_the_host():
    """Nothing is launched for these: the image pointers are never dereferenced, the descriptor is read on the host only."""
    lib = haff.load_library()
    P = ctypes.c_void_p
    IN, OUT = 0x100000, 0x900000
    H, W = 40, 64

    def call(desc, src=IN, dst=OUT, B=1, H=H, W=W, C=3, words=None, dev=0x4000):
        return int(lib.haff_crop_resample_u8(P(src), P(dst), B, H, W, C, P(desc.data_ptr()), P(dev), desc.numel() if words is None else words,
                                             None))
    good = ops.crop_descriptor([_box(3, 2, 30, 21)], [True], (H, W))

    def broken(word, value):
        d = good.clone()
        d[word] = value
        return d
    assert call(good, B=0) == -1 and call(good, H=0) == -1 and call(good, C=2) == -1 and call(good, src=0) == -1 and call(good, dev=0) == -1
    assert call(good, dst=IN) == -1 and call(good, dst=IN + H * W * 3 - 1) == -1           # out == in, overlap
    assert call(good, words=11) == -1 and call(good, words=good.numel() - 1) == -1         # a table past the end of the descriptor
    assert call(good, H=4097, W=4096) == -2
    assert call(broken(0, -1)) == -1 and call(broken(0, W - 29)) == -1 and call(broken(1, H - 20)) == -1       # a box outside the sample
    assert call(broken(2, 0)) == -1 and call(broken(3, H + 1)) == -1
    assert call(broken(6, 31)) == -1 and call(broken(4, 1)) == -1 and call(broken(5, 10)) == -1               # S, the paste
    assert call(broken(7, 4 | 2)) == -1                                                    # an unknown flag bit
    assert call(broken(9, 18)) == -1 and call(broken(8, -1)) == -1 and call(broken(11, 0)) == -1
    first_row = int(good[8])
    assert call(broken(first_row, -1)) == -1 and call(broken(first_row + 1, 6)) == -1      # a table row outside [0, S)
    last_row = int(good[8]) + (W - 1) * (2 + int(good[9]))
    assert call(broken(last_row, 30)) == -1
    # beyond the limits: more than a 4-fold down-scale (cw = 64 on W = 64 is the most a sample can give, so H shrinks instead)
    H2 = 15
    over = ops.crop_descriptor([_box(0, 0, 64, 15)], [False], (H2, W))
    assert not ops.crop_supported((H2, W), 64) and ops.crop_supported((16, W), 64)
    assert call(over, H=H2) == -2
    with pytest.raises(haff.lib.HaffLibraryError, match="-2"):      # ops.crop_resample: refused before anything is enqueued
        haff.lib.check(call(over, H=H2), "haff_crop_resample_u8")


# ---- the flag --------------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device before refusing the flag")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)


def test_flag_defaults_to_off_and_is_refused_with_synthetic_and_outside_the_unit_interval(monkeypatch):
    assert train_ds.parse_args([]).aug_crop == 0.0
    assert train_ds.parse_args(["--aug_crop", "0.6667"]).aug_crop == 0.6667
    _no_device(monkeypatch)
    with pytest.raises(SystemExit) as e:
        train_ds.main(["--aug_crop", "0.5", "--synthetic", "tiny"])
    assert "--aug_crop" in str(e.value) and "--synthetic" in str(e.value)
    for value in ("1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit) as e:
            train_ds.main(["--aug_crop", value, "--sam_records", "unused.pt"])
        assert "--aug_crop" in str(e.value) and "[0, 1]" in str(e.value)
        with pytest.raises(ValueError, match="aug_crop"):
            aff_dataset.AffRecordsDataset(_records(1), hcfg.tiny(), seed=0, aug_crop=float(value))


# ---- the draw --------------------------------------------------------------------------------------------------------------
def test_draw_crop_is_a_pure_function_of_seed_and_index():
    first = [aff_dataset.draw_crop(7, i, 0.6667) for i in range(60)]
    again = [aff_dataset.draw_crop(7, i, 0.6667) for i in reversed(range(60))][::-1]
    assert first == again and all(isinstance(v, bool) for v in first)
    assert [aff_dataset.draw_crop(1007, i, 0.6667) for i in range(60)] != first
    assert not any(aff_dataset.draw_crop(7, i, 0.0) for i in range(60)) and all(aff_dataset.draw_crop(7, i, 1.0) for i in range(60))
    # a generator of its own: not the flip's uniform, not the jitter's
    import random
    flips = [random.Random(f"haff-aug/7/{i}").random() < 0.6667 for i in range(60)]
    assert first != flips


def test_draw_crop_frequency_over_4000_samples():
    """Binomial(4000, 2/3): mean 2667, sigma 30; five sigma either way."""
    hits = sum(aff_dataset.draw_crop(7, i, 0.6667) for i in range(4000))
    print(f"crops {hits}")
    assert 2517 <= hits <= 2817


def test_ambiguous_narrations_are_always_cropped_when_the_crop_is_on():
    missed = [i for i in range(200) if not aff_dataset.draw_crop(3, i, 0.01)]
    assert len(missed) > 150
    for i in missed[:40]:
        assert aff_dataset.draw_crop(3, i, 0.01, "pick up something") and aff_dataset.draw_crop(3, i, 0.01, "move the things away")
        assert not aff_dataset.draw_crop(3, i, 0.01, "pick up the cup")
        assert not aff_dataset.draw_crop(3, i, 0.0, "pick up something")          # off is off


# ---- the dataset -----------------------------------------------------------------------------------------------------------
def _records(n=5, hw=(48, 64), seed=0, objects=True):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        x, y = 4 + 3 * i, 5 + 2 * i
        masks = {"aff_left": [[[x, y], [x + 20, y + 2], [x + 12, y + 18]]],
                 "aff_right": [] if i % 2 else [[[30, 10], [50, 12], [45, 30], [28, 28]]], "original_size": hw}
        if objects:
            masks["obj_left"] = [[[x, y], [x + 22, y + 1], [x + 14, y + 20], [x + 2, y + 15]]]
            masks["obj_right"] = [] if i % 2 else [[[28, 8], [52, 10], [47, 33], [26, 30]]]
        recs.append({"narration": f"Action Number {i} with the tool", "inpainted": rng.integers(0, 255, hw + (3,), dtype=np.uint8),
                     "taxonomy": [[1, 0, 0, 0], 0, [0, 0, 1, 0], 1, [0, 1, 0, 0]][i % 5], "masks": masks})
    return recs


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_zero_probability_changes_nothing(monkeypatch):
    def no_draw(*a, **k):
        raise AssertionError("draw_crop called with aug_crop 0")
    monkeypatch.setattr(aff_dataset, "draw_crop", no_draw)
    cfg = hcfg.tiny()
    for kw in ({}, {"aug_flip": 0.5, "aug_jitter": 0.25}):
        plain = [aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, **kw) for _ in range(2)]
        zero = [aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, aug_crop=0.0, **kw) for _ in range(2)]
        for i in range(12):
            assert _same(plain[0][i], zero[0][i]), i
            a, b = plain[1].raw_item(i), zero[1].raw_item(i)
            assert "crop" not in b and "crop_skipped" not in b and _same(a, b), i
        assert plain[0].rng.getstate() == zero[0].rng.getstate()


def test_the_crop_leaves_the_flip_and_jitter_draws_and_the_sample_sequence_alone():
    cfg = hcfg.tiny()
    two = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, aug_flip=0.5, aug_jitter=0.25)
    three = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, aug_flip=0.5, aug_jitter=0.25, aug_crop=0.6667)
    host = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, aug_flip=0.5, aug_jitter=0.25, aug_crop=0.6667)
    cropped = 0
    for i in range(20):
        a, b, h = two.raw_item(i), three.raw_item(i), host[i]
        assert b["aug"] == a["aug"] == aff_dataset.draw_augmentation(11, i, 0.5, 0.25)
        assert list(b) == list(a) + ["crop"] and _same({k: b[k] for k in a}, a)
        assert (b["crop"] is not None) == aff_dataset.draw_crop(11, i, 0.6667)
        assert h[3] == b["conversations"] and h[9] == b["questions"]
        cropped += b["crop"] is not None
    assert two.rng.getstate() == three.rng.getstate() == host.rng.getstate() and 8 <= cropped < 20
    assert three.crop_skipped == 0 and host.crop_skipped == 0


# ---- the box ---------------------------------------------------------------------------------------------------------------
def _filled_box(obj_left, obj_right, hw, flip):
    """The issue's definition, from the rasters: the extremes of fill(obj_left) | fill(obj_right), mirrored first for a flip."""
    H, W = hw
    union = cvlite.draw_contours_filled(hw, obj_left) | cvlite.draw_contours_filled(hw, obj_right)
    if flip:
        union = union[:, ::-1]
    ys, xs = np.nonzero(union)
    x0, y0 = max(int(xs.min()) - 50, 0), max(int(ys.min()) - 50, 0)
    x1, y1 = min(int(xs.max()) + 50, W), min(int(ys.max()) + 50, H)
    return _box(x0, y0, x1 - x0, y1 - y0)


BOX_FIXTURES = {
    "one hand": ((200, 300), [[[120, 80], [160, 85], [150, 130], [118, 120]]], []),
    "two hands": ((200, 300), [[[60, 70], [90, 75], [70, 100]]], [[[200, 90], [240, 60], [250, 140], [210, 120]]]),
    "two contours of one hand": ((200, 300), [[[60, 70], [90, 75], [70, 100]], [[100, 120], [110, 121], [104, 140]]], []),
    "one pixel": ((200, 300), [[[77, 131]]], []),
    "touching the left border": ((200, 300), [[[0, 90], [30, 95], [10, 120]]], []),
    "touching the top border": ((200, 300), [[[100, 0], [140, 4], [120, 30]]], []),
    "touching the right border": ((200, 300), [], [[[299, 60], [270, 70], [290, 100]]]),
    "touching the bottom border": ((200, 300), [], [[[100, 199], [140, 180], [150, 199]]]),
    "a vertex outside the plane": ((200, 300), [[[-40, 90], [60, 60], [60, 130]]], [[[250, 150], [330, 150], [330, 230], [250, 230]]]),
}


@pytest.mark.parametrize("name", sorted(BOX_FIXTURES))
@pytest.mark.parametrize("flip", [False, True])
def test_box_from_vertex_extremes_equals_the_box_of_the_filled_union(name, flip):
    hw, left, right = BOX_FIXTURES[name]
    box = aff_dataset.crop_box(left, right, hw, flip=flip)
    assert box == _filled_box(left, right, hw, flip), name
    assert box["S"] == max(box["cw"], box["ch"]) and 0 <= box["px"] <= box["S"] - box["cw"] and 0 <= box["py"] <= box["S"] - box["ch"]
    if name == "one pixel":
        assert (box["cw"], box["ch"]) == (100, 100)        # 50 before, the pixel, 49 after: x1 is exclusive, max_x inclusive
    if name == "one pixel" and flip:
        assert box["x0"] == 300 - 1 - 77 - 50


def test_no_object_gives_no_box():
    assert aff_dataset.crop_box([], [], (48, 64)) is None and aff_dataset.crop_box(None, [[]], (48, 64)) is None
    assert aff_dataset.crop_box([[[-9, -9], [-3, -9], [-5, -2]]], [], (48, 64)) is None      # wholly outside the plane


# ---- the host route --------------------------------------------------------------------------------------------------------
def _pillow_crop(image, bbox, mode):
    """process_cropped_sequences.py's crop_and_pad in a few lines of Pillow, written for this test (offset 50, BICUBIC)."""
    from PIL import Image
    im = Image.fromarray(image, mode)
    w, h = im.size
    min_x, min_y, max_x, max_y = bbox
    cut = im.crop((max(min_x - 50, 0), max(min_y - 50, 0), min(max_x + 50, w), min(max_y + 50, h)))
    side = max(cut.size)
    square = Image.new(mode, (side, side))
    square.paste(cut, ((side - cut.size[0]) // 2, (side - cut.size[1]) // 2))
    return np.asarray(square.resize((w, h), Image.BICUBIC))


def _bbox(*planes):
    ys, xs = np.nonzero(np.maximum.reduce(planes))
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def _wide_record(hw=(150, 260), seed=3):
    """An object well inside a plane larger than the 50 px margin, with odd S - cw."""
    rng = np.random.default_rng(seed)
    return {"narration": "cut the bread", "inpainted": rng.integers(0, 255, hw + (3,), dtype=np.uint8), "taxonomy": [1, 0, 0, 0],
            "masks": {"original_size": hw, "aff_left": [[[70, 60], [84, 62], [80, 80]]], "aff_right": [[[88, 70], [97, 71], [90, 85]]],
                      "obj_left": [[[66, 40], [86, 44], [82, 84], [68, 80]]], "obj_right": [[[85, 66], [99, 70], [92, 100]]]}}


@pytest.mark.parametrize("flip,jitter", [(False, None), (True, None), (False, (0.7, 1.3, 0.55)), (True, (1.45, 0.6, 1.2))])
def test_host_route_is_flip_then_crop_then_jitter_with_pillow(monkeypatch, flip, jitter):
    from PIL import Image
    cfg = hcfg.tiny()
    if jitter is not None:
        jitter = tuple(float(np.float32(v)) for v in jitter)
    monkeypatch.setattr(aff_dataset, "draw_augmentation", lambda seed, idx, pf, pj: {"flip": flip, "jitter": jitter})
    rec = _wide_record()
    hw, m = rec["masks"]["original_size"], rec["masks"]
    fills = {k: cvlite.draw_contours_filled(hw, m[k]) for k in ("aff_left", "aff_right", "obj_left", "obj_right")}
    frame = rec["inpainted"]
    tax = [1.0, 0.0, 0.0, 0.0]
    if flip:
        frame = np.asarray(Image.fromarray(frame).transpose(Image.FLIP_LEFT_RIGHT))
        fills = {"aff_left": fills["aff_right"][:, ::-1], "aff_right": fills["aff_left"][:, ::-1],
                 "obj_left": fills["obj_right"][:, ::-1], "obj_right": fills["obj_left"][:, ::-1]}
        tax = [0.0, 1.0, 0.0, 0.0]
    bbox = _bbox(fills["obj_left"], fills["obj_right"])
    want_frame = _pillow_crop(np.ascontiguousarray(frame), bbox, "RGB")
    want_left = (_pillow_crop(np.ascontiguousarray(fills["aff_left"]) * 255, bbox, "L") != 0).astype(np.uint8)
    want_right = (_pillow_crop(np.ascontiguousarray(fills["aff_right"]) * 255, bbox, "L") != 0).astype(np.uint8)
    if jitter is not None:
        want_frame = aff_dataset.augment_frame(want_frame, {"flip": False, "jitter": jitter})
    item = aff_dataset.AffRecordsDataset([rec], cfg, seed=2, aug_flip=0.5, aug_crop=1.0)[0]
    ref = aff_dataset.AffRecordsDataset([dict(rec, inpainted=want_frame)], cfg, seed=2)[0]
    assert torch.equal(item[1], ref[1]) and torch.equal(item[2], ref[2])          # SAM input and CLIP pixels of the cropped frame
    assert np.array_equal(item[4][0].numpy(), want_left) and np.array_equal(item[5][0].numpy(), want_right)
    assert want_left.sum() > fills["aff_left"].sum() and want_right.sum() > fills["aff_right"].sum()      # a closer view
    assert torch.equal(item[7]["left"], torch.from_numpy((want_left == 0).astype(np.int64) * 255))
    assert item[6] == tax
    plain = aff_dataset.AffRecordsDataset([rec], cfg, seed=2)[0]
    assert item[3] == plain[3] and not torch.equal(item[1], plain[1])
    # raw_item hands the record over as it is, with the box of the (mirrored) object planes
    raw = aff_dataset.AffRecordsDataset([rec], cfg, seed=2, aug_flip=0.5, aug_crop=1.0).raw_item(0)
    x0, y0 = max(bbox[0] - 50, 0), max(bbox[1] - 50, 0)
    assert raw["crop"] == _box(x0, y0, min(bbox[2] + 50, hw[1]) - x0, min(bbox[3] + 50, hw[0]) - y0)
    assert np.array_equal(raw["frame"], rec["inpainted"]) and raw["taxonomy"] == plain[6]


def test_the_mirror_of_a_crop_is_not_the_crop_of_the_mirror_and_the_loader_mirrors_first(monkeypatch):
    cfg = hcfg.tiny()
    rec = _wide_record()
    hw = rec["masks"]["original_size"]
    box = aff_dataset.crop_box(rec["masks"]["obj_left"], rec["masks"]["obj_right"], hw)
    flipped_box = aff_dataset.crop_box(rec["masks"]["obj_left"], rec["masks"]["obj_right"], hw, flip=True)
    assert (box["S"] - box["cw"]) % 2 == 1 and flipped_box["x0"] == hw[1] - (box["x0"] + box["cw"]) - 1    # inclusive max, exclusive x1
    mirrored = np.ascontiguousarray(rec["inpainted"][:, ::-1])
    flip_crop = aff_dataset.crop_image(mirrored, flipped_box)
    crop_flip = np.ascontiguousarray(aff_dataset.crop_image(rec["inpainted"], box)[:, ::-1])
    assert not np.array_equal(flip_crop, crop_flip)
    monkeypatch.setattr(aff_dataset, "draw_augmentation", lambda seed, idx, pf, pj: {"flip": True, "jitter": None})
    item = aff_dataset.AffRecordsDataset([rec], cfg, seed=2, aug_flip=1.0, aug_crop=1.0)[0]
    first = aff_dataset.AffRecordsDataset([dict(rec, inpainted=flip_crop)], cfg, seed=2)[0]
    second = aff_dataset.AffRecordsDataset([dict(rec, inpainted=crop_flip)], cfg, seed=2)[0]
    assert torch.equal(item[1], first[1]) and not torch.equal(item[1], second[1])


def test_a_frame_of_another_size_is_brought_to_the_planes_size_first():
    from PIL import Image
    cfg = hcfg.tiny()
    rec = _wide_record()
    small = dict(rec, inpainted=np.random.default_rng(5).integers(0, 255, (80, 130, 3), dtype=np.uint8))
    hw = rec["masks"]["original_size"]
    resized = np.asarray(Image.fromarray(small["inpainted"]).resize((hw[1], hw[0]), Image.BICUBIC))
    item = aff_dataset.AffRecordsDataset([small], cfg, seed=2, aug_crop=1.0)[0]
    ref = aff_dataset.AffRecordsDataset([dict(rec, inpainted=resized)], cfg, seed=2, aug_crop=1.0)[0]
    assert torch.equal(item[1], ref[1]) and torch.equal(item[2], ref[2]) and torch.equal(item[4], ref[4])
    plain = aff_dataset.AffRecordsDataset([small], cfg, seed=2)[0]
    assert item[8] != plain[8]                                   # the cropped frame has the planes' size, and the resize list says so


def test_a_sample_without_object_contours_is_not_cropped_and_is_counted():
    cfg = hcfg.tiny()
    recs = _records(3, objects=False)
    plain = aff_dataset.AffRecordsDataset(recs, cfg, seed=4)
    ds = aff_dataset.AffRecordsDataset(recs, cfg, seed=4, aug_crop=1.0)
    raw = aff_dataset.AffRecordsDataset(recs, cfg, seed=4, aug_crop=1.0)
    for i in range(4):
        assert _same(ds[i], plain[i])
        r = raw.raw_item(i)
        assert r["crop"] is None and r["crop_skipped"] is True
    assert ds.crop_skipped == 4 and raw.crop_skipped == 4


def test_from_local_keeps_the_object_contours(tmp_path):
    recs = _records(3)
    (tmp_path / "h5").mkdir()
    (tmp_path / "jsons").mkdir()
    (tmp_path / "h5" / "0-2_a.h5").write_bytes(b"")
    keys = ("aff_left", "aff_right", "obj_left", "obj_right")
    json.dump({str(i): dict({"original_size": [48, 64]}, **{k: r["masks"][k] for k in keys}) for i, r in enumerate(recs)},
              open(tmp_path / "jsons" / "0-2_a.json", "w"))
    data = {"data": {"inpainted": np.stack([r["inpainted"] for r in recs]), "narration": [r["narration"].encode() for r in recs],
                     "taxonomy": [2, 0, 1]}}
    kw = dict(h5_open=lambda path: data, seed=5)
    plain = aff_dataset.AffRecordsDataset.from_local(str(tmp_path), hcfg.tiny(), **kw)
    ds = aff_dataset.AffRecordsDataset.from_local(str(tmp_path), hcfg.tiny(), aug_crop=1.0, **kw)
    assert plain.aug_crop == 0.0 and (ds.aug_crop, ds.aug_seed) == (1.0, 5)
    for i in range(3):
        assert sorted(plain.records[i]["masks"]) == ["aff_left", "aff_right", "original_size"]      # no new key without the crop
        assert ds.records[i]["masks"]["obj_left"] == recs[i]["masks"]["obj_left"]
        assert ds.records[i]["masks"]["obj_right"] == recs[i]["masks"]["obj_right"]
    assert "crop" not in plain.raw_item(0)
    raw = ds.raw_item(0)
    rec = recs[aff_dataset.AffRecordsDataset(recs, hcfg.tiny(), seed=5).rng.randint(0, 2)]
    assert raw["crop"] == aff_dataset.crop_box(rec["masks"]["obj_left"], rec["masks"]["obj_right"], (48, 64))
    local = aff_dataset.AffRecordsDataset.from_local(str(tmp_path), hcfg.tiny(), aug_crop=1.0, **kw)[0]
    in_memory = aff_dataset.AffRecordsDataset(recs, hcfg.tiny(), seed=5, aug_crop=1.0)[0]
    uncropped = aff_dataset.AffRecordsDataset(recs, hcfg.tiny(), seed=5)[0]
    for k in (1, 2, 4, 5):                                       # the host route crops a local record as it crops an in-memory one
        assert _same(local[k], in_memory[k]), k
    assert not _same(local[1], uncropped[1])


def test_validation_set_ignores_the_option():
    cfg = hcfg.tiny()
    root = os.path.join(ROOT, "tests", "golden", "actaffordance_sample")
    a, b = aff_dataset.AffValDataset(root, cfg, seed=5), aff_dataset.AffValDataset(root, cfg, seed=5, aug_crop=1.0)
    for i in range(2):
        assert _same(a[i], b[i])
    a, b = aff_dataset.AffValDataset(root, cfg, seed=5), aff_dataset.AffValDataset(root, cfg, seed=5, aug_crop=1.0)
    assert "crop" not in b.raw_item(0)


# ---- the tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,out", [(1, 9), (5, 7), (53, 53), (101, 53), (200, 53), (212, 53), (213, 53), (37, 130), (300, 256), (456, 256),
                                   (1024, 256), (257, 1024), (1023, 1024)])
def test_vectorised_table_builder_equals_the_restatement_of_pillow(S, out):
    bounds, coeffs = preprocess.pil_resample_tables(S, out, "bicubic")
    fast_bounds, fast_coeffs = preprocess.pil_bicubic_tables_fast(S, out)
    assert fast_bounds.dtype == bounds.dtype and fast_coeffs.dtype == coeffs.dtype and fast_coeffs.shape == coeffs.shape
    assert np.array_equal(fast_bounds, bounds) and np.array_equal(fast_coeffs, coeffs)
    tab = ops.crop_table(S, out)
    assert tab.dtype == np.int32 and np.array_equal(tab[:, :2], bounds) and np.array_equal(tab[:, 2:], coeffs)
    assert ops.crop_table(S, out) is tab                          # cached per (S, out)
    if S <= 4 * out:
        assert tab.shape[1] - 2 <= 17


def test_descriptor_shares_tables_between_samples_of_one_square():
    a, b, c = _box(0, 0, 30, 21), _box(5, 3, 12, 30), _box(1, 1, 33, 9)
    d = ops.crop_descriptor([a, None, b, c], [False, True, True, False], (40, 64)).numpy()
    g = d[:48].reshape(4, 12)
    assert g[:, 7].tolist() == [4, 1, 5, 4] and not g[1, :7].any() and not g[1, 8:].any()
    assert g[0, :7].tolist() == [0, 0, 30, 21, 0, 4, 30] and g[2, :7].tolist() == [5, 3, 12, 30, 9, 0, 30]
    assert g[0, 8:].tolist() == g[2, 8:].tolist() and g[3, 8] != g[0, 8]           # one S, one table pair
    for row in (g[0], g[3]):
        for off, ks, n_out in ((row[8], row[9], 64), (row[10], row[11], 40)):
            assert np.array_equal(d[off:off + n_out * (2 + ks)].reshape(n_out, 2 + ks), ops.crop_table(int(row[6]), n_out))
    assert d.size == 48 + sum(ops.crop_table(S, n).size for S in (30, 33) for n in (64, 40))
