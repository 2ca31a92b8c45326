"""Training augmentation, the parts that need no GPU: --aug_flip / --aug_jitter and their refusals, the per-sample draw, the host
route of AffRecordsDataset (Pillow, the yardstick of the device route) and the C-ABI wiring of csrc/frame_augment.hip."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import haff
from haff import aff_dataset, config as hcfg, cvlite, train_ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"haff_jitter_stats_u8": 8, "haff_augment_u8": 9, "haff_flip_planes_u8": 7}


# ---- C-ABI wiring ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_augment_symbols_are_declared_exported_and_typed(name):
    from haff import lib as hlib
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    m = re.search(r"^int %s\(([^;]*)\);" % name, text, flags=re.M | re.S)
    assert m, f"include/haff_hip.h does not declare {name}"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    proto = hlib._PROTOS[name]
    assert len(proto) == len(params) == ENTRY_POINTS[name]
    for p, t in zip(params, proto):
        assert t is (hlib.c_void_p if "*" in p else hlib.c_int), (p, t)
    assert getattr(haff.load_library(), name).argtypes == proto
    assert "frame_augment.hip" in open(os.path.join(ROOT, "2handedafforder_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_arguments_on_the_host():
    """Nothing is launched for these: the refusals are host arithmetic on the pointers' values and the sizes."""
    lib = haff.load_library()
    P = ctypes.c_void_p
    IN, OUT, FLAGS, FACT, SUMS = 0x10000, 0x90000, 0x4000, 0x5000, 0x6000    # never dereferenced

    def stats(frames=IN, B=1, H=4, W=4, flags=FLAGS, fact=FACT, sums=SUMS):
        return int(lib.haff_jitter_stats_u8(P(frames), B, H, W, P(flags), P(fact), P(sums), None))

    def augment(src=IN, dst=OUT, B=1, H=4, W=4, flags=FLAGS, fact=FACT, sums=SUMS):
        return int(lib.haff_augment_u8(P(src), P(dst), B, H, W, P(flags), P(fact), P(sums), None))

    def planes(src=IN, dst=OUT, n=1, H=4, W=4, flags=FLAGS):
        return int(lib.haff_flip_planes_u8(P(src), P(dst), n, H, W, P(flags), None))
    for call in (stats, augment):
        assert call(B=0) == -1 and call(H=0) == -1 and call(W=-3) == -1
        assert call(flags=0) == -1 and call(fact=0) == -1 and call(sums=0) == -1
        assert call(flags=FLAGS + 2) == -1 and call(fact=FACT + 1) == -1 and call(sums=SUMS + 4) == -1
        assert call(H=4097, W=4096) == -2 and call(H=1, W=(1 << 24) + 1) == -2
        assert call(H=0, W=1 << 30) == -1                        # a bad size is a bad argument whatever the other one is
    assert stats(frames=0) == -1 and augment(src=0) == -1 and augment(dst=0) == -1
    assert augment(dst=IN) == -1 and augment(dst=IN + 47) == -1 and augment(src=IN + 40, dst=IN) == -1    # out == in, overlaps
    assert planes(n=0) == -1 and planes(H=0) == -1 and planes(W=0) == -1 and planes(src=0) == -1 and planes(dst=0) == -1
    assert planes(flags=0) == -1 and planes(flags=FLAGS + 1) == -1 and planes(dst=IN) == -1 and planes(dst=IN + 15) == -1


# ---- the flags -------------------------------------------------------------------------------------------------------------
def test_flags_default_to_off_and_parse_as_probabilities():
    args = train_ds.parse_args([])
    assert args.aug_flip == 0.0 and args.aug_jitter == 0.0
    args = train_ds.parse_args(["--aug_flip", "0.5", "--aug_jitter", "0.25"])
    assert args.aug_flip == 0.5 and args.aug_jitter == 0.25


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device before refusing the flags")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)


@pytest.mark.parametrize("flag", ["--aug_flip", "--aug_jitter"])
def test_flags_are_refused_with_synthetic_by_name(monkeypatch, flag):
    _no_device(monkeypatch)
    with pytest.raises(SystemExit) as e:
        train_ds.main([flag, "0.5", "--synthetic", "tiny"])
    assert flag in str(e.value) and "--synthetic" in str(e.value)


@pytest.mark.parametrize("flag,value", [("--aug_flip", "1.5"), ("--aug_jitter", "-0.1"), ("--aug_flip", "nan")])
def test_values_outside_the_unit_interval_are_refused_by_name(monkeypatch, flag, value):
    _no_device(monkeypatch)
    with pytest.raises(SystemExit) as e:
        train_ds.main([flag, value, "--sam_records", "unused.pt"])
    assert flag in str(e.value) and "[0, 1]" in str(e.value)
    with pytest.raises(ValueError, match=flag[2:]):
        aff_dataset.AffRecordsDataset(_records(1), hcfg.tiny(), seed=0, **{flag[2:]: float(value)})


# ---- the draw --------------------------------------------------------------------------------------------------------------
def test_draw_is_a_pure_function_of_seed_and_index():
    first = [aff_dataset.draw_augmentation(7, i, 0.5, 0.25) for i in range(50)]
    again = [aff_dataset.draw_augmentation(7, i, 0.5, 0.25) for i in reversed(range(50))][::-1]
    assert first == again                                             # whatever the call order
    other_rank = [aff_dataset.draw_augmentation(1007, i, 0.5, 0.25) for i in range(50)]
    assert other_rank != first and [a["flip"] for a in other_rank] != [a["flip"] for a in first]
    for a in first:
        assert set(a) == {"flip", "jitter"} and isinstance(a["flip"], bool)
        if a["jitter"] is not None:
            assert len(a["jitter"]) == 3
            for f in a["jitter"]:
                assert 0.4 <= f <= 1.6 and f == float(np.float32(f))  # rounded to fp32 once
    # all five draws are made whether or not they are used: the probabilities select, they do not shift the factors
    sure = aff_dataset.draw_augmentation(7, 3, 1.0, 1.0)
    assert sure["flip"] is True and sure["jitter"] is not None
    never = aff_dataset.draw_augmentation(7, 3, 0.0, 0.0)
    assert never == {"flip": False, "jitter": None}
    jittered = [i for i, a in enumerate(first) if a["jitter"] is not None]
    assert jittered and all(aff_dataset.draw_augmentation(7, i, 0.0, 1.0)["jitter"] == first[i]["jitter"] for i in jittered)


def test_draw_frequencies_over_4000_samples():
    """Seed 7 (deterministic counts): flips within 1850..2150, jitters within 900..1100 of 4000 at 0.5 / 0.25."""
    draws = [aff_dataset.draw_augmentation(7, i, 0.5, 0.25) for i in range(4000)]
    flips, jitters = sum(a["flip"] for a in draws), sum(a["jitter"] is not None for a in draws)
    print(f"flips {flips} jitters {jitters}")
    assert 1850 <= flips <= 2150 and 900 <= jitters <= 1100
    both = sum(a["flip"] and a["jitter"] is not None for a in draws)
    assert 350 <= both <= 650                                         # independent draws: about 500


# ---- the dataset -----------------------------------------------------------------------------------------------------------
def _records(n=5, hw=(48, 64), seed=0):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        x, y = 4 + 3 * i, 5 + 2 * i
        recs.append({"narration": f"Action Number {i} with the tool", "inpainted": rng.integers(0, 255, hw + (3,), dtype=np.uint8),
                     "taxonomy": [[1, 0, 0, 0], 0, [0, 0, 1, 0], 1, [0, 1, 0, 0]][i % 5],
                     "masks": {"aff_left": [[[x, y], [x + 20, y + 2], [x + 12, y + 18]]],
                               "aff_right": [] if i % 2 else [[[30, 10], [50, 12], [45, 30], [28, 28]]], "original_size": hw}})
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


def test_zero_probabilities_change_nothing(monkeypatch):
    def no_draw(*a, **k):
        raise AssertionError("draw_augmentation called with both probabilities 0")
    monkeypatch.setattr(aff_dataset, "draw_augmentation", no_draw)
    cfg = hcfg.tiny()
    plain = [aff_dataset.AffRecordsDataset(_records(), cfg, seed=11) for _ in range(2)]
    zero = [aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, aug_flip=0.0, aug_jitter=0.0) for _ in range(2)]
    for i in range(20):
        assert _same(plain[0][i], zero[0][i]), i
        a, b = plain[1].raw_item(i), zero[1].raw_item(i)
        assert "aug" not in b and _same(a, b), i
    assert plain[0].rng.getstate() == zero[0].rng.getstate()


def test_augmentation_draws_do_not_disturb_the_sample_sequence():
    cfg = hcfg.tiny()
    plain = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11)
    host = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, aug_flip=0.5, aug_jitter=0.25)
    raw = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11, aug_flip=0.5, aug_jitter=0.25)
    changed = 0
    for i in range(20):
        p, h, r = plain[i], host[i], raw.raw_item(i)
        assert h[3] == p[3] == r["conversations"] and h[9] == p[9] == r["questions"] and h[10] == p[10] == r["texts"]   # the narration too
        assert r["aug"] == aff_dataset.draw_augmentation(11, i, 0.5, 0.25)
        assert len(h) == len(p) == 12 and h[1].shape == p[1].shape and h[4].shape == p[4].shape
        changed += not torch.equal(h[1], p[1])
    assert plain.rng.getstate() == host.rng.getstate() == raw.rng.getstate()
    assert 5 <= changed < 20


def test_host_route_flip_exchanges_hands_taxonomy_and_mirrors_the_frame(monkeypatch):
    from PIL import Image
    cfg = hcfg.tiny()
    monkeypatch.setattr(aff_dataset, "draw_augmentation", lambda seed, idx, pf, pj: {"flip": True, "jitter": None})
    for k, (tax, want) in enumerate([([1, 0, 0, 0], [0, 1, 0, 0]), (0, [0, 1, 0, 0]), (1, [1, 0, 0, 0]), ([0, 0, 1, 0], [0, 0, 1, 0]),
                                     ([0.1, 0.2, 0.3, 0.4], [0.2, 0.1, 0.3, 0.4])]):
        rec = dict(_records(1, (48, 64), seed=k)[0], taxonomy=tax)
        left = cvlite.draw_contours_filled((48, 64), rec["masks"]["aff_left"])
        right = cvlite.draw_contours_filled((48, 64), rec["masks"]["aff_right"])
        assert left.sum() > 50 and right.sum() > 50 and not np.array_equal(left, right[:, ::-1])   # asymmetric hands
        plain = aff_dataset.AffRecordsDataset([rec], cfg, seed=2)[0]
        item = aff_dataset.AffRecordsDataset([rec], cfg, seed=2, aug_flip=1.0)[0]
        assert np.array_equal(item[5][0].numpy(), left[:, ::-1]) and np.array_equal(item[4][0].numpy(), right[:, ::-1])
        assert item[6] == [float(v) for v in want]
        assert torch.equal(item[7]["right"], torch.from_numpy((left[:, ::-1] == 0).astype(np.int64) * 255))
        assert item[3] == plain[3] and item[10] == plain[10]          # the narration is left alone
        mirrored = np.asarray(Image.fromarray(rec["inpainted"]).transpose(Image.FLIP_LEFT_RIGHT))
        assert np.array_equal(aff_dataset.augment_frame(rec["inpainted"], {"flip": True, "jitter": None}), mirrored)
        ref = aff_dataset.AffRecordsDataset([dict(rec, inpainted=mirrored)], cfg, seed=2)[0]
        assert torch.equal(item[1], ref[1]) and torch.equal(item[2], ref[2])   # SAM input and CLIP pixels come from the mirrored frame
        raw = aff_dataset.AffRecordsDataset([rec], cfg, seed=2, aug_flip=1.0).raw_item(0)
        assert raw["aug"] == {"flip": True, "jitter": None} and np.array_equal(raw["frame"], rec["inpainted"])
        assert raw["taxonomy"] == plain[6]                            # raw_item hands the record over as it is; DeviceIngest applies aug


def test_host_route_jitter_is_pillows_enhance_chain_before_the_resizes(monkeypatch):
    from PIL import Image, ImageEnhance
    cfg = hcfg.tiny()
    factors = tuple(float(np.float32(v)) for v in (0.7, 1.3, 0.55))
    monkeypatch.setattr(aff_dataset, "draw_augmentation", lambda seed, idx, pf, pj: {"flip": False, "jitter": factors})
    rec = _records(1)[0]
    im = Image.fromarray(rec["inpainted"])
    im = ImageEnhance.Color(ImageEnhance.Contrast(ImageEnhance.Brightness(im).enhance(factors[0])).enhance(factors[1])).enhance(factors[2])
    want = np.asarray(im)
    assert np.array_equal(aff_dataset.augment_frame(rec["inpainted"], {"flip": False, "jitter": factors}), want)
    item = aff_dataset.AffRecordsDataset([rec], cfg, seed=2, aug_jitter=1.0)[0]
    ref = aff_dataset.AffRecordsDataset([dict(rec, inpainted=want)], cfg, seed=2)[0]
    plain = aff_dataset.AffRecordsDataset([rec], cfg, seed=2)[0]
    assert torch.equal(item[1], ref[1]) and torch.equal(item[2], ref[2]) and not torch.equal(item[1], plain[1])
    assert torch.equal(item[4], plain[4]) and item[6] == plain[6]     # masks and taxonomy are not touched by the jitter


def test_from_local_takes_the_keywords(tmp_path):
    import json
    recs = _records(3)
    (tmp_path / "h5").mkdir()
    (tmp_path / "jsons").mkdir()
    (tmp_path / "h5" / "0-2_a.h5").write_bytes(b"")
    json.dump({str(i): {"original_size": [48, 64], "aff_left": r["masks"]["aff_left"], "aff_right": r["masks"]["aff_right"]}
               for i, r in enumerate(recs)}, open(tmp_path / "jsons" / "0-2_a.json", "w"))
    data = {"data": {"inpainted": np.stack([r["inpainted"] for r in recs]), "narration": [r["narration"].encode() for r in recs],
                     "taxonomy": [2, 0, 1]}}
    kw = dict(h5_open=lambda path: data, seed=5)
    plain = aff_dataset.AffRecordsDataset.from_local(str(tmp_path), hcfg.tiny(), **kw)
    ds = aff_dataset.AffRecordsDataset.from_local(str(tmp_path), hcfg.tiny(), aug_flip=0.5, aug_jitter=0.25, **kw)
    assert (plain.aug_flip, plain.aug_jitter) == (0.0, 0.0) and (ds.aug_flip, ds.aug_jitter, ds.aug_seed) == (0.5, 0.25, 5)
    assert "aug" not in plain.raw_item(0) and ds.raw_item(0)["aug"] == aff_dataset.draw_augmentation(5, 0, 0.5, 0.25)


def test_validation_set_ignores_the_options():
    cfg = hcfg.tiny()
    root = os.path.join(ROOT, "tests", "golden", "actaffordance_sample")
    a = aff_dataset.AffValDataset(root, cfg, seed=5)
    b = aff_dataset.AffValDataset(root, cfg, seed=5, aug_flip=1.0, aug_jitter=1.0)
    for i in range(3):
        assert _same(a[i], b[i])
    a, b = aff_dataset.AffValDataset(root, cfg, seed=5), aff_dataset.AffValDataset(root, cfg, seed=5, aug_flip=1.0, aug_jitter=1.0)
    for i in range(3):
        raw = b.raw_item(i)
        assert "aug" not in raw and _same(a.raw_item(i), raw)
