"""The object crop on the GPU feed: DeviceIngest.batch on samples that carry a "crop" box against collate_fn on the host route (Pillow),
to the byte, LisaTrainable's losses and gradients from both batches, to the bit (tiny geometry, fp32), and the samples the device
route hands to the host."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/test_train_ingest_gpu.py
from test_train_ingest_gpu import LOSS_KEYS, _blob   # noqa: E402

pytestmark = pytest.mark.gpu

FACTORS = tuple(float(np.float32(v)) for v in (1.45, 0.6, 1.2))
DRAWS = [{"flip": True, "jitter": FACTORS}, {"flip": False, "jitter": FACTORS}]       # forced per sample index


def _records(hw=(48, 64), frame_hw=None):
    """Two records with object contours beside the affordance ones; the second has one hand only."""
    H, W = hw
    rng = np.random.default_rng(12)
    recs = []
    for i in range(2):
        recs.append({"narration": ["cut the bread", "open the drawer"][i],
                     "inpainted": rng.integers(0, 255, tuple(frame_hw or hw) + (3,), dtype=np.uint8),
                     "taxonomy": [[1, 0, 0, 0], [0, 0, 1, 0]][i],
                     "masks": {"original_size": hw, "aff_left": [_blob(W * 0.3, H * 0.4, H * 0.12, 14 + i, 3)],
                               "aff_right": [] if i else [_blob(W * 0.55, H * 0.5, H * 0.1, 12, 4)],
                               "obj_left": [_blob(W * 0.3, H * 0.45, H * 0.2, 20, 5)],
                               "obj_right": [] if i else [_blob(W * 0.6, H * 0.5, H * 0.15, 16, 3)]}})
    return recs


def _feeds(dev, monkeypatch, recs, **kw):
    """The same two samples (one record each, so the sample is known) through both feeds, with DRAWS forced and every crop drawn."""
    from haff import aff_dataset, checkpoint, config as hcfg, train_ds
    from haff.train_ingest import DeviceIngest
    cfg = hcfg.tiny()
    tok = checkpoint.ByteTokenizer(cfg)
    items, raws = [], []
    for i, r in enumerate(recs):
        monkeypatch.setattr(aff_dataset, "draw_augmentation", lambda seed, idx, pf, pj, aug=DRAWS[i]: aug)
        items.append(aff_dataset.AffRecordsDataset([r], cfg, seed=2, aug_flip=0.5, aug_jitter=0.5, aug_crop=1.0)[0])
        raws.append(aff_dataset.AffRecordsDataset([r], cfg, seed=2, aug_flip=0.5, aug_jitter=0.5, aug_crop=1.0).raw_item(0))
    ingest = DeviceIngest(cfg, dev, torch.float32)
    return cfg, tok, train_ds.collate_fn(items, tok, 575), ingest.batch(raws, tok, 575, "llava_v1", **kw), raws, ingest


def _expected_frame(rec, aug, hw):
    """flip -> (resize to the planes' size) -> crop -> jitter with Pillow: the host loader's frame before its own resizes."""
    from haff import aff_dataset, cvlite
    m = rec["masks"]
    box = aff_dataset.crop_box(m["obj_left"], m["obj_right"], hw, flip=aug["flip"])
    left, right = cvlite.draw_contours_filled(hw, m["aff_left"]), cvlite.draw_contours_filled(hw, m["aff_right"])
    frame = aff_dataset.host_crop_sample(rec["inpainted"], left, right, [0.0] * 4, aug, box)[0]
    return aff_dataset.augment_frame(frame, {"flip": False, "jitter": aug["jitter"]})


def _assert_same_batch(device, host):
    for k in ("input_ids", "labels", "attention_masks", "offset", "taxonomies_list"):
        assert device[k].dtype == host[k].dtype and torch.equal(device[k].cpu(), host[k]), k
    assert device["resize_list"] == host["resize_list"] and device["conversation_list"] == host["conversation_list"]
    for k in ("masks_list_left", "masks_list_right"):
        for d, h in zip(device[k], host[k]):
            assert d.is_cuda and d.dtype == h.dtype and d.shape == h.shape and torch.equal(d.cpu(), h), k
    err = (device["images_clip"].cpu() - host["images_clip"]).abs().max().item()
    print(f"images_clip max abs difference {err:.3e}")
    assert device["images_clip"].dtype == host["images_clip"].dtype and torch.equal(device["images_clip"].cpu(), host["images_clip"])


def test_device_batch_equals_the_host_route_to_the_byte(dev, monkeypatch):
    from haff import ops
    calls = []
    crop_resample = ops.crop_resample
    monkeypatch.setattr(ops, "crop_resample", lambda x, *a, **k: (calls.append(tuple(x.shape)), crop_resample(x, *a, **k))[1])
    monkeypatch.setattr(ops, "flip_planes", lambda *a, **k: pytest.fail("the crop launch mirrors the planes itself"))
    recs = _records()
    cfg, tok, host, device, raws, ingest = _feeds(dev, monkeypatch, recs)
    assert all(r["crop"] is not None and r["aug"] == a for r, a in zip(raws, DRAWS))
    assert calls == [(2, 48, 64, 3), (4, 48, 64, 1)]            # one launch for the frames, one for both hands' planes of the batch
    frames = device["frames_u8"]
    assert frames.shape == (2, 48, 64, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    for i, (rec, aug) in enumerate(zip(recs, DRAWS)):
        want = _expected_frame(rec, aug, (48, 64))
        assert np.array_equal(frames[i].cpu().numpy(), want), i
        assert not np.array_equal(want, rec["inpainted"])
    _assert_same_batch(device, host)
    assert device["taxonomies_list"].tolist() == [[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]     # the mirrored sample's hands exchanged
    assert float(device["masks_list_right"][0].sum()) > 0 and float(device["masks_list_left"][1].sum()) > 0
    assert ingest.host_crops == 0 and ingest.crop_skipped == 0 and ingest.host_augments == 0 and ingest.host_fills == 0


def test_the_crop_changes_frames_and_masks_against_flip_and_jitter_alone(dev, monkeypatch):
    """A silently skipped crop cannot pass: the same draws without aug_crop give other pixels and other masks."""
    from haff import aff_dataset, checkpoint, config as hcfg
    from haff.train_ingest import DeviceIngest
    recs = _records()
    cfg, tok, host, device, raws, _ = _feeds(dev, monkeypatch, recs)
    bare = []
    for i, r in enumerate(recs):
        monkeypatch.setattr(aff_dataset, "draw_augmentation", lambda seed, idx, pf, pj, aug=DRAWS[i]: aug)
        bare.append(aff_dataset.AffRecordsDataset([r], cfg, seed=2, aug_flip=0.5, aug_jitter=0.5).raw_item(0))
    assert all("crop" not in r for r in bare)
    plain = DeviceIngest(cfg, dev, torch.float32).batch(bare, tok, 575, "llava_v1")
    assert torch.equal(plain["input_ids"], device["input_ids"]) and torch.equal(plain["taxonomies_list"], device["taxonomies_list"])
    for i in range(2):
        assert not torch.equal(plain["frames_u8"][i], device["frames_u8"][i])
        assert not torch.equal(plain["masks_list_left"][i], device["masks_list_left"][i])


def test_a_frame_of_another_size_takes_the_host_route_and_is_counted(dev, monkeypatch):
    from haff import ops
    recs = _records(frame_hw=(60, 90))
    calls = []
    crop_resample = ops.crop_resample
    monkeypatch.setattr(ops, "crop_resample", lambda x, *a, **k: (calls.append(tuple(x.shape)), crop_resample(x, *a, **k))[1])
    cfg, tok, host, device, raws, ingest = _feeds(dev, monkeypatch, recs)
    assert ingest.host_crops == 2 and ingest.crop_skipped == 0 and calls == []
    assert device["frames_u8"].shape == (2, 48, 64, 3)          # the reference resizes the frame to the planes' size before it crops
    for i, (rec, aug) in enumerate(zip(recs, DRAWS)):
        assert np.array_equal(device["frames_u8"][i].cpu().numpy(), _expected_frame(rec, aug, (48, 64))), i
    _assert_same_batch(device, host)


def test_a_geometry_beyond_the_kernels_limit_takes_the_host_route_and_is_counted(dev, monkeypatch):
    """The limits themselves are pinned on the entry point; here the scale limit is lowered so that these samples pass it."""
    from haff import ops
    recs = _records()
    cfg, tok, host, want, raws, ingest = _feeds(dev, monkeypatch, recs)
    monkeypatch.setattr(ops, "CROP_MAX_SCALE", 1)               # S = 64 on H = 48
    monkeypatch.setattr(ops, "crop_resample", lambda *a, **k: pytest.fail("the crop kernel was called for a geometry over the limit"))
    cfg, tok, host, device, raws, ingest = _feeds(dev, monkeypatch, recs)
    assert ingest.host_crops == 2
    assert torch.equal(device["frames_u8"], want["frames_u8"]) and torch.equal(device["images_clip"], want["images_clip"])
    for k in ("masks_list_left", "masks_list_right"):
        assert all(torch.equal(a, b) for a, b in zip(device[k], want[k])), k
    assert torch.equal(device["taxonomies_list"], want["taxonomies_list"])


def test_samples_without_object_contours_are_not_cropped_and_are_counted(dev, monkeypatch):
    recs = _records()
    for r in recs:
        r["masks"]["obj_left"], r["masks"]["obj_right"] = [], []
    cfg, tok, host, device, raws, ingest = _feeds(dev, monkeypatch, recs)
    assert all(r["crop"] is None and r["crop_skipped"] for r in raws)
    assert ingest.crop_skipped == 2 and ingest.host_crops == 0
    _assert_same_batch(device, host)                            # flip and jitter as without the crop


def test_frames_of_different_sizes_are_cropped_one_call_each(dev, monkeypatch):
    from haff import ops
    recs = [_records((48, 64))[0], _records((56, 40))[1]]
    calls = []
    crop_resample = ops.crop_resample
    monkeypatch.setattr(ops, "crop_resample", lambda x, *a, **k: (calls.append(tuple(x.shape)), crop_resample(x, *a, **k))[1])
    cfg, tok, host, device, raws, ingest = _feeds(dev, monkeypatch, recs)
    assert isinstance(device["frames_u8"], list) and [tuple(f.shape) for f in device["frames_u8"]] == [(48, 64, 3), (56, 40, 3)]
    assert sorted(calls) == sorted([(1, 48, 64, 3), (1, 56, 40, 3), (2, 48, 64, 1), (2, 56, 40, 1)])
    for f, rec, aug in zip(device["frames_u8"], recs, DRAWS):
        assert np.array_equal(f.cpu().numpy(), _expected_frame(rec, aug, rec["masks"]["original_size"]))
    _assert_same_batch(device, host)
    assert ingest.host_crops == 0


def test_losses_and_gradients_are_the_same_to_the_bit_on_both_feeds(dev, monkeypatch):
    from haff import weights as hw
    from haff.train_model import LisaTrainable
    cfg, tok, host, device, raws, _ = _feeds(dev, monkeypatch, _records())
    model = LisaTrainable(cfg, hw.make_state_dict(cfg, 21), dtype=torch.float32, device=dev, lora_dropout=0.0, lora_init_b_zero=False,
                          seed=3)
    runs = []
    for batch in ({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in host.items()}, device):
        model.zero_grad()
        out = model(**batch)
        out["loss"].backward()
        runs.append(({k: float(out[k].detach()) for k in LOSS_KEYS},
                     {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}))
    (loss_h, grad_h), (loss_d, grad_d) = runs
    worst = max((grad_d[k] - g).abs().max().item() for k, g in grad_h.items())
    print("host-built", loss_h, "device-built", loss_d, f"worst gradient difference {worst:.3e}")
    assert set(grad_h) == set(grad_d) and len(grad_h) > 150
    for k in LOSS_KEYS:
        assert np.isfinite(loss_d[k]) and loss_d[k] == loss_h[k], k
    for k, g in grad_h.items():
        assert torch.equal(grad_d[k], g), k


# ---- train_ds.main --aug_crop -----------------------------------------------------------------------------------------------------
def test_train_ds_crops_alike_on_both_feeds(dev, tmp_path, capsys, monkeypatch):
    """train_ds.py --aug_flip --aug_crop --aug_jitter with --device_ingest (HIP, tables made by the prefetch thread) and without
    (Pillow): the same printed losses, within the bar of tests/test_train_augment_gpu.py (REL plus the four printed decimals)."""
    from haff import aff_dataset, config as hcfg, ops, train_ds, weights as hw
    from test_real_weights_gpu import _write_inputs
    from test_train_ingest_gpu import REL, _numbers
    cfg = hcfg.tiny()
    base, clip, sam, _ = _write_inputs(tmp_path, cfg, hw.make_state_dict(cfg, 9))
    recs = []
    for k in range(3):
        for r in _records((96, 128)):
            recs.append(dict(r, inpainted=np.random.default_rng(k).integers(0, 255, (96, 128, 3), dtype=np.uint8)))
    recs[1]["narration"] = "put something down"                  # always cropped
    torch.save(recs, str(tmp_path / "records.pt"))
    argv = ["--version", str(base), "--vision-tower", str(clip), "--vision_pretrained", str(sam), "--sam_records",
            str(tmp_path / "records.pt"), "--steps_per_epoch", "2", "--grad_accumulation_steps", "1", "--batch_size", "4", "--precision",
            "fp32", "--log_base_dir", str(tmp_path / "runs"), "--val_samples", "2", "--lr", "0.0003", "--image_size", str(cfg.sam.img_size),
            "--model_max_length", "3000", "--lora_dropout", "0.0", "--epochs", "1", "--seed", "7", "--no_eval", "--aug_flip", "0.5",
            "--aug_crop", "0.6667", "--aug_jitter", "0.25"]
    drawn = [aff_dataset.draw_crop(7, i, 0.6667) for i in range(8)]
    assert 2 <= sum(drawn) < 8 and any(drawn[:4]) and any(drawn[4:])
    calls, tables = [], []
    crop_resample, crop_table = ops.crop_resample, ops.crop_table
    monkeypatch.setattr(ops, "crop_resample", lambda x, *a, **k: (calls.append(tuple(x.shape)), crop_resample(x, *a, **k))[1])

    def spy_table(S, out):
        import threading
        tables.append(threading.current_thread().name)
        return crop_table(S, out)
    monkeypatch.setattr(ops, "crop_table", spy_table)
    ops._crop_tables.clear()
    train_ds.main(argv + ["--exp_name", "dev", "--device_ingest"])
    out_d = capsys.readouterr().out
    assert calls == [(4, 96, 128, 3), (8, 96, 128, 1)] * 2       # a launch pair per step: training only
    assert tables and tables[0].startswith("haff-prefetch")      # the first builder of a table is the prefetch thread
    assert "training augmentation: flip p=0.5, object crop p=0.6667, colour jitter p=0.25 (HIP kernels on the device)" in out_d
    assert "cropped on the host" not in out_d
    train_ds.main(argv + ["--exp_name", "host"])
    out_h = capsys.readouterr().out
    assert len(calls) == 4 and "object crop p=0.6667, colour jitter p=0.25 (Pillow on the host)" in out_h
    (loss_d, _), (loss_h, _) = _numbers(out_d), _numbers(out_h)
    print("device ingest:", loss_d, "| host loader:", loss_h)
    assert len(loss_d) == len(loss_h) == 2
    for a, b in zip(loss_d, loss_h):
        assert np.isfinite(a) and abs(a - b) <= REL * abs(b) + 1e-4, (a, b)
