"""Training augmentation on the GPU: DeviceIngest.batch on samples that carry "aug" against collate_fn on the host route (Pillow),
LisaTrainable.forward(frames_u8=) against the host-built augmented batch, and train_ds.main --aug_flip --aug_jitter on both feeds
(tiny geometry, fp32)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/augment_ref.py, tests/test_train_ingest_gpu.py
import augment_ref as A   # noqa: E402
from test_train_ingest_gpu import LOSS_KEYS, REL, _blob, _numbers, _records   # noqa: E402  (REL: the project's bar for feeding uint8 frames)

pytestmark = pytest.mark.gpu

# With flip 1.0 / jitter 0.5 dataset seed 20 draws {flip} for sample 0 and {flip, jitter} for sample 1 (asserted in the fixture).
SEED = 20


@pytest.fixture(scope="module")
def augmented_batches(dev):
    """Two 300 x 400 records, one mirrored and one mirrored and jittered, as collate_fn's host-built batch (Pillow), as DeviceIngest's
    (HIP), and the un-augmented device batch of the same samples."""
    from haff import aff_dataset, checkpoint, config as hcfg, train_ds
    from haff.train_ingest import DeviceIngest
    cfg = hcfg.tiny()
    tok = checkpoint.ByteTokenizer(cfg)
    recs = _records(3, (300, 400))
    kw = dict(seed=SEED, aug_flip=1.0, aug_jitter=0.5)
    a, b = aff_dataset.AffRecordsDataset(recs, cfg, **kw), aff_dataset.AffRecordsDataset(recs, cfg, **kw)
    plain = aff_dataset.AffRecordsDataset(recs, cfg, seed=SEED)
    host = train_ds.collate_fn([a[0], a[1]], tok, 575)
    raws = [b.raw_item(0), b.raw_item(1)]
    assert raws[0]["aug"]["flip"] and raws[0]["aug"]["jitter"] is None and raws[1]["aug"]["flip"] and raws[1]["aug"]["jitter"] is not None
    ingest = DeviceIngest(cfg, dev, torch.float32)
    device = ingest.batch(raws, tok, 575, "llava_v1")
    bare = DeviceIngest(cfg, dev, torch.float32).batch([plain.raw_item(0), plain.raw_item(1)], tok, 575, "llava_v1")
    return cfg, tok, host, device, bare, raws, ingest


def test_device_batch_equals_the_host_route(augmented_batches):
    cfg, tok, host, device, bare, raws, ingest = augmented_batches
    assert set(device) == set(bare) == set(host) | {"frames_u8"} and device["images"] is None   # exactly the keys of an un-augmented batch
    frames = device["frames_u8"]
    assert frames.shape == (2, 300, 400, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    for i, r in enumerate(raws):
        want = A.pil_augment(r["frame"], r["aug"]["flip"], r["aug"]["jitter"])
        assert np.array_equal(frames[i].cpu().numpy(), want), i
        assert not np.array_equal(want, r["frame"])
    for k in ("input_ids", "labels", "attention_masks", "offset", "taxonomies_list"):
        assert device[k].dtype == host[k].dtype and torch.equal(device[k].cpu(), host[k]), k
    assert device["resize_list"] == host["resize_list"] == [(168, 224)] * 2
    assert device["conversation_list"] == host["conversation_list"] and device["questions_list"] == host["questions_list"]
    for k in ("masks_list_left", "masks_list_right"):
        for d, h in zip(device[k], host[k]):
            assert d.is_cuda and d.dtype == h.dtype and d.shape == h.shape == (1, 300, 400) and torch.equal(d.cpu(), h), k
    err = (device["images_clip"].cpu() - host["images_clip"]).abs().max().item()
    print(f"images_clip max abs difference {err:.3e}")
    assert err <= 1e-6
    assert ingest.host_augments == 0 and ingest.host_fills == 0


def test_both_feeds_differ_from_the_unaugmented_batch(augmented_batches):
    """A silently skipped augmentation cannot pass: same samples and prompts, other pixels, masks and taxonomies."""
    cfg, tok, host, device, bare, raws, _ = augmented_batches
    assert torch.equal(bare["input_ids"], device["input_ids"])
    for i in range(2):
        assert torch.equal(bare["frames_u8"][i].cpu(), torch.from_numpy(raws[i]["frame"]))
        assert not torch.equal(bare["frames_u8"][i], device["frames_u8"][i])
        assert not torch.equal(bare["images_clip"][i], device["images_clip"][i])
        assert not torch.equal(bare["images_clip"][i].cpu(), host["images_clip"][i])
        # the mirrored sample's right hand is the mirror of its old left hand
        assert torch.equal(device["masks_list_right"][i], bare["masks_list_left"][i].flip(-1))
        assert torch.equal(device["masks_list_left"][i], bare["masks_list_right"][i].flip(-1))
        assert not torch.equal(device["masks_list_left"][i], bare["masks_list_left"][i])
        assert not torch.equal(host["masks_list_left"][i], bare["masks_list_left"][i].cpu())
    taxes = bare["taxonomies_list"].tolist()
    assert device["taxonomies_list"].tolist() == [[t[1], t[0], t[2], t[3]] for t in taxes]
    assert any(t[0] != t[1] for t in taxes)                    # and the exchange is visible on these records


def test_frames_of_different_sizes_are_augmented_one_call_each(augmented_batches, dev, monkeypatch):
    from haff import aff_dataset, train_ds
    from haff.train_ingest import DeviceIngest
    cfg, tok = augmented_batches[0], augmented_batches[1]
    recs = _records(1, (90, 120)) + _records(1, (120, 90), seed=1) + _records(1, (64, 67), seed=2)
    for r in recs:                       # one mask size, so that forward can stack the ground truth
        r["masks"]["original_size"] = (64, 80)
        r["masks"]["aff_left"], r["masks"]["aff_right"] = [_blob(30, 30, 15, 20, 3)], [_blob(50, 40, 12, 16, 4)]
    factors = tuple(A.fp32(v) for v in (1.45, 0.6, 1.2))
    draws = [{"flip": True, "jitter": factors}, {"flip": False, "jitter": None}, {"flip": False, "jitter": factors}]
    raws, items = [], []
    for r, aug in zip(recs, draws):
        monkeypatch.setattr(aff_dataset, "draw_augmentation", lambda seed, idx, pf, pj, aug=aug: aug)
        raws.append(aff_dataset.AffRecordsDataset([r], cfg, seed=2, aug_flip=0.5).raw_item(0))
        items.append(aff_dataset.AffRecordsDataset([r], cfg, seed=2, aug_flip=0.5)[0])
    ingest = DeviceIngest(cfg, dev, torch.float32)
    out = ingest.batch(raws, tok, 575, "llava_v1")
    host = train_ds.collate_fn(items, tok, 575)
    assert isinstance(out["frames_u8"], list) and [tuple(f.shape) for f in out["frames_u8"]] == [(90, 120, 3), (120, 90, 3), (64, 67, 3)]
    for f, r, aug in zip(out["frames_u8"], raws, draws):
        assert np.array_equal(f.cpu().numpy(), A.pil_augment(r["frame"], aug["flip"], aug["jitter"]))
    assert (out["images_clip"].cpu() - host["images_clip"]).abs().max().item() <= 1e-6
    for k in ("masks_list_left", "masks_list_right"):
        assert all(torch.equal(d.cpu(), h) for d, h in zip(out[k], host[k])), k
    assert torch.equal(out["taxonomies_list"], host["taxonomies_list"]) and ingest.host_augments == 0


def test_frames_over_the_kernels_limit_are_augmented_on_the_host_and_counted(augmented_batches, dev, monkeypatch):
    """The limit itself (2^24 pixels) is pinned on the entry points; here it is lowered so that 300 x 400 frames pass it."""
    from haff import ops
    from haff.train_ingest import DeviceIngest
    cfg, tok, host, device, bare, raws, _ = augmented_batches
    monkeypatch.setattr(ops, "AUG_MAX_PIXELS", 300 * 400 - 1)

    def no_kernel(*a, **k):
        raise AssertionError("the frame kernels were called for a frame over the limit")
    monkeypatch.setattr(ops, "augment_frames", no_kernel)
    ingest = DeviceIngest(cfg, dev, torch.float32)
    out = ingest.batch(raws, tok, 575, "llava_v1")
    assert ingest.host_augments == 2
    assert torch.equal(out["frames_u8"], device["frames_u8"]) and torch.equal(out["images_clip"], device["images_clip"])
    for k in ("masks_list_left", "masks_list_right"):      # the planes are still mirrored on the device
        assert all(torch.equal(a, b) for a, b in zip(out[k], device[k])), k
    assert torch.equal(out["taxonomies_list"], device["taxonomies_list"])


def test_forward_from_augmented_uint8_frames_matches_the_host_built_batch(augmented_batches, dev):
    """Measured on MI355X: see the printed lines; 0 is expected for all six losses and every gradient class, because the augmented
    frames, masks and taxonomies are bit-identical on the two routes."""
    from haff import weights as hw
    from haff.train_model import LisaTrainable
    from test_train_gpu import grad_class
    cfg, tok, host, device, bare, raws, _ = augmented_batches
    model = LisaTrainable(cfg, hw.make_state_dict(cfg, 21), dtype=torch.float32, device=dev, lora_dropout=0.0, lora_init_b_zero=False,
                          seed=3)
    runs = []
    for batch in ({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in host.items()}, device, bare):
        model.zero_grad()
        out = model(**batch)
        out["loss"].backward()
        runs.append(({k: float(out[k].detach()) for k in LOSS_KEYS},
                     {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}))
    (loss_h, grad_h), (loss_d, grad_d), (loss_b, _) = runs
    worst = 0.0
    for k in LOSS_KEYS:
        rel = abs(loss_d[k] - loss_h[k]) / max(abs(loss_h[k]), 1e-12)
        worst = max(worst, rel)
        print(f"{k}: host-built {loss_h[k]:.7f} device-built {loss_d[k]:.7f} rel {rel:.3e} (un-augmented {loss_b[k]:.7f})")
    by_class = {}
    assert set(grad_h) == set(grad_d) and len(grad_h) > 150
    for k, gh in grad_h.items():
        scale = gh.abs().max().item()
        err = (grad_d[k] - gh).abs().max().item()
        if scale < 1e-6:          # analytically zero gradients (k_proj.bias: softmax is shift-invariant) are float noise
            assert err < 1e-6, k
            continue
        c = grad_class(k)
        by_class[c] = max(by_class.get(c, 0.0), err / scale)
    print(f"worst loss difference {worst:.3e}; worst gradient difference per class: "
          + ", ".join(f"{c} {v:.3e}" for c, v in sorted(by_class.items())))
    for k in LOSS_KEYS:
        assert np.isfinite(loss_d[k]) and abs(loss_d[k] - loss_h[k]) <= REL * abs(loss_h[k]), k
    for c, v in by_class.items():
        assert v <= REL, f"gradient class {c}: {v:.3e} > {REL:.3e}"
    assert abs(loss_b["loss"] - loss_d["loss"]) > 100 * REL * abs(loss_d["loss"])     # the augmentation reaches the losses


# ---- train_ds.main --aug_flip --aug_jitter ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint_files(tmp_path_factory):
    from haff import config as hcfg, weights as hw
    from test_real_weights_gpu import _write_inputs
    tmp = tmp_path_factory.mktemp("augment_cli")
    cfg = hcfg.tiny()
    base, clip, sam, _ = _write_inputs(tmp, cfg, hw.make_state_dict(cfg, 9))
    records = tmp / "six_records.pt"
    torch.save(_records(6, (96, 128)), str(records))
    # 3 steps of 4 samples: with --seed 7 the samples 5, 6 and 10 are mirrored and 9 and 11 jittered (asserted in the test)
    return ["--version", str(base), "--vision-tower", str(clip), "--vision_pretrained", str(sam), "--sam_records", str(records),
            "--steps_per_epoch", "3", "--grad_accumulation_steps", "1", "--batch_size", "4", "--precision", "fp32",
            "--log_base_dir", str(tmp / "runs"), "--val_samples", "2", "--lr", "0.0003", "--image_size", str(cfg.sam.img_size),
            "--model_max_length", "3000", "--lora_dropout", "0.0", "--epochs", "1", "--seed", "7", "--aug_flip", "0.5",
            "--aug_jitter", "0.25"]


def test_train_ds_augments_alike_on_both_feeds(dev, checkpoint_files, capsys, monkeypatch):
    """The same losses and validation scores with --device_ingest (HIP) and without (Pillow), within REL plus 1e-4, the resolution
    of the four printed decimals."""
    from haff import aff_dataset, ops, train_ds
    draws = [aff_dataset.draw_augmentation(7, i, 0.5, 0.25) for i in range(12)]
    assert [i for i, a in enumerate(draws) if a["flip"]] == [5, 6, 10] and [i for i, a in enumerate(draws) if a["jitter"]] == [9, 11]
    calls = {"frames": 0, "planes": 0}
    augment_frames, flip_planes = ops.augment_frames, ops.flip_planes

    def count_frames(*a, **k):
        calls["frames"] += 1
        return augment_frames(*a, **k)

    def count_planes(*a, **k):
        calls["planes"] += 1
        return flip_planes(*a, **k)
    monkeypatch.setattr(ops, "augment_frames", count_frames)
    monkeypatch.setattr(ops, "flip_planes", count_planes)
    train_ds.main(checkpoint_files + ["--exp_name", "dev", "--device_ingest"])
    out_d = capsys.readouterr().out
    assert calls == {"frames": 2, "planes": 2}             # the second and third batches; training only, never the validation set
    assert "training augmentation: flip p=0.5, colour jitter p=0.25" in out_d and "augmented on the host" not in out_d
    train_ds.main(checkpoint_files + ["--exp_name", "host"])
    out_h = capsys.readouterr().out
    assert calls == {"frames": 2, "planes": 2} and "training augmentation: flip p=0.5, colour jitter p=0.25" in out_h
    (loss_d, iou_d), (loss_h, iou_h) = _numbers(out_d), _numbers(out_h)
    print("device ingest:", loss_d, iou_d, "| host loader:", loss_h, iou_h)
    assert len(loss_d) == len(loss_h) == 3 and len(iou_d) == len(iou_h) == 1
    for a, b in zip(loss_d + list(iou_d[0]), loss_h + list(iou_h[0])):
        assert np.isfinite(a) and abs(a - b) <= REL * abs(b) + 1e-4, (a, b)
