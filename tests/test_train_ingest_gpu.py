"""Device-side training ingest on the GPU: haff_fill_contours_u8 byte for byte against cvlite.draw_contours_filled, DeviceIngest.batch
against collate_fn on the same raw samples, LisaTrainable.forward(frames_u8=) against the host-built batch, and train_ds.main
--device_ingest end to end (tiny geometry, fp32)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/contour_ref.py, tests/test_train_gpu.py
import contour_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

# The project's bar for feeding the SAM encoder from uint8 frames instead of host-normalised tensors
# (tests/test_preprocess_gpu.py::test_evaluate_from_uint8_frames_equals_host_preprocessing, on evaluate() outputs).
REL = 2e-5


def _fill(planes, hw, dev, out=None):
    from haff import ops
    return ops.fill_contours(planes, hw, dev, out=out).cpu().numpy()


def _ref(planes, hw):
    from haff import cvlite
    return np.stack([cvlite.draw_contours_filled(hw, cs) for cs in planes]) if planes else np.zeros((0,) + tuple(hw), np.uint8)


@pytest.mark.parametrize("name", sorted(R.named_cases()))
def test_fill_equals_cvlite_on_the_named_shapes(dev, name):
    hw, cs = R.named_cases()[name]
    got = _fill([cs], hw, dev)
    want = _ref([cs], hw)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ"
    if name in ("empty", "outside"):
        assert not got.any()
    if name == "comb":
        assert max(len(R.row_spans([tuple(p) for p in cs[0]], y)) for y in range(5, 36)) == 40   # 80 crossings: two ballot passes


def test_fill_one_launch_over_five_planes_does_not_bleed(dev):
    hw, planes = R.MULTI_PLANE
    assert [len(p) for p in planes] == [0, 1, 3, 1, 0]
    got = _fill(planes, hw, dev)
    assert np.array_equal(got, _ref(planes, hw))
    assert not got[0].any() and not got[4].any() and got[2].all()


def test_fill_equals_cvlite_on_the_300_random_cases(dev):
    """The cases of the CPU test, one launch per plane size (every polygon list on a plane of its own)."""
    cases = R.random_cases(300, 0)
    for hw in sorted({hw for hw, _ in cases}):
        planes = [cs for h, cs in cases if h == hw]
        got, want = _fill(planes, hw, dev), _ref(planes, hw)
        bad = [i for i in range(len(planes)) if not np.array_equal(got[i], want[i])]
        assert not bad, f"{hw}: planes {bad[:5]} differ, first contours {planes[bad[0]]}"


def test_fill_zeroes_a_dirty_buffer(dev):
    hw, planes = R.MULTI_PLANE
    out = torch.full((len(planes),) + hw, 0xAB, dtype=torch.uint8, device=dev)
    first = _fill(planes, hw, dev, out=out)
    again = _fill(planes, hw, dev, out=out)          # now dirty with the first result, and a different request
    assert np.array_equal(first, _ref(planes, hw)) and np.array_equal(again, first)
    moved = [planes[1], [], [], [], planes[3]]
    assert np.array_equal(_fill(moved, hw, dev, out=out), _ref(moved, hw))


def _over_limit_contours():
    from haff import ops
    many = [[5 + (i % 30), 5 + (i // 30) % 20] for i in range(ops.FILL_MAX_VERTS + 1)]
    far = [[3, 3], [ops.FILL_MAX_COORD, 10], [20, 25]]
    return many, far


def test_fill_refuses_over_limit_polygons_and_touches_nothing(dev):
    from haff import ops
    from haff.lib import HaffLibraryError
    ok = [[2, 2], [20, 4], [9, 17]]
    for bad in _over_limit_contours():
        assert not ops.fill_contours_supported(bad) and ops.fill_contours_supported(ok)
        out = torch.full((2, 33, 47), 0x5A, dtype=torch.uint8, device=dev)
        with pytest.raises(HaffLibraryError, match="code -1"):
            ops.fill_contours([[ok], [bad]], (33, 47), dev, out=out)
        torch.cuda.synchronize()
        assert bool((out == 0x5A).all())
    at_limit = [[5 + (i % 30), 5 + (i // 30) % 20] for i in range(ops.FILL_MAX_VERTS)]
    assert np.array_equal(_fill([[at_limit]], (33, 47), dev), _ref([[at_limit]], (33, 47)))


# ---- the batch -------------------------------------------------------------------------------------------------------------------
def _blob(cx, cy, r, n, k):
    t = 2 * np.pi * np.arange(n) / n
    rad = r * (1 + 0.25 * np.sin(k * t))
    return np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], 1).astype(np.int32).tolist()


def _records(n, hw, seed=0):
    rng = np.random.default_rng(seed)
    H, W = hw
    texts = ["cut the bread", "open the drawer", "pour water", "hold the pan", "stir the pot", "lift the lid"]
    recs = []
    for i in range(n):
        recs.append({"narration": texts[i % 6], "inpainted": rng.integers(0, 255, (H, W, 3), dtype=np.uint8),
                     "taxonomy": [[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]][i % 3],
                     "masks": {"aff_left": [_blob(W * 0.3, H * 0.4, H * 0.2, 40 + i, 5), _blob(W * 0.5, H * 0.8, H * 0.1, 12, 3)],
                               "aff_right": [_blob(W * 0.7, H * 0.5, H * 0.25, 60, 4 + i)], "original_size": (H, W)}})
    return recs


@pytest.fixture(scope="module")
def two_batches(dev):
    """The same two seeded samples as collate_fn's host-built batch and as DeviceIngest's: two 300 x 400 frames with contours."""
    from haff import aff_dataset, checkpoint, config as hcfg, train_ds
    from haff.train_ingest import DeviceIngest
    cfg = hcfg.tiny()
    tok = checkpoint.ByteTokenizer(cfg)
    recs = _records(3, (300, 400))
    a, b = aff_dataset.AffRecordsDataset(recs, cfg, seed=4), aff_dataset.AffRecordsDataset(recs, cfg, seed=4)
    host = train_ds.collate_fn([a[0], a[1]], tok, 575)
    raws = [b.raw_item(0), b.raw_item(1)]
    ingest = DeviceIngest(cfg, dev, torch.float32)
    device = ingest.batch(raws, tok, 575, "llava_v1")
    return cfg, tok, host, device, raws, ingest


def test_device_batch_equals_collate_fn(two_batches):
    cfg, tok, host, device, raws, ingest = two_batches
    assert set(device) == set(host) | {"frames_u8"} and device["images"] is None
    assert device["frames_u8"].shape == (2, 300, 400, 3) and device["frames_u8"].dtype == torch.uint8 and device["frames_u8"].is_cuda
    for k in ("input_ids", "labels", "attention_masks", "offset", "taxonomies_list"):
        assert device[k].dtype == host[k].dtype and torch.equal(device[k].cpu(), host[k]), k
    assert device["resize_list"] == host["resize_list"] == [(168, 224)] * 2
    assert device["conversation_list"] == host["conversation_list"] and device["inference"] is host["inference"] is False
    assert device["questions_list"] == host["questions_list"] and device["sampled_classes_list"] == host["sampled_classes_list"]
    for k in ("masks_list_left", "masks_list_right"):
        for d, h in zip(device[k], host[k]):
            assert d.is_cuda and d.dtype == h.dtype and d.shape == h.shape == (1, 300, 400) and torch.equal(d.cpu(), h), k
        assert all(float(d.sum()) > 1000 for d in device[k])
    for d, h in zip(device["label_list"], host["label_list"]):
        assert tuple(d["left"].shape) == tuple(h["left"].shape) == (300, 400) and tuple(d["right"].shape) == tuple(h["right"].shape)
    err = (device["images_clip"].cpu() - host["images_clip"]).abs().max().item()
    print(f"images_clip max abs difference {err:.3e}")
    assert device["images_clip"].shape == host["images_clip"].shape and err <= 1e-6
    assert ingest.host_fills == 0


def test_over_limit_polygon_takes_the_host_fill(two_batches, dev):
    from haff import cvlite
    from haff.train_ingest import DeviceIngest
    cfg, tok, host, device, raws, _ = two_batches
    many, _far = _over_limit_contours()
    raw = dict(raws[0], contours_left=[many], mask_hw=(33, 47), frame=raws[0]["frame"])
    ingest = DeviceIngest(cfg, dev, torch.float32)
    out = ingest.batch([raw], tok, 575, "llava_v1")
    assert ingest.host_fills == 1
    assert np.array_equal(out["masks_list_left"][0][0].cpu().numpy(), cvlite.draw_contours_filled((33, 47), [many]).astype(np.float32))
    assert np.array_equal(out["masks_list_right"][0][0].cpu().numpy(),
                          cvlite.draw_contours_filled((33, 47), raw["contours_right"]).astype(np.float32))


def test_frames_of_different_sizes_become_a_list(two_batches, dev):
    from haff import aff_dataset, train_ds
    from haff.train_ingest import DeviceIngest
    cfg, tok = two_batches[0], two_batches[1]
    recs = _records(1, (90, 120)) + _records(1, (120, 90), seed=1)
    for r in recs:                       # one mask size, so that forward can stack the ground truth
        r["masks"]["original_size"] = (64, 80)
        r["masks"]["aff_left"], r["masks"]["aff_right"] = [_blob(30, 30, 15, 20, 3)], [_blob(50, 40, 12, 16, 4)]
    raws = []
    for r in recs:
        raws.append(aff_dataset.AffRecordsDataset([r], cfg, seed=2).raw_item(0))
    out = DeviceIngest(cfg, dev, torch.float32).batch(raws, tok, 575, "llava_v1")
    assert isinstance(out["frames_u8"], list) and [tuple(f.shape) for f in out["frames_u8"]] == [(90, 120, 3), (120, 90, 3)]
    assert out["resize_list"] == [(168, 224), (224, 168)] and out["images_clip"].shape == (2, 3, 224, 224)
    host = train_ds.collate_fn([aff_dataset.AffRecordsDataset([r], cfg, seed=2)[0] for r in recs], tok, 575)
    assert (out["images_clip"].cpu() - host["images_clip"]).abs().max().item() <= 1e-6
    for k in ("masks_list_left", "masks_list_right"):
        assert all(torch.equal(d.cpu(), h) for d, h in zip(out[k], host[k]))


def test_validation_set_batch_and_inference_forward(two_batches, dev):
    """AffValDataset through DeviceIngest: the uploaded PNG planes, > 0; forward(inference=True) gives the host-built batch's masks."""
    from haff import aff_dataset, train_ds, weights as hw
    from haff.train_ingest import DeviceIngest
    from haff.train_model import LisaTrainable
    cfg, tok = two_batches[0], two_batches[1]
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")
    a, b = aff_dataset.AffValDataset(root, cfg, seed=3), aff_dataset.AffValDataset(root, cfg, seed=3)
    host = train_ds.collate_fn([a[0]], tok, 575)
    device = DeviceIngest(cfg, dev, torch.float32).batch([b.raw_item(0)], tok, 575, "llava_v1")
    assert device["inference"] is True and torch.equal(device["input_ids"], host["input_ids"]) and device["resize_list"] == host["resize_list"]
    assert torch.equal(device["taxonomies_list"], host["taxonomies_list"])
    for k in ("masks_list_left", "masks_list_right"):
        assert torch.equal(device[k][0].cpu(), (host[k][0] > 0).float()), k
    assert (device["images_clip"].cpu() - host["images_clip"]).abs().max().item() <= 1e-6
    model = LisaTrainable(cfg, hw.make_state_dict(cfg, 21), dtype=torch.float32, device=dev, lora_dropout=0.0, seed=3).eval()
    with torch.no_grad():
        out_h = model(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in host.items()})
        out_d = model(**device)
    for k in ("pred_masks_left", "pred_masks_right", "pred_taxonomies"):
        ref = out_h[k].float().cpu()
        err = (out_d[k].float().cpu() - ref).abs().max().item()
        print(f"{k}: max abs difference {err:.3e} of {ref.abs().max().item():.3e}")
        assert err <= REL * ref.abs().max().item(), k


# Worst |g_device - g_host| / max|g_host| over the tensors of a class, fp32, tiny geometry, the two 300 x 400 frames of `two_batches`.
# Every class starts from REL (2e-5); a class listed here would have needed more and be bounded at 4x its measured value (fp32
# re-association between two correct paths moves by small factors between shapes and devices; a wrong pixel moves a loss by orders
# more). Measured on MI355X: 0 for all six losses and all ten gradient classes (the device-built batch is bit-identical: the ingest
# kernels are Pillow-exact and haff_patchify_u8 normalises as the host does), images_clip difference 0. So no class is listed.
GRAD_CLASS_BOUND = {}
LOSS_KEYS = ("loss", "ce_loss", "taxonomy_ce_loss", "mask_bce_loss", "mask_dice_loss", "mask_loss")


def test_forward_from_uint8_frames_matches_the_host_built_batch(two_batches, dev):
    from haff import weights as hw
    from haff.train_model import LisaTrainable
    from test_train_gpu import grad_class
    cfg, tok, host, device, raws, _ = two_batches
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
    for k in LOSS_KEYS:
        rel = abs(loss_d[k] - loss_h[k]) / max(abs(loss_h[k]), 1e-12)
        print(f"{k}: host-built {loss_h[k]:.7f} device-built {loss_d[k]:.7f} rel {rel:.3e}")
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
    print("worst gradient difference per class: " + ", ".join(f"{c} {v:.3e}" for c, v in sorted(by_class.items())))
    for k in LOSS_KEYS:
        assert np.isfinite(loss_d[k]) and abs(loss_d[k] - loss_h[k]) <= REL * abs(loss_h[k]), k
    for c, v in by_class.items():
        assert v <= GRAD_CLASS_BOUND.get(c, REL), f"gradient class {c}: {v:.3e} > {GRAD_CLASS_BOUND.get(c, REL):.3e}"


# ---- train_ds.main --device_ingest ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint_files(tmp_path_factory):
    from haff import config as hcfg, weights as hw
    from test_real_weights_gpu import _write_inputs
    tmp = tmp_path_factory.mktemp("ingest_cli")
    cfg = hcfg.tiny()
    base, clip, sam, _ = _write_inputs(tmp, cfg, hw.make_state_dict(cfg, 9))
    records = tmp / "six_records.pt"
    torch.save(_records(6, (96, 128)), str(records))
    return cfg, tmp, ["--version", str(base), "--vision-tower", str(clip), "--vision_pretrained", str(sam), "--sam_records", str(records),
                      "--steps_per_epoch", "2", "--grad_accumulation_steps", "1", "--batch_size", "2", "--precision", "fp32",
                      "--log_base_dir", str(tmp / "runs"), "--val_samples", "2", "--lr", "0.0003", "--image_size", str(cfg.sam.img_size),
                      "--model_max_length", "3000", "--lora_dropout", "0.0"]


def _numbers(out):
    losses = [float(v) for v in re.findall(r"\tLoss (\S+) \(", out)]
    iou = [(float(a), float(b)) for a, b in re.findall(r"IoU: (\S+), IoCM: (\S+)", out)]
    return losses, iou


def _spy_on_raw_item(monkeypatch):
    from haff import aff_dataset
    seen = []
    raw_item = aff_dataset.AffRecordsDataset.raw_item

    def spy(self, idx):
        if not self.inference:
            seen.append(idx)
        return raw_item(self, idx)
    monkeypatch.setattr(aff_dataset.AffRecordsDataset, "raw_item", spy)
    return seen


def _prefetch_threads():
    import threading
    return [t for t in threading.enumerate() if t.name.startswith("haff-prefetch")]


def test_train_ds_device_ingest_matches_the_host_loader(dev, checkpoint_files, capsys, monkeypatch):
    """2 steps + validation with the flag and without it: the progress lines' losses and the validation IoU / IoCM agree within REL
    plus 1e-4, the resolution of the four printed decimals (each value is rounded on its own)."""
    from haff import train_ds
    cfg, tmp, argv = checkpoint_files
    seen = _spy_on_raw_item(monkeypatch)
    train_ds.main(argv + ["--epochs", "1", "--exp_name", "dev", "--device_ingest"])
    out_d = capsys.readouterr().out
    assert seen[:4] == [0, 1, 2, 3] and seen == list(range(len(seen))) and len(seen) <= 4 + 3 * 2   # in order, two batches ahead
    assert not _prefetch_threads()
    train_ds.main(argv + ["--epochs", "1", "--exp_name", "host"])
    out_h = capsys.readouterr().out
    assert len(seen) <= 4 + 3 * 2                        # the host loader never calls raw_item
    (loss_d, iou_d), (loss_h, iou_h) = _numbers(out_d), _numbers(out_h)
    print("device ingest:", loss_d, iou_d, "| host loader:", loss_h, iou_h)
    assert len(loss_d) == len(loss_h) == 2 and len(iou_d) == len(iou_h) == 1
    for a, b in zip(loss_d + list(iou_d[0]), loss_h + list(iou_h[0])):
        assert np.isfinite(a) and abs(a - b) <= REL * abs(b) + 1e-4, (a, b)


def test_train_ds_device_ingest_resumes_at_the_next_sample(dev, checkpoint_files, capsys, monkeypatch):
    from haff import train_ds
    cfg, tmp, argv = checkpoint_files
    seen = _spy_on_raw_item(monkeypatch)
    run = argv + ["--exp_name", "resume", "--device_ingest", "--no_eval"]      # without validation every epoch saves latest.pt
    train_ds.main(run + ["--epochs", "1"])
    assert "saved checkpoint" in capsys.readouterr().out and seen[:4] == [0, 1, 2, 3]
    del seen[:]
    train_ds.main(run + ["--epochs", "2"])
    out = capsys.readouterr().out
    assert "resume training from" in out and "start from epoch 1" in out and "Epoch: [1][1/2]" in out
    assert seen[:4] == [4, 5, 6, 7]                      # global_step 2 x accumulation 1 x batch 2: the next sample
    losses = _numbers(out)[0]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses)
    assert not _prefetch_threads()
