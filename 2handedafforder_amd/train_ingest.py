"""Device-side training ingest (train_ds.py --device_ingest): the fine-tune batch made on the GPU.

The default loader builds every sample on the host inside the step loop: two Pillow resizes, a normalised fp32 [3,S,S] tensor, two
Python polygon fills and two int64 label planes per sample (aff_dataset.AffRecordsDataset.__getitem__, utils/aff_dataset.py:198-280
of the reference). Here the loader hands over only the uint8 frame, the contour vertex lists and the prompt (`raw_item`), and

  images_clip       FrameIngest.clip_pixels           (csrc/frame_ingest.hip, Pillow-exact)
  SAM input         LisaTrainable.forward(frames_u8=)  (FrameIngest.sam_frames + haff_patchify_u8, as evaluate(frames_u8=))
  ground-truth masks ops.fill_contours                  (csrc/contour_fill.hip, cvlite-exact)
  augmentation      ops.augment_frames / flip_planes   (csrc/frame_augment.hip, Pillow-exact; only for samples that carry "aug")
  object crop       ops.crop_resample                  (csrc/frame_crop.hip, Pillow-exact; only for samples that carry a "crop" box)

are made from them in HBM. The text half is train_ds.collate_text, the code collate_fn itself runs. `Prefetcher` is the one
background thread that calls `raw_item` (decode, HDF5 read, prompt) and the tokeniser ahead of the step loop; the main thread
only uploads and launches.
"""
import queue
import threading

import torch

from . import cvlite
from . import ops
from .aff_dataset import augment_frame, flip_taxonomy, host_crop_sample
from .preprocess import FrameIngest, get_preprocess_shape


class Prefetcher:
    """One producer thread: `fetch(i)` for consecutive i from `start`, `batch_size` at a time, at most `depth` finished batches
    ahead of the consumer (one producer keeps a seeded dataset's rng sequence). `get()` returns (items, prepare(items)) of the next
    batch, in order; an exception in the thread is raised by the `get()` that reaches it, and by every later one. The thread ends on
    `close()` (also when the queue is full and nobody consumes) and is a daemon, so an abandoned loop cannot keep the process alive."""

    def __init__(self, fetch, start, batch_size, depth=2, prepare=None):
        self._fetch, self._prepare, self._next, self._bs = fetch, prepare, int(start), int(batch_size)
        self._q = queue.Queue(maxsize=depth)
        self._stop = threading.Event()
        self._error = None
        self._thread = threading.Thread(target=self._run, name="haff-prefetch", daemon=True)
        self._thread.start()

    def _put(self, entry):
        while not self._stop.is_set():
            try:
                self._q.put(entry, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def _run(self):
        try:
            while not self._stop.is_set():
                items = []
                for _ in range(self._bs):
                    items.append(self._fetch(self._next))
                    self._next += 1
                entry = (items, self._prepare(items) if self._prepare is not None else None)
                if not self._put((entry, None)):
                    return
        except BaseException as e:   # noqa: BLE001 — handed to the consumer, whatever it is
            self._put((None, e))

    def get(self):
        if self._error is not None:
            raise self._error
        if self._stop.is_set():
            raise RuntimeError("Prefetcher.get() after close()")
        entry, err = self._q.get()
        if err is not None:
            self._error = err
            raise err
        return entry

    def close(self):
        self._stop.set()
        while True:          # make room, so a producer blocked on a full queue sees the stop flag at once
            try:
                self._q.get_nowait()
            except queue.Empty:
                break
        self._thread.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _ShapeOnly:
    """label_list entry: forward() reads label planes only for their .shape (the reference's int64 H x W planes are never built)."""

    def __init__(self, hw):
        self.shape = torch.Size(hw)


class DeviceIngest:
    """raw samples (dataset.raw_item) -> the dict train_ds.collate_fn returns, with `images` None, `frames_u8` the batch's uint8 HWC
    frames in HBM (one [B,H,W,3] tensor when the sizes agree, else a list of [H,W,3]), `images_clip` / the mask lists made on the
    device and `label_list` carrying shapes only. `host_fills` counts the planes that had a polygon beyond the fill kernel's
    host-checked limits (ops.FILL_MAX_VERTS vertices, |coordinate| < ops.FILL_MAX_COORD) and were filled by cvlite instead.
    A sample that carries "aug" (aff_dataset.draw_augmentation) is augmented here as AffRecordsDataset.__getitem__ does it on the
    host: the uploaded frame is jittered and / or mirrored before anything is derived from it, the filled planes are mirrored and
    exchanged between the hands, taxonomy entries 0 and 1 are exchanged. `host_augments` counts the frames beyond
    ops.AUG_MAX_PIXELS, which Pillow augmented before the upload.
    A sample that carries a "crop" box (aff_dataset.crop_box of a sample that drew the object crop) is mirrored and cropped in one
    pass of ops.crop_resample, frames and filled planes alike, before the jitter: flip -> crop -> jitter as on the host. `host_crops`
    counts the samples the host cropped before the upload (a frame of another size than its planes, which the reference resizes
    first, or a geometry beyond ops.crop_supported); `crop_skipped` those that drew the crop and had no object to centre on."""

    def __init__(self, cfg, device, dtype):
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        if self.device.type != "cuda":
            raise RuntimeError("DeviceIngest builds the batch in HBM (cuda device); the host loader is train_ds.collate_fn")
        self.ingest = FrameIngest(self.device)
        self.host_fills = 0
        self.host_augments = 0
        self.host_crops = 0
        self.crop_skipped = 0

    def text(self, raw_samples, tokenizer, model_max_length=575, conv_type="llava_v1"):
        """The text half (host only: what Prefetcher runs in its thread). The crop's coefficient tables are made here too, so the
        main thread finds them in ops.crop_table's cache."""
        from .train_ds import collate_text
        for r in raw_samples:
            if r.get("crop") is not None:
                for n_out in r["mask_hw"]:
                    ops.crop_table(r["crop"]["S"], n_out)
        convs, offs = [], [0]
        for r in raw_samples:
            convs.extend(r["conversations"])
            offs.append(offs[-1] + len(r["conversations"]))
        return collate_text(convs, tokenizer, model_max_length, True, conv_type, inference=raw_samples[0]["inference"], offsets=offs)

    def _host_crops(self, raw_samples):
        """The samples as the device route takes them: one whose crop the kernel does not take is cropped here with Pillow (mirror
        included; the jitter stays for the device) and goes on as a frame with finished planes, like a validation sample."""
        out = []
        for r in raw_samples:
            self.crop_skipped += bool(r.get("crop_skipped"))
            box = r.get("crop")
            if box is not None and (r["frame"].shape[:2] != tuple(r["mask_hw"]) or not ops.crop_supported(r["mask_hw"], box["S"])):
                aug = r.get("aug")
                left, right = (cvlite.draw_contours_filled(tuple(r["mask_hw"]), list(r[k] or []), 1)
                               for k in ("contours_left", "contours_right"))
                frame, left, right, taxonomy = host_crop_sample(r["frame"], left, right, r["taxonomy"], aug, box)
                r = {k: v for k, v in r.items() if k not in ("contours_left", "contours_right", "crop")}
                r.update(frame=frame, plane_left=left, plane_right=right, taxonomy=taxonomy)
                if aug is not None:
                    r["aug"] = {"flip": False, "jitter": aug["jitter"]}
                self.host_crops += 1
            out.append(r)
        return out

    def _frames(self, raw_samples):
        """The uploaded frames, augmented: one [B,H,W,3] tensor with per-frame flags, or one call per frame of a list."""
        frames = [r["frame"] for r in raw_samples]
        boxes = [r.get("crop") for r in raw_samples]
        # None for a sample that drew nothing (or carries no draw: the validation sets)
        augs = [a if a and (a["flip"] or a["jitter"] is not None) else None for a in (r.get("aug") for r in raw_samples)]
        for i, a in enumerate(augs):
            if a and not ops.augment_frames_supported(frames[i].shape[:2]):
                frames[i], augs[i] = augment_frame(frames[i], a), None       # beyond the kernels' limit: Pillow, before the upload
                self.host_augments += 1
        frames = self._upload_frames(frames)
        if any(boxes):                     # mirror and crop in one pass; what is left for augment_frames is the jitter
            flips = [bool(a and a["flip"]) for a in augs]
            if torch.is_tensor(frames):    # the samples without a box are copied (mirrored where they drew the flip)
                frames = ops.crop_resample(frames, boxes, flips)
                cropped = [True] * len(augs)
            else:
                frames = [ops.crop_resample(f[None], [b], [fl])[0] if b else f for f, b, fl in zip(frames, boxes, flips)]
                cropped = [b is not None for b in boxes]
            augs = [({"flip": False, "jitter": a["jitter"]} if a["jitter"] is not None else None) if a and c else a
                    for a, c in zip(augs, cropped)]
        if not any(augs):
            return frames
        if torch.is_tensor(frames):
            return ops.augment_frames(frames, augs)
        return [ops.augment_frames(f[None], [a])[0] if a else f for f, a in zip(frames, augs)]

    def _upload_frames(self, frames):
        if len({f.shape for f in frames}) == 1:
            host = torch.empty((len(frames),) + frames[0].shape, dtype=torch.uint8, pin_memory=True)
            for i, f in enumerate(frames):
                host[i].copy_(torch.from_numpy(f))
            return host.to(self.device, non_blocking=True)
        return [ops.upload_pinned(f, self.device) for f in frames]

    def _masks(self, raw_samples):
        """float [1,H,W] per sample and hand. Samples of one mask size share one launch of the fill kernel."""
        n = len(raw_samples)
        left, right = [None] * n, [None] * n
        groups = {}
        for i, r in enumerate(raw_samples):
            if "plane_left" in r:          # validation set: the PNG planes are the ground truth
                for dst, key in ((left, "plane_left"), (right, "plane_right")):
                    dst[i] = (ops.upload_pinned(r[key], self.device) > 0).float()[None]
            else:
                groups.setdefault(tuple(r["mask_hw"]), []).append(i)
        for hw, idxs in groups.items():
            planes, redo = [], []
            for i in idxs:
                for key in ("contours_left", "contours_right"):
                    contours = list(raw_samples[i][key] or [])
                    if all(ops.fill_contours_supported(c) for c in contours):
                        planes.append(contours)
                    else:                  # beyond the kernel's limits: this plane is filled on the host and uploaded
                        planes.append([])
                        redo.append((len(planes) - 1, contours))
            filled = ops.fill_contours(planes, hw, self.device)
            for k, contours in redo:
                filled[k].copy_(ops.upload_pinned(cvlite.draw_contours_filled(hw, contours), self.device), non_blocking=True)
                self.host_fills += 1
            flips = [bool((raw_samples[i].get("aug") or {}).get("flip")) for i in idxs]
            boxes = [raw_samples[i].get("crop") for i in idxs]
            if any(boxes):                 # both hands' planes of the group in one launch: mirror, then the crop of the mirrored plane
                filled = ops.crop_resample(filled[..., None], [b for b in boxes for _ in range(2)],
                                           [f for f in flips for _ in range(2)])[..., 0]
            elif any(flips):               # flip(fill(contours)), never a fill of mirrored vertices: the scanline fill is not symmetric
                flags = torch.tensor([ops.AUG_FLIP * f for f in flips for _ in range(2)], dtype=torch.int32).pin_memory()
                filled = ops.flip_planes(filled, flags.to(self.device, non_blocking=True))
            filled = filled.float()
            for j, i in enumerate(idxs):
                a, b = (1, 0) if flips[j] else (0, 1)          # a mirrored sample's right hand is its old left one
                left[i], right[i] = filled[2 * j + a][None], filled[2 * j + b][None]
        return left, right

    def batch(self, raw_samples, tokenizer, model_max_length=575, conv_type="llava_v1", text=None):
        cfg = self.cfg
        if text is None:
            text = self.text(raw_samples, tokenizer, model_max_length, conv_type)
        if any("crop" in r for r in raw_samples):
            raw_samples = self._host_crops(raw_samples)
        frames = self._frames(raw_samples)
        if torch.is_tensor(frames):
            clip = self.ingest.clip_pixels(frames, cfg.clip.image, self.dtype)
        else:
            clip = torch.cat([self.ingest.clip_pixels(f[None], cfg.clip.image, self.dtype) for f in frames], 0)
        left, right = self._masks(raw_samples)
        return {"images": None, "frames_u8": frames, "images_clip": clip,
                # the small integer tensors stay on the host: forward() does its bookkeeping from host copies and uploads them itself
                "input_ids": text["input_ids"], "labels": text["labels"], "attention_masks": text["attention_masks"],
                "masks_list_left": left, "masks_list_right": right,
                "label_list": [{"left": _ShapeOnly(r["mask_hw"]), "right": _ShapeOnly(r["mask_hw"])} for r in raw_samples],
                "resize_list": [get_preprocess_shape(r["frame"].shape[0], r["frame"].shape[1], cfg.sam.img_size) for r in raw_samples],
                "offset": text["offset"], "inference": raw_samples[0]["inference"], "conversation_list": text["conversation_list"],
                "taxonomies_list": torch.stack([torch.tensor(flip_taxonomy(r["taxonomy"]) if (r.get("aug") or {}).get("flip")
                                                             else r["taxonomy"]) for r in raw_samples], 0),
                "image_paths": [None] * len(raw_samples), "questions_list": [r["questions"] for r in raw_samples],
                "sampled_classes_list": [r["texts"] for r in raw_samples]}
