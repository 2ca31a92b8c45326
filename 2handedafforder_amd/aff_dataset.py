"""2HANDS sample loader — the caller BEFORE the training path.

Mirrors `2Haff/utils/aff_dataset.py:48-346` (`AffDataset`) for records of the public HF dataset layout
(`_load_from_huggingface`, :117-150): each record carries `narration` (or `text`), `image` (or `inpainted`), `taxonomy`
and `masks = {aff_left: [contour, ...], aff_right: [...], original_size: (h, w)}` with OpenCV-style contours
(lists of (x, y) points). `__getitem__` reproduces :198-280: a RANDOM record per call (the reference ignores `idx`),
masks re-drawn from the contours, the question/answer templates of :29-46, one conversation of the default template (llava_v1 unless train_ds.py --conv_type says otherwise), CLIP and SAM
preprocessing, and the 11/12-tuple that `collate_fn` (utils/dataset.py:30-169 = train_ds.collate_fn here) consumes.

`AffValDataset` mirrors `AffDatasetVal` (:350-544): the benchmark folder walk (`<root>/<video>/<frame>/{inpainting.png,
aff_left.png, aff_right.png, annotation.json}`, a missing hand is an all-zero mask, frames without an image / annotation /
any mask are skipped), the same 12-tuple with `inference=True`.

Contours are filled by `cvlite.draw_contours_filled`, a restatement of `cv2.drawContours(..., FILLED)` from OpenCV's published
sources (this image has no cv2; tests/test_cvlite_cpu.py holds hand-derived fixtures — parity with cv2 itself is unpinned).
The local h5/json layout (`_load_from_local`, :152-183, :307-338) is `AffRecordsDataset.from_local`: all of its index / ordering
logic is here; the HDF5 reader itself is h5py, which is not installed in this image (ImportError naming it unless `h5_open=` is given).
"""
import random

import numpy as np
import torch

from . import cvlite
from . import preprocess
from . import prompt as hprompt

SHORT_QUESTION_LIST = [
    hprompt.DEFAULT_IMAGE_TOKEN + "\n" + "Can you show me where I have to interact with the objects to perform the following task: {class_name}?",
    hprompt.DEFAULT_IMAGE_TOKEN + "\n" + "Please segment the region to perform the action '{class_name}' in this image.",
    hprompt.DEFAULT_IMAGE_TOKEN + "\n" + "How can I perform the action '{class_name}' in this image? Please respond with segmentation mask.",
    hprompt.DEFAULT_IMAGE_TOKEN + "\n" + "How can I perform the action '{class_name}' in this image? Please output segmentation mask.",
]
ANSWER_LIST = ["It is [SEG].", "Sure, [SEG].", "Sure, it is [SEG].", "Sure, the segmentation result is [SEG].", "[SEG]."]


def recreate_mask_from_contours(contours, shape):
    """aff_dataset.py:340-346: binary uint8 mask of `shape` = (h, w) with every contour filled
    (`cv2.drawContours(mask, [np.array(contour, np.int32)], -1, 1, thickness=cv2.FILLED)` per contour)."""
    return cvlite.draw_contours_filled(shape, contours, 1)


def _taxonomy_vector(t):
    """Records store the 4-way soft target [left-only, right-only, both, both] (LISA.py:359-361); a bare class index
    becomes its one-hot."""
    if isinstance(t, bytes):
        t = int(t.decode("utf-8"))
    if isinstance(t, (int, np.integer)):
        v = [0.0] * 4
        v[int(t)] = 1.0
        return v
    v = [float(x) for x in np.asarray(t, dtype=np.float64).reshape(-1)]
    assert len(v) == 4, f"taxonomy must have 4 entries, got {len(v)}"
    return v


JITTER_RANGE = (0.4, 1.6)   # apply_jitter.py: brightness, contrast and colour factors


def check_probability(name, p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{name} is a probability in [0, 1], not {p}")
    return p


def draw_augmentation(seed, idx, p_flip, p_jitter):
    """The training augmentation of sample `idx`: {"flip": bool, "jitter": None | (fb, fc, fs)}. A pure function of its arguments
    (a generator of its own per (dataset seed, idx), never the dataset's rng), so it is the same on resume, on either feed and
    whatever the fetch order. Five draws in a fixed order, made whether or not they are used: flip, jitter, then the brightness,
    contrast and colour factors, uniform in JITTER_RANGE and rounded to fp32 once (Pillow hands `(float)alpha` to its C code)."""
    g = random.Random(f"haff-aug/{seed}/{idx}")
    u_flip, u_jitter = g.random(), g.random()
    factors = tuple(float(np.float32(g.uniform(*JITTER_RANGE))) for _ in range(3))
    return {"flip": u_flip < p_flip, "jitter": factors if u_jitter < p_jitter else None}


def augment_frame(image, aug):
    """`aug` on a uint8 HWC frame with Pillow itself (the yardstick of csrc/frame_augment.hip): apply_jitter.py's
    Brightness -> Contrast -> Color and horizontal_flip.py's mirror. They commute: the jitter is pointwise apart from one
    whole-frame mean, which a mirror keeps."""
    from PIL import Image, ImageEnhance
    if not aug["flip"] and aug["jitter"] is None:
        return image
    im = Image.fromarray(image, "RGB")
    if aug["jitter"] is not None:
        for enhance, f in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), aug["jitter"]):
            im = enhance(im).enhance(f)
    if aug["flip"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.array(im)          # a writable copy, as the record's own frame is


def flip_taxonomy(v):
    """horizontal_flip.py exchanges the hands: left-only <-> right-only, entries 0 and 1 of the 4-vector."""
    return [v[1], v[0]] + list(v[2:])


CROP_MARGIN = 50                         # process_cropped_sequences.py: the object box is grown by 50 px on every side
CROP_ALWAYS = ("something", "things")    # a narration with one of these names no object: the reference always crops it


def draw_crop(seed, idx, p_crop, narration=""):
    """Whether sample `idx` is replaced by its object-centred view (process_cropped_sequences.py). A pure function with a generator
    of its own, apart from draw_augmentation's, so setting it leaves the flip and jitter draws of every index as they were.
    One uniform draw; a narration that says "something" or "things" is cropped whatever the draw."""
    if p_crop <= 0.0:
        return False
    u = random.Random(f"haff-crop/{seed}/{idx}").random()
    return u < p_crop or any(w in narration for w in CROP_ALWAYS)


def crop_box(obj_left, obj_right, hw, flip=False):
    """The crop of process_cropped_sequences.py for planes of hw = (H, W): the inclusive extremes of fill(obj_left) | fill(obj_right),
    grown by CROP_MARGIN and clamped (x1 / y1 exclusive although max_x / max_y are inclusive, as in the script), then centred on a
    square of side S = max(cw, ch). flip: the box of the MIRRORED planes (the mirror of a crop is not the crop of the mirror).
    Vertex extremes when every vertex lies inside the plane (a filled polygon touches its extreme vertices), else the extremes of
    the filled union. None when there is no object pixel."""
    H, W = int(hw[0]), int(hw[1])
    polys = [np.asarray(c, dtype=np.int32).reshape(-1, 2) for c in list(obj_left or []) + list(obj_right or [])]
    polys = [p for p in polys if len(p)]
    if not polys:
        return None
    pts = np.concatenate(polys, 0)
    lo, hi = pts.min(0), pts.max(0)
    if lo[0] >= 0 and lo[1] >= 0 and hi[0] < W and hi[1] < H:
        min_x, min_y, max_x, max_y = int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1])
    else:
        ys, xs = np.nonzero(cvlite.draw_contours_filled((H, W), polys, 1))
        if len(ys) == 0:
            return None
        min_x, min_y, max_x, max_y = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
    if flip:
        min_x, max_x = W - 1 - max_x, W - 1 - min_x
    x0, y0 = max(min_x - CROP_MARGIN, 0), max(min_y - CROP_MARGIN, 0)
    x1, y1 = min(max_x + CROP_MARGIN, W), min(max_y + CROP_MARGIN, H)
    cw, ch = x1 - x0, y1 - y0
    S = max(cw, ch)
    return {"x0": x0, "y0": y0, "cw": cw, "ch": ch, "px": (S - cw) // 2, "py": (S - ch) // 2, "S": S}


def crop_image(image, box):
    """crop_and_pad of process_cropped_sequences.py with Pillow itself (the yardstick of csrc/frame_crop.hip) on a uint8 HWC frame
    or a uint8 HW plane: the box cut out, pasted centred on a black square and stretched back to the image's size (bicubic)."""
    from PIL import Image
    im = Image.fromarray(image, "RGB" if image.ndim == 3 else "L")
    square = Image.new(im.mode, (box["S"], box["S"]))
    square.paste(im.crop((box["x0"], box["y0"], box["x0"] + box["cw"], box["y0"] + box["ch"])), (box["px"], box["py"]))
    return np.array(square.resize(im.size, Image.BICUBIC))


def crop_plane(plane, box):
    """A 0/1 filled plane through crop_image as a 0/255 `L` plane; the new mask is every non-zero pixel of the result."""
    return (crop_image((plane != 0).astype(np.uint8) * 255, box) != 0).astype(np.uint8)


def resize_frame(image, hw):
    """The frame at the planes' size (process_cropped_sequences.py resizes it before it crops): Pillow's bicubic."""
    from PIL import Image
    return np.array(Image.fromarray(image, "RGB").resize((int(hw[1]), int(hw[0])), Image.BICUBIC))


def host_crop_sample(image, left, right, taxonomy, aug, box):
    """flip -> crop of one sample on the host: the frame (brought to the planes' size first), both filled planes and the taxonomy.
    `box` is crop_box(..., flip=aug's flip). The jitter is left to the caller: it follows the crop."""
    if aug is not None and aug["flip"]:
        image = augment_frame(image, {"flip": True, "jitter": None})
        left, right = np.ascontiguousarray(right[:, ::-1]), np.ascontiguousarray(left[:, ::-1])
        taxonomy = flip_taxonomy(taxonomy)
    if image.shape[:2] != left.shape:
        image = resize_frame(image, left.shape)
    return crop_image(image, box), crop_plane(left, box), crop_plane(right, box), taxonomy


class AffRecordsDataset(torch.utils.data.Dataset):
    """AffDataset over in-memory records (what `load_dataset(name, split="train")` yields). aug_flip / aug_jitter: the probabilities
    of the training augmentation (draw_augmentation; both 0: none, and nothing about the samples changes). aug_crop: the probability
    of the object-centred view (draw_crop; 0: no draw, no new key anywhere); the records then carry masks["obj_left" / "obj_right"].
    `crop_skipped` counts the samples that drew a crop and had no object to centre on."""

    def __init__(self, records, cfg, samples_per_epoch=500 * 8 * 2 * 10, inference=False, seed=None, aug_flip=0.0, aug_jitter=0.0,
                 aug_crop=0.0):
        self.records = list(records)
        if not self.records:
            raise ValueError("no records")
        self.cfg, self.samples_per_epoch, self.inference = cfg, samples_per_epoch, inference
        self.size = len(self.records)
        self.original_size = None
        for r in self.records:
            m = r.get("masks") or {}
            if "original_size" in m:
                self.original_size = tuple(int(x) for x in m["original_size"])
                break
        self.rng = random.Random(seed)
        self._set_augmentation(seed, aug_flip, aug_jitter, aug_crop)

    def _set_augmentation(self, seed, aug_flip, aug_jitter, aug_crop=0.0):
        self.aug_flip, self.aug_jitter = check_probability("aug_flip", aug_flip), check_probability("aug_jitter", aug_jitter)
        self.aug_crop, self.crop_skipped = check_probability("aug_crop", aug_crop), 0
        # an unseeded dataset draws its samples from the OS; so does its augmentation
        self.aug_seed = seed if seed is not None else random.SystemRandom().getrandbits(63)

    def _draw_aug(self, idx):
        """None when both probabilities are 0 (no draw is made), else draw_augmentation for this sample."""
        if self.aug_flip == 0.0 and self.aug_jitter == 0.0:
            return None
        return draw_augmentation(self.aug_seed, idx, self.aug_flip, self.aug_jitter)

    def _draw_crop_box(self, idx, text, masks, shape, aug):
        """None, or crop_box of a sample that drew the crop (no draw at all with aug_crop == 0). `aug` decides the mirror."""
        if self.aug_crop == 0.0 or not draw_crop(self.aug_seed, idx, self.aug_crop, text):
            return None
        box = crop_box(masks.get("obj_left"), masks.get("obj_right"), shape, flip=bool(aug and aug["flip"]))
        if box is None:
            self.crop_skipped += 1
        return box

    @classmethod
    def from_hf(cls, name, cfg, **kw):
        try:
            from datasets import load_dataset
        except ImportError as e:  # aff_dataset.py:108-113
            raise ImportError(f"'{name}' looks like a HuggingFace dataset id but the 'datasets' library is missing") from e
        return cls(load_dataset(name, split="train"), cfg, **kw)

    @classmethod
    def from_local(cls, base_image_dir, cfg, h5_open=None, **kw):
        """The local 2HANDS layout of `_load_from_local` / `extract_index_from_h5` (aff_dataset.py:152-183, 307-338):

            <dir>/h5/<start>-<end>_*.h5     group `data` with datasets `inpainted` [n, H, W, 3] uint8, `narration` [n] bytes,
                                            `taxonomy` [n]; a file holds the samples start..end (inclusive) of the global index
            <dir>/jsons/<start>-<end>_*.json  {"0": {"original_size": [h, w], "aff_left": [contours], "aff_right": [contours]}, ...}

        Everything the reference does with it is here: the json files are read in the order of the first number in their names
        and their entries appended in key order to ONE global list of contour masks (:160-183), `original_size` comes from entry
        "0" of the first file, the number of samples is the sum of the `inpainted` lengths, and sample i is fetched from the
        file whose name range contains i (:307-321) at row i - start. The one thing this image lacks is the HDF5 reader:
        `h5_open(path)` must return a mapping like `h5py.File(path, "r")`; left None it is h5py's, and its absence raises
        ImportError naming the dependency (h5py, any version that reads the files written by 2HANDS/scripts)."""
        import json
        import os
        import re
        if h5_open is None:
            try:
                import h5py
            except ImportError as e:
                raise ImportError("the local 2HANDS layout (<dir>/h5/*.h5 + <dir>/jsons/*.json, aff_dataset.py:152-183) is read "
                                  "through h5py, which is not installed here: `pip install h5py`, or pass h5_open=, or export "
                                  "the records and use AffRecordsDataset / from_hf") from e
            h5_open = lambda path: h5py.File(path, "r")   # noqa: E731
        image_dir, json_dir = os.path.join(base_image_dir, "h5"), os.path.join(base_image_dir, "jsons")

        def first_number(name):
            m = re.search(r"(\d+)", name)
            return int(m.group(1)) if m else float("inf")
        h5_names = [f for f in os.listdir(image_dir) if f.endswith(".h5")]
        ranges = []
        for f in h5_names:
            m = re.match(r"(\d+)-(\d+)_", f)
            if m:
                ranges.append((int(m.group(1)), int(m.group(2)), os.path.join(image_dir, f)))
        size = 0
        for f in h5_names:
            h = h5_open(os.path.join(image_dir, f))
            size += int(h["data"]["inpainted"].shape[0])
            if hasattr(h, "close"):
                h.close()
        masks_left, masks_right, original_size = [], [], None
        keep_objects = float(kw.get("aug_crop", 0.0)) > 0.0     # the object contours beside the affordance ones, only for the crop
        objs_left, objs_right = [], []
        for name in sorted(os.listdir(json_dir), key=first_number):
            with open(os.path.join(json_dir, name)) as fh:
                data = json.load(fh)
            if original_size is None:
                original_size = [int(x) for x in data["0"]["original_size"]]
            for key in data:
                masks_left.append(data[key].get("aff_left", []))
                masks_right.append(data[key].get("aff_right", []))
                if keep_objects:
                    objs_left.append(data[key].get("obj_left", []))
                    objs_right.append(data[key].get("obj_right", []))
        if len(masks_left) < size:
            raise ValueError(f"{size} samples in h5/ but contours for only {len(masks_left)} in jsons/")

        class _LocalRecords:
            """records[i] for AffRecordsDataset: fetched from the h5 file whose name range holds i (extract_index_from_h5)."""

            def __len__(self):
                return size

            def __getitem__(self, i):
                for lo, hi, path in ranges:
                    if lo <= i <= hi:
                        h = h5_open(path)
                        d = h["data"]
                        rec = {"narration": d["narration"][i - lo], "inpainted": np.asarray(d["inpainted"][i - lo]),
                               "taxonomy": d["taxonomy"][i - lo],
                               "masks": {"original_size": original_size, "aff_left": masks_left[i], "aff_right": masks_right[i]}}
                        if keep_objects:
                            rec["masks"]["obj_left"], rec["masks"]["obj_right"] = objs_left[i], objs_right[i]
                        if hasattr(h, "close"):
                            h.close()
                        return rec
                raise ValueError(f"Index {i} not found in any file in {image_dir}.")

            def __iter__(self):
                return (self[i] for i in range(size))
        ds = cls.__new__(cls)
        ds.records = _LocalRecords()
        ds.cfg, ds.samples_per_epoch, ds.inference = cfg, kw.get("samples_per_epoch", 500 * 8 * 2 * 10), kw.get("inference", False)
        ds.size, ds.original_size, ds.rng = size, tuple(original_size), random.Random(kw.get("seed"))
        ds._set_augmentation(kw.get("seed"), kw.get("aug_flip", 0.0), kw.get("aug_jitter", 0.0), kw.get("aug_crop", 0.0))
        return ds

    def __len__(self):
        return self.samples_per_epoch

    def __getitem__(self, idx):
        item = self.records[self.rng.randint(0, self.size - 1)]        # the reference draws a random sample per call
        text = item.get("narration", item.get("text", ""))
        if isinstance(text, bytes):
            text = text.decode("utf-8")
        image = np.array(item["image"] if "image" in item else item["inpainted"])
        if image.ndim == 2:
            image = np.stack([image] * 3, -1)
        image = np.ascontiguousarray(image[..., :3]).astype(np.uint8)
        taxonomy = _taxonomy_vector(item.get("taxonomy", 2))
        m = item.get("masks") or {}
        shape = tuple(int(x) for x in m.get("original_size", self.original_size or image.shape[:2]))
        left = recreate_mask_from_contours(m.get("aff_left", []), shape)
        right = recreate_mask_from_contours(m.get("aff_right", []), shape)
        aug = self._draw_aug(idx)
        box = self._draw_crop_box(idx, text, m, shape, aug)
        if box is not None:                 # flip -> crop -> jitter: the jitter's frame mean is the cropped frame's
            image, left, right, taxonomy = host_crop_sample(image, left, right, taxonomy, aug, box)
            if aug is not None and aug["jitter"] is not None:
                image = augment_frame(image, {"flip": False, "jitter": aug["jitter"]})
        elif aug is not None:               # before any resize; the masks are mirrored rasters, never fills of mirrored vertices
            image = augment_frame(image, aug)
            if aug["flip"]:
                left, right = np.ascontiguousarray(right[:, ::-1]), np.ascontiguousarray(left[:, ::-1])
                taxonomy = flip_taxonomy(taxonomy)
        label = {"left": torch.from_numpy((left == 0).astype(np.int64) * 255),
                 "right": torch.from_numpy((right == 0).astype(np.int64) * 255)}
        cfg = self.cfg
        image_clip = preprocess.clip_preprocess(torch.from_numpy(image.copy()), cfg.clip.image)
        resized = preprocess.resize_longest_side(torch.from_numpy(image.copy()), cfg.sam.img_size)
        resize = tuple(resized.shape[:2])
        image_t = preprocess.sam_preprocess(resized, cfg.sam.img_size)
        question = self.rng.choice(SHORT_QUESTION_LIST).format(class_name=text.lower())
        answer = self.rng.choice(ANSWER_LIST)
        conv = hprompt.default_conversation()
        conv.append_message(conv.roles[0], question)
        conv.append_message(conv.roles[1], answer)
        out = (None, image_t, image_clip, [conv.get_prompt()], torch.from_numpy(left).unsqueeze(0),
               torch.from_numpy(right).unsqueeze(0), taxonomy, label, resize, [question], [text])
        return out + (self.inference,)

    def raw_item(self, idx):
        """What train_ingest.DeviceIngest builds the sample from on the device: no resize, no normalised tensor, no filled mask, no
        label planes. Draws from self.rng in __getitem__'s order (record, then question, then answer), so a seeded run sees the
        same samples and prompts either way. With an augmentation probability set the dict also carries "aug" (draw_augmentation
        for this idx): what __getitem__ applies with Pillow, DeviceIngest applies on the device. With aug_crop set it carries "crop" too
        (crop_box of a sample that drew the crop, else None), and "crop_skipped" when the draw found no object."""
        item = self.records[self.rng.randint(0, self.size - 1)]
        text = item.get("narration", item.get("text", ""))
        if isinstance(text, bytes):
            text = text.decode("utf-8")
        image = np.array(item["image"] if "image" in item else item["inpainted"])
        if image.ndim == 2:
            image = np.stack([image] * 3, -1)
        image = np.ascontiguousarray(image[..., :3]).astype(np.uint8)
        m = item.get("masks") or {}
        shape = tuple(int(x) for x in m.get("original_size", self.original_size or image.shape[:2]))
        question = self.rng.choice(SHORT_QUESTION_LIST).format(class_name=text.lower())
        answer = self.rng.choice(ANSWER_LIST)
        conv = hprompt.default_conversation()
        conv.append_message(conv.roles[0], question)
        conv.append_message(conv.roles[1], answer)
        # the vertex lists as cvlite.draw_contours_filled reads them (int32 [n,2]): converted here, off the main thread
        left, right = ([np.asarray(c, dtype=np.int32).reshape(-1, 2) for c in m.get(k) or []] for k in ("aff_left", "aff_right"))
        raw = {"frame": image, "contours_left": left, "contours_right": right, "mask_hw": shape,
               "taxonomy": _taxonomy_vector(item.get("taxonomy", 2)), "conversations": [conv.get_prompt()],
               "questions": [question], "texts": [text], "inference": self.inference}
        aug = self._draw_aug(idx)
        if aug is not None:                 # applied by DeviceIngest; frame, contours and taxonomy are the record's own here
            raw["aug"] = aug
        if self.aug_crop > 0.0:             # the box of the (mirrored) object planes, or None: not drawn, or nothing to centre on
            skipped = self.crop_skipped
            raw["crop"] = self._draw_crop_box(idx, text, m, shape, aug)
            if self.crop_skipped != skipped:
                raw["crop_skipped"] = True
        return raw


class AffValDataset(torch.utils.data.Dataset):
    """AffDatasetVal (aff_dataset.py:350-544): the ActAffordance-style benchmark folders as validation samples."""

    def __init__(self, base_image_dir, cfg, seed=None, aug_flip=0.0, aug_jitter=0.0, aug_crop=0.0):
        # the validation set is never augmented: the training set's keywords are accepted and ignored
        self.cfg = cfg
        self.images, self.affs_left, self.affs_right, self.narrations, self.taxonomies = self.load_data_from_nested_folders(base_image_dir)
        self.size = len(self.images)
        self.rng = random.Random(seed)

    def __len__(self):
        return self.size

    @staticmethod
    def load_data_from_nested_folders(root_folder):
        """:457-544. Two directory levels; a leaf needs inpainting.png, annotation.json and at least one of aff_left.png /
        aff_right.png (the missing hand becomes zeros of the other's shape). Masks are read as 8-bit grayscale
        (cv2.imread(..., IMREAD_GRAYSCALE): identical to PIL's "L" for the single-channel PNGs the benchmark ships)."""
        import json
        import os
        from PIL import Image
        images, lefts, rights, narrations, taxonomies = [], [], [], [], []
        for l1 in os.listdir(root_folder):
            p1 = os.path.join(root_folder, l1)
            if not os.path.isdir(p1):
                continue
            for l2 in os.listdir(p1):
                p2 = os.path.join(p1, l2)
                if not os.path.isdir(p2):
                    continue
                files = set(os.listdir(p2))
                has_l, has_r = "aff_left.png" in files, "aff_right.png" in files
                if "inpainting.png" not in files or "annotation.json" not in files or not (has_l or has_r):
                    continue
                images.append(np.array(Image.open(os.path.join(p2, "inpainting.png"))))
                left = np.array(Image.open(os.path.join(p2, "aff_left.png")).convert("L")) if has_l else None
                right = np.array(Image.open(os.path.join(p2, "aff_right.png")).convert("L")) if has_r else None
                lefts.append(left if left is not None else np.zeros_like(right))
                rights.append(right if right is not None else np.zeros_like(left))
                with open(os.path.join(p2, "annotation.json")) as f:
                    ann = json.load(f)
                narrations.append(ann.get("narration", ""))
                taxonomies.append(ann.get("taxonomy", ""))
        return images, lefts, rights, narrations, taxonomies

    def __getitem__(self, idx):
        idx = self.rng.randint(0, self.size - 1)                         # :394 — the reference draws a random sample here too
        text, image, taxonomy = self.narrations[idx], self.images[idx], self.taxonomies[idx]
        if image.ndim == 2:
            image = np.stack([image] * 3, -1)
        image = np.ascontiguousarray(image[..., :3]).astype(np.uint8)
        left, right = self.affs_left[idx], self.affs_right[idx]
        label = {"left": torch.from_numpy((left == 0).astype(np.int64) * 255),
                 "right": torch.from_numpy((right == 0).astype(np.int64) * 255)}
        cfg = self.cfg
        image_clip = preprocess.clip_preprocess(torch.from_numpy(image.copy()), cfg.clip.image)
        resized = preprocess.resize_longest_side(torch.from_numpy(image.copy()), cfg.sam.img_size)
        resize = tuple(resized.shape[:2])
        image_t = preprocess.sam_preprocess(resized, cfg.sam.img_size)
        question = self.rng.choice(SHORT_QUESTION_LIST).format(class_name=text.lower())
        answer = self.rng.choice(ANSWER_LIST)
        conv = hprompt.default_conversation()
        conv.append_message(conv.roles[0], question)
        conv.append_message(conv.roles[1], answer)
        return (None, image_t, image_clip, [conv.get_prompt()], torch.from_numpy(left).unsqueeze(0),
                torch.from_numpy(right).unsqueeze(0), taxonomy, label, resize, [question], [text], True)

    def raw_item(self, idx):
        """AffRecordsDataset.raw_item for the benchmark folders: the ground truth is the PNG planes themselves. Same rng order as
        __getitem__ (sample, then question, then answer)."""
        idx = self.rng.randint(0, self.size - 1)
        text, image, taxonomy = self.narrations[idx], self.images[idx], self.taxonomies[idx]
        if image.ndim == 2:
            image = np.stack([image] * 3, -1)
        image = np.ascontiguousarray(image[..., :3]).astype(np.uint8)
        left, right = self.affs_left[idx], self.affs_right[idx]
        question = self.rng.choice(SHORT_QUESTION_LIST).format(class_name=text.lower())
        answer = self.rng.choice(ANSWER_LIST)
        conv = hprompt.default_conversation()
        conv.append_message(conv.roles[0], question)
        conv.append_message(conv.roles[1], answer)
        return {"frame": image, "plane_left": left, "plane_right": right, "mask_hw": tuple(left.shape), "taxonomy": taxonomy,
                "conversations": [conv.get_prompt()], "questions": [question], "texts": [text], "inference": True}
