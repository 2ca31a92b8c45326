"""Building the 2HANDS training set from hand masks and completed object masks: the step in front of `train_ds.py --sam_records`.

The reference does it in three scripts; each is a subcommand here, with its arguments, and `build` runs the whole chain:

  extract_affordances COMPLETED HAND OUT   2HANDS/scripts/affordance_extraction_preparation.py --extract_affordances (and, with OUT ==
                                           COMPLETED, misc/determine_mask_overlap.py): for left/ and right/, files matched by name, the
                                           hand mask padded to a square, resized nearest to the completed mask, cv2.bitwise_and, a PNG.
  process_affordances DIR K                --process_affordances, in place: empty masks deleted, the rest dilated with a K x K
                                           rectangle and every non-zero pixel recoloured to 255.
  create_dataset --dir --out --name ...    2HANDS/scripts/create_dataset.py: is_valid / check_threshold over the sequence folders
                                           (annotation.json, inpainted_frame.png, aff_/obj_{left,right}.png), then
                                           compress_masks_to_json.convert_masks_to_json: <out>/jsons/<name>.json, and
                                           <out>/records/<name>.pt, the list `train_ds.py --sam_records` loads as it stands.
  build --completed C --hand H --objects O --sequences S --k K --out --name ...
                                           the three in one pass, no intermediate PNG. The tree (the reference's pipeline.bash
                                           assembles its own with steps that are commented out there, so the layout is defined HERE):
                                             C/left/<seq>.png  C/right/<seq>.png   completed object masks (extract's first argument)
                                             H/left/<seq>.png  H/right/<seq>.png   hand masks (extract's second argument)
                                             O/left/<seq>.png  O/right/<seq>.png   object masks: the sequence's obj_left / obj_right
                                             S/<seq>/annotation.json  S/<seq>/inpainted_frame.png
                                           A sequence has aff_<side>.png when C/<side>/<seq>.png and H/<side>/<seq>.png both exist and
                                           their AND is not empty (process_affordances deletes an empty one), and obj_<side>.png when
                                           O/<side>/<seq>.png exists; from there on it is create_dataset on those virtual files.

--route device (default) runs the mask arithmetic in HIP (ops.affordance_extract, csrc/affordance_extract.hip) and the contours in
HIP (contours.ContourReader); --route host runs cvlite. Both write the same files byte for byte. Per batch `build` makes one
affordance_extract call for the affordance planes, one statistics-only call for the object planes and one ContourReader.read over
the four planes of the kept sequences. On the device route a plane past the kernel's limits (a side over 4096) goes through cvlite
and is counted in `host_extracts`, as is an AND plane of grey values other than 0 / 255 in extract_affordances (the kernel writes the
recoloured plane, the file holds the grey values); ContourReader.host_walks counts its own. The CLI prints both when non-zero.

Record: {"narration", "image" (the frame as PIL loads it, RGB), "taxonomy" (the annotation's 4-vector), "noun", "verb", "obj_id_left",
"obj_id_right", "masks": {"original_size": (H, W), "aff_left", "aff_right", "obj_left", "obj_right"}}; a missing hand is [].

Deviations from the reference, all deliberate:
  * folders and files are visited in sorted order (os.listdir's order is unspecified);
  * a sequence whose object mask is all zero is counted invalid (`empty_object`; the reference raises at min() of an empty array),
    and so is one with an affordance mask but no object mask of that hand (`missing_object`; the reference raises there too);
  * mask files are read through PIL convert("L"): cv2.imread(IMREAD_GRAYSCALE)'s value for grey files and for RGB files with equal
    channels (both weightings sum to one); for coloured masks it is not, and that stays unpinned;
  * the h5 file is not written (h5py is not available here): records/<name>.pt carries what it held;
  * `white` of check_threshold is sum / 255 of the grey plane in Python floats: the reference divides the three-channel sum by 765,
    the same double for equal channels.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

from . import cvlite

SIDES = ("left", "right")
INVALID_VERB_CLASSES = ("eat", "look", "search", "feel", "transition", "wait", "smell", "finish", "unfreeze")
PHASES = ("decode", "kernels", "contours", "writes")


def read_grey(path):
    from PIL import Image
    return np.array(Image.open(path).convert("L"))


def write_png(path, plane):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(plane)).save(path)


class _Route:
    """The primitive both routes share: run(items, k, want_out) over items = [(plane, hand or None)] (numpy uint8) returns per item
    (handle of the dilated and recoloured plane or None, the eight statistics words of ops.AFF_EXTRACT_STATS); contours(handles) the
    external contours of each; to_numpy(handle) the plane. Everything above it is route-independent code."""
    name = None

    def __init__(self):
        self.host_extracts, self.host_walks = 0, 0
        self.seconds = dict.fromkeys(PHASES, 0.0)

    def timed(self, phase):
        return _Timer(self, phase)

    @staticmethod
    def host_item(plane, hand, k):
        a = plane if hand is None else cvlite.extract_affordance(plane, hand)
        out = np.where(cvlite.dilate_rect(a, k) != 0, 255, 0).astype(np.uint8)
        ys, xs = np.nonzero(out)
        box = [int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())] if len(ys) else [a.shape[0], -1, a.shape[1], -1]
        grey = bool(((a != 0) & (a != 255)).any())
        stats = [int(np.count_nonzero(a)), int(len(ys)), int(a.sum(dtype=np.int64))] + box + [(1 if hand is not None else 0) | (2 if grey else 0)]
        return out, stats


class _Timer:
    def __init__(self, route, phase):
        self.route, self.phase = route, phase

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        self.route.sync()
        self.route.seconds[self.phase] += time.perf_counter() - self.t0


class HostRoute(_Route):
    name = "host"

    def sync(self):
        pass

    def run(self, items, k, want_out=True):
        res = [self.host_item(p, h, k) for p, h in items]
        return [(o if want_out else None, s) for o, s in res]

    def contours(self, handles):
        return [cvlite.find_contours_external(h) for h in handles]

    def to_numpy(self, handle):
        return handle


class DeviceRoute(_Route):
    name = "device"

    def __init__(self, device="cuda:0"):
        super().__init__()
        import torch
        from . import contours, ops
        self.torch, self.ops, self.device = torch, ops, torch.device(device)
        self.reader = contours.ContourReader()
        self.tables = {}

    def sync(self):
        self.torch.cuda.synchronize(self.device)

    def _tables(self, hand_hw, out_hw):
        key = (tuple(hand_hw), tuple(out_hw))
        if key not in self.tables:
            self.tables[key] = self.ops.nearest_pad_tables(hand_hw, out_hw, device=self.device)
        return self.tables[key]

    def run(self, items, k, want_out=True):
        torch = self.torch
        res, call, where = [None] * len(items), [], []
        for i, (plane, hand) in enumerate(items):
            if max(plane.shape + (hand.shape if hand is not None else ())) > self.ops.AFF_EXTRACT_MAX_SIDE:
                self.host_extracts += 1                       # past the kernel's limits: cvlite, counted
                out, stats = self.host_item(plane, hand, k)
                res[i] = (torch.from_numpy(out).to(self.device) if want_out else None, stats)
                continue
            p = torch.from_numpy(np.ascontiguousarray(plane)).to(self.device)
            h = None if hand is None else torch.from_numpy(np.ascontiguousarray(hand)).to(self.device)
            t = None if hand is None else self._tables(hand.shape, plane.shape)
            out = torch.empty_like(p) if want_out else None
            call.append((p, h, t, out))
            where.append(i)
        if call:
            stats = self.ops.affordance_extract(call, k).cpu().tolist()       # the one synchronisation
            for i, c, s in zip(where, call, stats):
                res[i] = (c[3], s)
        return res

    def contours(self, handles):
        from .contours import host_walk
        max_side = self.ops.HAUSDORFF_MAX_SIDE                # ops.contour_extract's
        small = [h for h in handles if max(h.shape) <= max_side]
        found = iter(self.reader.read(small)) if small else iter(())
        out = []
        for h in handles:
            if max(h.shape) <= max_side:
                out.append(next(found))
            else:
                out.append(host_walk(self.reader, cvlite.find_contours_external, h))
        self.host_walks = self.reader.host_walks
        return out

    def to_numpy(self, handle):
        return handle.cpu().numpy()


def make_route(name, device="cuda:0"):
    if name == "host":
        return HostRoute()
    if name == "device":
        return DeviceRoute(device)
    raise ValueError(f"--route is device or host, not {name!r}")


def _batches(seq, n):
    for i in range(0, len(seq), n):
        yield seq[i:i + n]


# ---- extract_affordances / process_affordances ------------------------------------------------------------------------------------

def extract_affordances(completed_dir, hand_dir, out_dir, route, batch=64, log=print):
    """affordance_extraction_preparation.py:256-296. Returns the number of PNGs written."""
    written = 0
    for side in SIDES:
        c_sub, h_sub, o_sub = (os.path.join(d, side) for d in (completed_dir, hand_dir, out_dir))
        os.makedirs(o_sub, exist_ok=True)
        for names in _batches(sorted(os.listdir(c_sub)), batch):
            todo = []
            with route.timed("decode"):
                for name in names:
                    hand_path = os.path.join(h_sub, name)
                    if not os.path.isfile(hand_path):
                        log(f"Skipping {name}: No corresponding file in {h_sub}")
                        continue
                    try:
                        completed, hand = read_grey(os.path.join(c_sub, name)), read_grey(hand_path)
                    except (OSError, ValueError):
                        log(f"Skipping {name}: Could not read one or both masks.")
                        continue
                    if completed.shape != (max(hand.shape),) * 2:
                        log(f"Resizing {name} to match dimensions of {hand_path}.")
                    todo.append((name, completed, hand))
            if not todo:
                continue
            with route.timed("kernels"):
                res = route.run([(c, h) for _, c, h in todo], 1)
            with route.timed("writes"):
                for (name, completed, hand), (out, stats) in zip(todo, res):
                    if stats[7] & 2:                          # grey values other than 0 / 255: the file holds them, not the recolour
                        if route.name == "device":
                            route.host_extracts += 1
                        plane = cvlite.extract_affordance(completed, hand)
                    else:
                        plane = route.to_numpy(out)
                    path = os.path.join(o_sub, name)
                    write_png(path, plane)
                    log(f"Updated mask saved: {path}")
                    written += 1
    return written


def process_affordances(directory, k, route, batch=64):
    """affordance_extraction_preparation.py:298-304, in place. Returns (deleted, kept)."""
    deleted = kept = 0
    for side in SIDES:
        sub = os.path.join(directory, side)
        for names in _batches(sorted(os.listdir(sub)), batch):
            with route.timed("decode"):
                planes = [read_grey(os.path.join(sub, name)) for name in names]
            with route.timed("kernels"):
                res = route.run([(p, None) for p in planes], k)
            with route.timed("writes"):
                for name, (out, stats) in zip(names, res):
                    path = os.path.join(sub, name)
                    if stats[0] == 0:                         # delete_empty_masks: tested before the dilation
                        os.remove(path)
                        deleted += 1
                    else:
                        write_png(path, route.to_numpy(out))
                        kept += 1
    return deleted, kept


# ---- create_dataset -----------------------------------------------------------------------------------------------------------------

def extract_verb_class_dict(verb_class_file):
    with open(verb_class_file) as fh:
        return list(csv.DictReader(fh))


def map_verb_to_class(verb, verb_classes, log=print):
    """create_dataset.py:19-26: the first row whose raw `instances` FIELD contains the verb, a substring test on the CSV string."""
    for row in verb_classes:
        if verb in row["instances"]:
            return row["key"]
    log("Verb not found")
    return ""


def check_threshold(sum_of_values, limit):
    """create_dataset.py:104-114 on the grey plane: white = sum / 255 in Python floats, valid when 20 < white < limit."""
    white = sum_of_values / 255
    return white < limit and white > 20, white


def is_valid(files, annotation, white_sums, limit, categories, verb_classes, log=print):
    """create_dataset.py:28-102, rule for rule, on a sequence's file names, its annotation and white_sums = {"left": sum of the grey
    values of aff_left.png, ...} for the affordance files that exist. Returns (valid, reason)."""
    if "annotation.json" not in files or "inpainted_frame.png" not in files:
        return False, "missing_file"
    data = annotation
    taxonomy = data["taxonomy"]
    if data["noun"] is None or data["verb"] is None or data["narration"] is None:
        return False, "null_annotation"
    verb_class = map_verb_to_class(data["verb"], verb_classes, log)
    if verb_class == "" or verb_class in INVALID_VERB_CLASSES:
        log("found invalid verb_class: ", verb_class)
        return False, "verb_class"
    has = {s: f"aff_{s}.png" in files and f"obj_{s}.png" in files for s in SIDES}
    if taxonomy[0] == 0:                                      # the bimanual case
        if not (has["left"] and has["right"]):
            return False, "missing_file"
        if data["obj_left"] not in categories and data["obj_right"] not in categories and "all" not in categories:
            return False, "category"
        ok_left, ok_right = check_threshold(white_sums["left"], limit)[0], check_threshold(white_sums["right"], limit)[0]
        return (True, "valid") if ok_left and ok_right else (False, "threshold")
    if not (has["left"] or has["right"]):
        return False, "missing_file"
    side = "left" if has["left"] else "right"                 # the left hand alone when the left pair exists
    if data[f"obj_{side}"] not in categories and "all" not in categories:
        return False, "category"
    return (True, "valid") if check_threshold(white_sums[side], limit)[0] else (False, "threshold")


class _Sequence:
    """One sequence folder as create_dataset sees it: the file names it 'has', its annotation and frame path, and per hand the
    affordance / object planes as route handles (filled by the caller)."""

    def __init__(self, name, files, annotation, frame_path):
        self.name, self.files, self.annotation, self.frame_path = name, set(files), annotation, frame_path
        self.aff, self.obj, self.white, self.obj_nonzero = {}, {}, {}, {}


def _load_annotation(path):
    with open(path) as fh:
        return json.load(fh)


def _finish(seqs, route, limit, categories, verb_classes, log, records, entries, reasons):
    """validity, object checks, contours and packing of one batch of _Sequence: appends to records / entries, counts in reasons"""
    kept = []
    for s in seqs:
        ok, why = is_valid(s.files, s.annotation, s.white, limit, categories, verb_classes, log)
        if ok:
            for side in SIDES:                                # what the reference reads (and raises on) for a valid sequence
                if f"aff_{side}.png" in s.files:
                    if side not in s.obj:
                        ok, why = False, "missing_object"
                    elif s.obj_nonzero[side] == 0:
                        ok, why = False, "empty_object"
        reasons[why] = reasons.get(why, 0) + 1
        if ok:
            kept.append(s)
    if not kept:
        return
    handles, slots = [], []
    for i, s in enumerate(kept):
        for key, planes in (("aff", s.aff), ("obj", s.obj)):
            for side in SIDES:
                if f"aff_{side}.png" in s.files:              # a hand without an affordance file is zeros in the reference: []
                    handles.append(planes[side])
                    slots.append((i, f"{key}_{side}"))
    with route.timed("contours"):
        found = route.contours(handles)
    lists = [{f"{key}_{side}": [] for key in ("aff", "obj") for side in SIDES} for _ in kept]
    for (i, slot), c in zip(slots, found):
        lists[i][slot] = [np.asarray(x).reshape(-1, 2).tolist() for x in c]
    from PIL import Image
    with route.timed("decode"):
        frames = [np.asarray(Image.open(s.frame_path).convert("RGB")) for s in kept]
    for s, m, frame in zip(kept, lists, frames):
        side = "left" if "aff_left.png" in s.files else "right"
        size = tuple(int(v) for v in s.aff[side].shape)
        ann = s.annotation
        entries.append({"original_size": size, "aff_left": m["aff_left"], "aff_right": m["aff_right"], "obj_left": m["obj_left"],
                        "obj_right": m["obj_right"]})
        records.append({"narration": ann["narration"], "image": frame, "taxonomy": list(ann["taxonomy"]), "noun": ann["noun"],
                        "verb": ann["verb"], "obj_id_left": ann["obj_left"] if ann.get("obj_left") is not None else "",
                        "obj_id_right": ann["obj_right"] if ann.get("obj_right") is not None else "",
                        "masks": dict(entries[-1])})


def _write_dataset(out, name, records, entries, reasons, route, log):
    import torch
    with route.timed("writes"):
        os.makedirs(os.path.join(out, "jsons"), exist_ok=True)
        os.makedirs(os.path.join(out, "records"), exist_ok=True)
        with open(os.path.join(out, "jsons", name + ".json"), "w") as fh:
            json.dump({i: e for i, e in enumerate(entries)}, fh)                # convert_masks_to_json's structure, int keys dumped
        torch.save(list(records), os.path.join(out, "records", name + ".pt"))
    valid = reasons.get("valid", 0)
    invalid = sum(reasons.values()) - valid
    log("Valid Frames Total: ", valid)
    log("Invalid Frames Total: ", invalid)
    if valid + invalid:
        log(str(round(valid / (invalid + valid) * 100, 2)) + "% were valid frames")
    return {"valid": valid, "invalid": invalid, "reasons": dict(sorted(reasons.items()))}


def create_dataset(directory, out, name, limit, categories, verb_class_file, route, batch=64, log=print):
    """create_dataset.py:116-215 over the sequence folders of `directory` (sorted)."""
    verb_classes = extract_verb_class_dict(verb_class_file)
    records, entries, reasons = [], [], {}
    folders = [f for f in sorted(os.listdir(directory)) if os.path.isdir(os.path.join(directory, f))]
    for names in _batches(folders, batch):
        seqs, aff_items, obj_items = [], [], []
        with route.timed("decode"):
            for folder in names:
                path = os.path.join(directory, folder)
                files = set(os.listdir(path))
                ann = _load_annotation(os.path.join(path, "annotation.json")) if "annotation.json" in files else None
                s = _Sequence(folder, files, ann, os.path.join(path, "inpainted_frame.png"))
                for side in SIDES:
                    if f"aff_{side}.png" in files:
                        aff_items.append((s, side, read_grey(os.path.join(path, f"aff_{side}.png"))))
                    if f"obj_{side}.png" in files:
                        obj_items.append((s, side, read_grey(os.path.join(path, f"obj_{side}.png"))))
                seqs.append(s)
        with route.timed("kernels"):
            # k = 1: the plane recoloured (the contours see `!= 0` either way) and, in word 2, the sum check_threshold wants
            aff_res = route.run([(p, None) for _, _, p in aff_items], 1) if aff_items else []
            obj_res = route.run([(p, None) for _, _, p in obj_items], 1) if obj_items else []
        for (s, side, _), (handle, stats) in zip(aff_items, aff_res):
            s.aff[side], s.white[side] = handle, stats[2]
        for (s, side, _), (handle, stats) in zip(obj_items, obj_res):
            s.obj[side], s.obj_nonzero[side] = handle, stats[0]
        _finish(seqs, route, limit, categories, verb_classes, log, records, entries, reasons)
    return _write_dataset(out, name, records, entries, reasons, route, log)


def build(completed, hand, objects, sequences, k, out, name, limit, categories, verb_class_file, route, batch=64, log=print):
    """extract_affordances, process_affordances and create_dataset in one pass over the tree of the module docstring."""
    verb_classes = extract_verb_class_dict(verb_class_file)
    records, entries, reasons = [], [], {}
    folders = [f for f in sorted(os.listdir(sequences)) if os.path.isdir(os.path.join(sequences, f))]
    for names in _batches(folders, batch):
        seqs, aff_items, obj_items = [], [], []
        with route.timed("decode"):
            for folder in names:
                path = os.path.join(sequences, folder)
                files = set(os.listdir(path)) & {"annotation.json", "inpainted_frame.png"}
                ann = _load_annotation(os.path.join(path, "annotation.json")) if "annotation.json" in files else None
                s = _Sequence(folder, files, ann, os.path.join(path, "inpainted_frame.png"))
                for side in SIDES:
                    c, h, o = (os.path.join(d, side, folder + ".png") for d in (completed, hand, objects))
                    if os.path.isfile(c) and os.path.isfile(h):
                        aff_items.append((s, side, read_grey(c), read_grey(h)))
                    if os.path.isfile(o):
                        obj_items.append((s, side, read_grey(o)))
                seqs.append(s)
        with route.timed("kernels"):
            aff_res = route.run([(c, h) for _, _, c, h in aff_items], k) if aff_items else []
            obj_res = route.run([(p, None) for _, _, p in obj_items], 1) if obj_items else []     # (the planes stay for the contours)
        for (s, side, _, _), (handle, stats) in zip(aff_items, aff_res):
            if stats[0] == 0:
                continue                                      # empty after the AND: process_affordances deletes the file
            s.files.add(f"aff_{side}.png")
            s.aff[side], s.white[side] = handle, 255 * stats[1]     # the file would hold 255 on every pixel of `out`
        for (s, side, _), (handle, stats) in zip(obj_items, obj_res):
            s.files.add(f"obj_{side}.png")
            s.obj[side], s.obj_nonzero[side] = handle, stats[0]
        _finish(seqs, route, limit, categories, verb_classes, log, records, entries, reasons)
    return _write_dataset(out, name, records, entries, reasons, route, log)


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------

def make_parser():
    parser = argparse.ArgumentParser(prog="python -m 2handedafforder_amd.dataset_build", description=__doc__.split("\n\n")[0])
    sub = parser.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--route", default="device", choices=("device", "host"), help="HIP kernels (default) or cvlite on the host")
        p.add_argument("--batch", default=64, type=int, help="files / sequences per kernel call")

    def dataset(p):
        p.add_argument("--out", required=True)
        p.add_argument("--name", required=True)
        p.add_argument("--limit", default=30000, type=float)
        p.add_argument("--categories", default=[], nargs="+")
        p.add_argument("--verb-class-file", required=True, help="EPIC_100_verb_classes.csv (columns id, key, instances)")

    p = sub.add_parser("extract_affordances", help="AND of completed masks and hand masks")
    p.add_argument("completed")
    p.add_argument("hand")
    p.add_argument("out")
    common(p)
    p = sub.add_parser("process_affordances", help="delete empty masks, dilate, recolour; in place")
    p.add_argument("dir")
    p.add_argument("k", type=int)
    common(p)
    p = sub.add_parser("create_dataset", help="validity rules, contours, jsons/ and records/")
    p.add_argument("--dir", required=True)
    dataset(p)
    common(p)
    p = sub.add_parser("build", help="the whole chain without intermediate PNGs")
    for flag in ("--completed", "--hand", "--objects", "--sequences"):
        p.add_argument(flag, required=True)
    p.add_argument("--k", required=True, type=int)
    dataset(p)
    common(p)
    return parser


def main(argv=None):
    args = make_parser().parse_args(argv)
    if getattr(args, "k", 1) < 1 or getattr(args, "k", 1) > 31:
        raise SystemExit("the dilation factor is 1..31")
    if args.batch < 1:
        raise SystemExit("--batch is at least 1")
    route = make_route(args.route)
    if args.command == "extract_affordances":
        extract_affordances(args.completed, args.hand, args.out, route, args.batch)
    elif args.command == "process_affordances":
        deleted, kept = process_affordances(args.dir, args.k, route, args.batch)
        print(f"{args.dir}: {deleted} empty masks deleted, {kept} dilated by {args.k} and recoloured")
    elif args.command == "create_dataset":
        create_dataset(args.dir, args.out, args.name, args.limit, args.categories, args.verb_class_file, route, args.batch)
    else:
        build(args.completed, args.hand, args.objects, args.sequences, args.k, args.out, args.name, args.limit, args.categories,
              args.verb_class_file, route, args.batch)
    if args.command in ("create_dataset", "build"):
        print(f"{os.path.join(args.out, 'records', args.name + '.pt')}: loads with train_ds.py --sam_records; the h5 file is not "
              "written (no h5py here)")
    if route.host_extracts:
        print(f"host_extracts: {route.host_extracts} planes went through cvlite")
    if route.host_walks:
        print(f"host_walks: {route.host_walks} planes were walked on the host")
    return 0


if __name__ == "__main__":
    sys.exit(main())
