"""Predicted masks as 2HANDS contour records: the writing side of the format aff_dataset.AffRecordsDataset reads.

The reference writes it with `cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)` over every mask, every contour kept
(2HANDS/scripts/utils/compress_masks_to_json.py:60-92, called from create_dataset.py:207). Here the contours come from the device
(ops.contour_extract, csrc/contour_hausdorff.hip): ContourReader reads back two small tables and the used vertex prefixes, and
recomputes on the host (cvlite.find_contours_external) only a plane the kernel flagged.
"""
import numpy as np
import torch

from . import cvlite, ops


def host_walk(counter, walk, *planes):
    """The one rule for planes the device flagged or does not take: counted in counter.host_walks, read back, walked on the host."""
    counter.host_walks += 1
    return walk(*(p.cpu().numpy() for p in planes))


class ContourReader:
    """read(planes) -> per plane the list of int32 [n, 1, 2] arrays `cvlite.find_contours_external(plane)` returns, element for
    element. planes: uint8 CUDA tensors [H, W] (a list, or one [n, H, W] tensor), on where != 0. max_contours / max_vertices are
    the device buffers' capacities per plane; a plane past either (or with the kernel's fault flag) is read back whole and walked on
    the host, and counted in `host_walks`."""

    def __init__(self, max_contours=1024, max_vertices=65536):
        self.max_contours, self.max_vertices = int(max_contours), int(max_vertices)
        if self.max_contours < 1 or self.max_vertices < 1:
            raise ValueError("max_contours and max_vertices are capacities of at least 1")
        self.host_walks = 0

    def read(self, planes):
        planes = list(planes)
        if not planes:
            return []
        summary, offsets, verts = ops.contour_extract(planes, self.max_contours, self.max_vertices)
        summary = summary.cpu().numpy()                          # the one synchronisation
        out = []
        for i, plane in enumerate(planes):
            n_contours, n_vertices, flags = (int(v) for v in summary[i, :3])
            if flags:
                out.append(host_walk(self, cvlite.find_contours_external, plane))
                continue
            if n_contours == 0:
                out.append([])
                continue
            offs = offsets[i, :n_contours + 1].cpu().numpy()
            pts = verts[i, :n_vertices].cpu().numpy().astype(np.int32)
            out.append([pts[offs[k]:offs[k + 1]].reshape(-1, 1, 2) for k in range(n_contours)])
        return out


def contour_lists(contours):
    """find_contours_external's arrays as plain [[x, y], ...] lists: what a record and a JSON file hold."""
    return [np.asarray(c).reshape(-1, 2).tolist() for c in contours]


def prediction_record(narration, image_u8, taxonomy_index, planes_left, planes_right, original_size):
    """One record as AffRecordsDataset consumes it. planes_left / planes_right: the hand's contours as ContourReader.read returns
    them for its plane ([] for a hand the taxonomy gate closed); taxonomy_index: the predicted class; original_size: (H0, W0)."""
    return {"narration": narration, "image": np.asarray(image_u8), "taxonomy": int(taxonomy_index),
            "masks": {"original_size": (int(original_size[0]), int(original_size[1])),
                      "aff_left": contour_lists(planes_left), "aff_right": contour_lists(planes_right)}}


def save_records(path, records):
    """What `train_ds.py --sam_records PATH` loads as it stands."""
    torch.save(list(records), path)
