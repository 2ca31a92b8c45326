"""Expected values and fixtures of the device contour extraction (csrc/contour_hausdorff.hip haff_contour_extract,
ops.contour_extract, haff.contours).

The expectation is `cvlite.find_contours_external(m)`, the host route as it stands, flattened into the kernel's three output arrays;
everything is an integer, so every comparison against the device is exact equality. Two facts about that list are restated here from
scipy.ndimage.label, independent of the walk: which pixels start a contour and in which order (the kernel's start rule), and that
filling the contours gives the plane with its holes filled (what a record round-trips to).
"""
import numpy as np

from haff import cvlite

import hausdorff_ref as R

TILE = R.TILE
OVERFLOW, FAULT, TOO_MANY = 1, 2, 4


def contours(m):
    return cvlite.find_contours_external(np.asarray(m).astype(np.uint8))


def expected(m):
    """(summary int32 [4], offsets int32 [n_contours + 1], verts int16 [n_vertices, 2]) the device writes for plane m when both
    capacities suffice."""
    c = contours(m)
    lens = [len(x) for x in c]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    verts = np.concatenate([x.reshape(-1, 2) for x in c]).astype(np.int16) if c else np.zeros((0, 2), np.int16)
    return np.array([len(c), int(offsets[-1]), 0, 0], np.int32), offsets, verts


def starts_by_rule(m):
    """The start rule from scipy.ndimage.label: the raster-first pixels (x, y) of the 8-connected foreground components whose
    raster-first pixel has x == 0 or a left neighbour in the outside background, in DESCENDING raster order."""
    from scipy import ndimage
    fg = np.pad(np.asarray(m) != 0, 1)
    comp, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    back, _ = ndimage.label(~fg)                               # 4-connected by default
    outside = back == back[0, 0]
    flat = comp.reshape(-1)
    idx = np.flatnonzero(flat)
    _, first = np.unique(flat[idx], return_index=True)
    roots = idx[first]                                         # raster-first pixel of every component, padded raster index
    w = fg.shape[1]
    keep = [int(r) for r in roots if outside.reshape(-1)[r - 1]]   # x == 0 unpadded: the left neighbour is the ring
    return [(r % w - 1, r // w - 1) for r in sorted(keep, reverse=True)]


def holes_filled(m):
    """~outside background: the plane with every hole (and everything inside it) filled."""
    return (~cvlite._outside_background(np.asarray(m) != 0))[1:-1, 1:-1].astype(np.uint8)


# ---- fixtures beyond hausdorff_ref's --------------------------------------------------------------------------------------------

def _z(h, w):
    return np.zeros((h, w), np.uint8)


def nested():
    """A ring, an island in its hole, that island's own hole, and a blob inside that: one external contour."""
    m = _z(21, 23)
    m[1:20, 1:22] = 1
    m[3:18, 3:20] = 0
    m[5:16, 5:18] = 1          # the island in the hole: not external
    m[7:14, 7:16] = 0
    m[9:12, 9:13] = 1          # inside the island's hole: not external either
    return m


def four_edges():
    """One component on each frame edge (the left one's root at x == 0, another rooted at (0, 0)'s row), one free in the middle."""
    m = _z(20, 24)
    m[0, 5:9] = 1              # top edge
    m[8:12, 0] = 1             # left edge, root at x == 0
    m[8:12, 23] = 1            # right edge
    m[19, 10:15] = 1           # bottom edge
    m[9:11, 10:13] = 1
    return m


def corners():
    m = _z(6, 7)
    m[0, 0] = m[0, 6] = m[5, 0] = m[5, 6] = 1
    return m


def seam_pair():
    """Two bars that meet only across the tile seam x = TILE - 1 | TILE (one component), and two that stop one pixel short of
    meeting across the seam y = TILE - 1 | TILE (two components)."""
    t = TILE
    m = _z(2 * t + 5, 2 * t + 3)
    m[4, t - 6:t] = 1
    m[4, t:t + 6] = 1
    m[t - 4:t - 1, 10] = 1
    m[t:t + 4, 10] = 1
    return m


def seam_diagonal():
    """Two pixels that are diagonal neighbours across the corner of four tiles, and two inside a tile: one component each pair."""
    t = TILE
    m = _z(2 * t, 2 * t)
    m[t - 1, t - 1] = m[t, t] = 1
    m[t - 1, t + 5] = m[t, t + 4] = 1          # the anti-diagonal across the horizontal seam
    m[5, 5] = m[6, 6] = 1
    return m


def isolated_grid():
    """64 x 64, a pixel on every other row and column: 1024 one-vertex contours."""
    m = _z(64, 64)
    m[::2, ::2] = 1
    return m


def over_lds():
    """1025 x 1024 (one row over the 2^20 pixels the walk holds in LDS): three small blobs, far apart."""
    m = _z(1025, 1024)
    m[3:9, 5:12] = 1
    m[500:520, 1000:1024] = 1
    m[510:515, 1005:1010] = 0                  # with a hole
    m[1024, 0:3] = 1
    m[1022:1024, 2] = 1
    return m


def new_planes():
    """name -> plane: the fixtures of this file."""
    p = {"nested": nested(), "four_edges": four_edges(), "corners": corners(), "seam_pair": seam_pair(),
         "seam_diagonal": seam_diagonal(), "isolated_grid": isolated_grid(), "empty": _z(9, 11), "full": np.ones((9, 11), np.uint8),
         "full_tile": np.ones((TILE + 1, 2 * TILE + 1), np.uint8), "over_lds": over_lds()}
    p["nested_255"] = nested() * 255           # on is != 0, not == 1
    return p


def device_planes():
    """(name, plane) of the one mixed-shape device call: this file's fixtures, then hausdorff_ref's small, random, wide and real
    planes."""
    out = list(new_planes().items())
    out += list(R.small_planes().items())
    out += [(f"noise{k}", m) for k, m in enumerate(R.random_planes())]
    out += [("wide_both", R.wide_planes()[0]), ("wide_first", R.wide_planes()[1])]
    out += [("real_left", R.real_pair()[0]), ("real_right", R.real_pair()[1])]
    return out


def cpu_planes():
    """(name, plane) for the two CPU facts: everything above but the 855 x 855 pair (the host walk of those takes seconds), plus
    hausdorff_ref's distance planes."""
    out = [(n, m) for n, m in device_planes() if not n.startswith("real_")]
    return out + list(R.distance_planes().items())
