"""CPU restatement of csrc/contour_fill.hip (haff_fill_contours_u8) and the cases its tests share.

`fill_planes` follows the kernels step by step, in Python integers: the closed form of cvlite._line8's Bresenham walk (pixel i of
a line has taken floor((2*minor*i + major - 1) / (2*major)) minor-axis steps, so pixels are independent work items) and the
row-parallel scanline fill (each row on its own: the 16.16 crossings of the polygon's non-horizontal edges, every crossing's rank
and successor in (value, edge index) order, even ranks open a span). The reference both are held to is cvlite.draw_contours_filled.
"""
import random

import numpy as np

MAX_VERTS, MAX_COORD = 4096, 32768   # the entry point's host-checked limits


def cdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def line_pixels(x0, y0, x1, y1):
    """Every pixel of cvlite._line8(x0, y0, x1, y1), unclipped, from the closed form."""
    if x1 < x0:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx = x1 - x0
    sy = 1 if y1 >= y0 else -1
    dy = abs(y1 - y0)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    out = []
    for i in range(major + 1):
        c = (2 * minor * i + major - 1) // (2 * major) if major > 0 else 0
        out.append((x0 + c, y0 + sy * i) if steep else (x0 + i, y0 + sy * c))
    return out


def row_spans(pts, y):
    """The [x1, x2] spans (unclipped, inclusive) the fill kernel writes on row y of one polygon."""
    n = len(pts)
    cross = []
    for e in range(n):
        px, py = pts[e - 1]
        qx, qy = pts[e]
        y0, y1 = min(py, qy), max(py, qy)
        if y0 <= y < y1:
            d = cdiv((qx - px) * 65536, qy - py)
            cross.append((px if py < qy else qx) * 65536 + (y - y0) * d)
    spans = {}
    for k, xk in enumerate(cross):
        rank, nxt = 0, None
        for j, xj in enumerate(cross):
            if xj < xk or (xj == xk and j < k):
                rank += 1
            elif j != k:
                nxt = xj if nxt is None else min(nxt, xj)
        if rank % 2 == 0 and rank + 1 < len(cross):
            spans[rank] = (xk >> 16, nxt >> 16)
    return [spans[r] for r in sorted(spans)]


def fill_planes(planes, hw):
    """uint8 [len(planes), H, W]: what haff_fill_contours_u8 computes for one list of contours per plane."""
    H, W = hw
    out = np.zeros((len(planes), H, W), dtype=np.uint8)
    for pl, contours in enumerate(planes):
        for c in contours or []:
            pts = [(int(x), int(y)) for x, y in np.asarray(c, dtype=np.int32).reshape(-1, 2)]
            n = len(pts)
            for e in range(n):
                for x, y in line_pixels(*pts[e - 1], *pts[e]):
                    if 0 <= x < W and 0 <= y < H:
                        out[pl, y, x] = 1
            ys = [(pts[e - 1][1], pts[e][1]) for e in range(n) if pts[e - 1][1] != pts[e][1]]
            if n < 2 or len(ys) < 2:
                continue
            ymin, ymax = min(min(a, b) for a, b in ys), max(max(a, b) for a, b in ys)
            for y in range(max(ymin, 0), min(ymax, H)):
                for x1, x2 in row_spans(pts, y):
                    if x1 < W and x2 >= 0:
                        out[pl, y, max(x1, 0):min(x2, W - 1) + 1] = 1
    return out


def random_cases(n=300, seed=0):
    """(hw, contours) x n: 1-3 contours of 1-12 vertices, coordinates in [-8, W+8] x [-8, H+8], planes of 48x64, 33x47 and 64x64."""
    rng = random.Random(seed)
    cases = []
    for _ in range(n):
        h, w = rng.choice([(48, 64), (33, 47), (64, 64)])
        cs = []
        for _ in range(rng.randint(1, 3)):
            cs.append([[rng.randint(-8, w + 8), rng.randint(-8, h + 8)] for _ in range(rng.randint(1, 12))])
        cases.append(((h, w), cs))
    return cases


def comb(teeth=40, pitch=3, top=4, bottom=36):
    """A comb whose rows between the teeth's tips and the spine cross 2 * teeth edges (80 for 40 teeth: more than a wave's lanes)."""
    pts = []
    for t in range(teeth):
        x = 2 + pitch * t
        pts += [[x, bottom], [x, top], [x + 1, top], [x + 1, bottom]]
    pts += [[2 + pitch * teeth, bottom], [2 + pitch * teeth, bottom + 2], [2, bottom + 2]]
    return pts


def named_cases():
    """name -> (hw, contours): the shapes the kernel's branches and borders are pinned at. Planes of 48x64 and 33x47: no dimension
    is a multiple of a wave or of 16."""
    A, B = (48, 64), (33, 47)
    return {
        "empty": (A, []),
        "single_vertex": (B, [[[5, 7]]]),
        "two_vertices": (A, [[[3, 4], [40, 30]]]),
        "horizontal_only": (B, [[[2, 9], [30, 9], [17, 9]]]),
        "rectangle": (A, [[[10, 10], [30, 10], [30, 25], [10, 25]]]),
        "diamond": (B, [[[20, 4], [32, 16], [20, 28], [8, 16]]]),
        "concave_u": (A, [[[8, 5], [18, 5], [18, 30], [40, 30], [40, 5], [52, 5], [52, 42], [8, 42]]]),
        "bow_tie": (B, [[[5, 5], [40, 28], [40, 5], [5, 28]]]),
        "cut_left": (A, [[[-6, 10], [12, 8], [9, 30], [-7, 25]]]),
        "cut_right": (A, [[[50, 10], [70, 14], [69, 33], [55, 30]]]),
        "cut_top": (B, [[[10, -7], [30, -5], [28, 9], [14, 12]]]),
        "cut_bottom": (B, [[[10, 25], [30, 22], [33, 40], [8, 39]]]),
        "outside": (A, [[[70, 50], [90, 52], [80, 70]], [[-30, -20], [-10, -25], [-15, -5]]]),
        "overlapping": (A, [[[5, 5], [35, 8], [30, 30], [8, 28]], [[20, 15], [55, 12], [58, 40], [25, 44]]]),
        "comb": ((40, 128), [comb()]),
        # the crossing of the long edge at its last rows is x0 * 65536 + rows * dx with |dx| * rows = 65000 * 65536 > 2^31
        "wide_edge": (A, [[[-32500, -20], [32500, 60], [32500, 70], [-32500, -10]]]),
    }


MULTI_PLANE = ((33, 47), [[], [[[3, 3], [20, 5], [12, 20]]],
                          [[[0, 0], [46, 0], [46, 32], [0, 32]], [[10, 10], [30, 12], [20, 30]], [[40, 1]]],
                          [[[25, 25], [60, 28], [44, 50]]], []])   # 0, 1, 3, 1, 0 polygons
