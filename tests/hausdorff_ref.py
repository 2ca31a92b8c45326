"""Expected values and fixtures of the device Hausdorff route (csrc/contour_hausdorff.hip, ops.contour_hausdorff).

The expected vertex lists are `cvlite.find_contours_external(m)[0]`, the squared distances numpy integer broadcasting on them, the
final floats `evaluation.calculate_hausdorff`: the host route as it stands. Everything is an integer until the last square root, so
every comparison against the device is exact equality.

The fixtures are the smallest planes at which a stage can go wrong; TILE and CHUNK restate the two sizes of the kernels they are
built around (the labelling kernel's LDS tile side and the distance kernel's LDS chunk, csrc/contour_hausdorff.hip kTile / kChunk).
"""
import math
import os

import numpy as np

from haff import cvlite, evaluation

TILE = 32          # label_tile_kernel labels TILE x TILE pixels in LDS; label_seam_kernel joins the tiles
CHUNK = 1024       # hausdorff_d2_kernel stages the inner list through LDS CHUNK points at a time
OVERFLOW_BENCH, FAULT_BENCH, OVERFLOW_PRED, FAULT_PRED = 1, 2, 4, 8
SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")


# ---- the reference ----------------------------------------------------------------------------------------------------------

def vertices(m):
    """int64 [n, 2] (x, y): the ordered vertices of find_contours_external(m)[0]; [0, 2] without a contour."""
    c = cvlite.find_contours_external(np.asarray(m).astype(np.uint8))
    return c[0].reshape(-1, 2).astype(np.int64) if c else np.zeros((0, 2), np.int64)


def d2(a, b):
    """max over a of min over b of |a - b|^2, in integers, 256 outer points at a time."""
    best = 0
    for i in range(0, len(a), 256):
        d = a[i:i + 256, None, :] - b[None, :, :]
        best = max(best, int((d * d).sum(-1).min(1).max()))
    return best


def expected_row(vb, vp, flags=0):
    """The device's result row for a pair of vertex lists: both distances 0 when a side is empty or a flag is set."""
    if flags or len(vb) == 0 or len(vp) == 0:
        return [len(vb), len(vp), 0, 0, flags, 0]
    return [len(vb), len(vp), d2(vp, vb), d2(vb, vp), flags, 0]


def distances(row, shape):
    """(directed, symmetric) from a result row: the two empty rules of calculate_hausdorff, one math.sqrt of an integer each."""
    nb, n_pred, d_pb, d_bp = row[:4]
    if n_pred == 0:
        d = float(np.sqrt(shape[0] ** 2 + shape[1] ** 2))
        return d, d
    if nb == 0:
        return 0, 0
    return math.sqrt(d_pb), math.sqrt(max(d_pb, d_bp))


def start_by_rule(m):
    """The issue's start-pixel rule, from scipy.ndimage.label: the maximum, over the foreground pixels whose left neighbour is
    outside, of the raster-first pixel of the pixel's 8-connected component; None without a candidate. (x, y)."""
    from scipy import ndimage
    fg = np.pad(np.asarray(m) != 0, 1)
    comp, _ = ndimage.label(fg, structure=np.ones((3, 3), int))
    back, _ = ndimage.label(~fg)                               # 4-connected by default
    outside = back == back[0, 0]
    cand = fg & np.roll(outside, 1, axis=1)
    if not cand.any():
        return None
    flat = comp.reshape(-1)
    first = {}
    for i in np.flatnonzero(flat):
        first.setdefault(flat[i], i)
    root = max(first[c] for c in np.unique(comp[cand]))
    return int(root % fg.shape[1]) - 1, int(root // fg.shape[1]) - 1


def component_first_pixel(m, xy):
    """The raster-first pixel (x, y) of the 8-connected foreground component of m that holds the pixel xy."""
    from scipy import ndimage
    comp, _ = ndimage.label(np.asarray(m) != 0, structure=np.ones((3, 3), int))
    ys, xs = np.nonzero(comp == comp[xy[1], xy[0]])
    return int(xs[0]), int(ys[0])


# ---- fixtures ---------------------------------------------------------------------------------------------------------------

def _z(h, w):
    return np.zeros((h, w), np.uint8)


def _on(h, w, pixels):
    m = _z(h, w)
    for x, y in pixels:
        m[y, x] = 1
    return m


def spiral(h, w, centre=False, sealed=False):
    """A one-pixel-wide wall spiralling inwards from (0, 0) with three pixels of background between its turns. centre: one more
    pixel at the inner end of the background channel, touching no wall: a component of its own, external only through the whole
    length of the channel. sealed: the channel's mouth (column 0, rows 1-3) is walled up, so that pixel is not external."""
    m = _z(h, w)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        nx, ny = x + dx, y + dy
        ahead = [(nx + k * dx, ny + k * dy) for k in range(1, 4)]     # keep the channel three pixels wide
        if 0 <= nx < w and 0 <= ny < h and not any(0 <= ax < w and 0 <= ay < h and m[ay, ax] for ax, ay in ahead):
            x, y = nx, ny
            m[y, x] = 1
            turns = 0
        else:
            dx, dy = -dy, dx
            turns += 1
    if centre:
        cy, cx = _channel_end(m)
        m[cy, cx] = 1
    if sealed:
        m[1:4, 0] = 1
    return m


def _channel_end(m):
    """Among the background pixels that touch no wall, the one farthest (4-connected steps) from the plane's edge."""
    h, w = m.shape
    dist = np.full((h, w), -1)
    frontier = [(y, x) for y in range(h) for x in range(w) if m[y, x] == 0 and (y in (0, h - 1) or x in (0, w - 1))]
    for y, x in frontier:
        dist[y, x] = 0
    while frontier:
        nxt = []
        for y, x in frontier:
            for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                if 0 <= yy < h and 0 <= xx < w and m[yy, xx] == 0 and dist[yy, xx] < 0:
                    dist[yy, xx] = dist[y, x] + 1
                    nxt.append((yy, xx))
        frontier = nxt
    pad = np.pad(m, 1)
    near = sum(pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) > 0
    dist[near] = -1
    cy, cx = np.unravel_index(int(np.argmax(dist)), dist.shape)
    assert dist[cy, cx] > 0
    return int(cy), int(cx)


def comb(h, w):
    """Teeth in every other column over the full height, joined only by the bottom row."""
    m = _z(h, w)
    m[:, ::2] = 1
    m[h - 1, :] = 1
    return m


def battlement(n, width=126):
    """Bars two rows thick joined by a spine in column 0, n one-pixel merlons on them: about two vertices per merlon on a small
    plane. many_vertices() pins the (n, width) that give the exact counts the distance kernel's edges need."""
    per = (width - 2) // 2
    bars = (n + per - 1) // per if n else 1
    m = _z(4 * bars + 1, width)
    left = n
    for b in range(bars):
        y = 4 * b + 2
        m[y:y + 2, :] = 1
        k = min(per, left)
        left -= k
        m[y - 1, 2:2 + 2 * k:2] = 1
    m[1:, 0] = 1
    return m


_MANY = {26: (10, 126), CHUNK - 1: (491, 126), CHUNK: (489, 124), CHUNK + 1: (492, 126), 3 * CHUNK + 1: (1476, 126)}


def many_vertices(v, canvas=(100, 128)):
    """A plane whose [0] has exactly v vertices (tests/test_hausdorff_ref_cpu.py asserts the counts), on a common canvas."""
    b = battlement(*_MANY[v])
    m = _z(*canvas)
    m[:b.shape[0], :b.shape[1]] = b
    return m


def small_planes():
    """name -> plane: every small fixture of the issue's list."""
    t = TILE
    p = {}
    p["empty"] = _z(5, 7)
    p["full"] = np.ones((5, 7), np.uint8)
    p["one_on"] = np.ones((1, 1), np.uint8)
    p["one_off"] = _z(1, 1)
    p["pixel_first"] = _on(5, 7, [(0, 0)])
    p["pixel_last"] = _on(5, 7, [(6, 4)])
    p["pixel_inside"] = _on(5, 7, [(3, 2)])
    p["row_1x7"] = np.ones((1, 7), np.uint8)
    p["column_7x1"] = np.ones((7, 1), np.uint8)
    p["row_inside"] = _on(5, 9, [(x, 2) for x in range(2, 7)])
    p["diagonal"] = _on(8, 8, [(i + 1, i + 1) for i in range(6)])
    p["antidiagonal"] = _on(8, 8, [(6 - i, i + 1) for i in range(6)])
    p["plus"] = _on(9, 9, [(4, y) for y in range(1, 8)] + [(x, 4) for x in range(1, 8)])
    p["thin_L"] = _on(9, 9, [(2, y) for y in range(1, 8)] + [(x, 7) for x in range(2, 8)])
    two = _z(12, 12)
    two[1:4, 1:4] = 1
    two[6:10, 5:11] = 1
    p["two_blobs"] = two                                          # [0] is the later one
    trap = _z(12, 12)
    trap[1:10, 1:3] = 1                                           # B: starts on row 1 ...
    trap[8:10, 1:11] = 1                                          # ... and reaches below and right of A
    trap[3:6, 6:9] = 1                                            # A: starts on row 3, [0]
    p["trap"] = trap
    ring = _z(13, 13)
    ring[1:12, 1:12] = 1
    ring[3:10, 3:10] = 0
    p["ring"] = ring.copy()
    ring[5:8, 5:8] = 1
    p["ring_with_blob"] = ring                                    # the blob starts later but is not external
    corner = _z(8, 8)
    corner[1:4, 1:4] = 1
    corner[4:7, 4:7] = 1
    p["corner_touch"] = corner                                    # one 8-connected component
    dia = _on(9, 9, [(4, 1), (3, 2), (5, 2), (2, 3), (6, 3), (1, 4), (7, 4), (2, 5), (6, 5), (3, 6), (5, 6), (4, 7)])
    p["diamond"] = dia.copy()
    dia[4, 4] = 1
    p["diamond_with_pixel"] = dia                                 # inside the diamond is not outside: no diagonal leaks
    for h, w in ((t - 1, t - 1), (t, t), (t + 1, t + 1), (t + 1, 2 * t + 1), (2 * t + 3, 4 * t + 1)):
        p[f"spiral_{h}x{w}"] = spiral(h, w)
        p[f"spiral_centre_{h}x{w}"] = spiral(h, w, centre=True)
        p[f"spiral_sealed_{h}x{w}"] = spiral(h, w, centre=True, sealed=True)
        p[f"comb_{h}x{w}"] = comb(h, w)
        p[f"comb_down_{h}x{w}"] = comb(h, w)[::-1].copy()
    return p


def random_planes():
    out = []
    for k in range(40):
        density = (0.3, 0.45, 0.55, 0.7)[k % 4]
        out.append((np.random.default_rng(1000 + k).random((48, 48)) < density).astype(np.uint8))
    return out


def distance_planes():
    """name -> plane on the common canvas: contours of 1, 2, c-1, c, c+1 and 3c+1 vertices, and the tie pair."""
    c = CHUNK
    p = {f"v{v}": many_vertices(v) for v in (c - 1, c, c + 1, 3 * c + 1)}
    p["v1"] = _on(100, 128, [(64, 50)])
    p["v2"] = _on(100, 128, [(x, 60) for x in range(20, 41)])
    p["tie"] = _on(100, 128, [(30, 50)])                          # equally far from both ends of v2's line
    return p


DISTANCE_PAIRS = [("v1", "v1025"), ("v1025", "v1"), ("v2", "v1024"), ("v1023", "v3073"), ("v3073", "v1024"), ("v1024", "v1024"),
                  ("v1025", "v1023"), ("v2", "tie"), ("tie", "v2"), ("v1", "v2")]


def wide_planes():
    """The largest coordinates: 2 x 4096 with pixels at both ends ([0] is the one at (4095, 1)), against the pixel at (0, 0)."""
    return _on(2, 4096, [(0, 0), (4095, 1)]), _on(2, 4096, [(0, 0)])


def real_pair():
    """One 855 x 855 pair of the sample's ground truth: left against right hand."""
    from PIL import Image
    leaf = os.path.join(SAMPLE, "8f91bc0d-9ce7-4b31-aba7-dd59791917df", "00000029")
    return tuple((np.array(Image.open(os.path.join(leaf, f"aff_{s}.png")).convert("L")) > 0).astype(np.uint8) for s in ("left", "right"))


def all_cpu_fixtures():
    """(name, plane) of everything but the 855 x 855 pair."""
    out = list(small_planes().items())
    out += [(f"noise{k}", m) for k, m in enumerate(random_planes())]
    out += list(distance_planes().items())
    out += [("wide_both", wide_planes()[0]), ("wide_first", wide_planes()[1]), ("capacity", many_vertices(26, (8, 128)))]
    return out


def cpu_pairs():
    """(bench, pred) planes of equal shape from the fixtures: each small plane against its point mirror, the noise planes against
    one another, the distance edges, the wide pair both ways, and the two empty rules."""
    pairs = []
    for m in small_planes().values():
        pairs.append((m, m[::-1, ::-1].copy()))
    r = random_planes()
    pairs += [(r[k], r[(k + 7) % 40]) for k in range(40)]
    d = distance_planes()
    pairs += [(d[a], d[b]) for a, b in DISTANCE_PAIRS]
    w = wide_planes()
    pairs += [(w[0], w[1]), (w[1], w[0])]
    e = small_planes()
    pairs += [(e["empty"], e["full"]), (e["full"], e["empty"]), (e["empty"], e["empty"])]
    return pairs


def calculate_hausdorff(bench, pred):
    return evaluation.calculate_hausdorff(bench > 0, pred > 0)
