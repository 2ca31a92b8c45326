"""An independent restatement of the affordance extraction (2HANDS/scripts/affordance_extraction_preparation.py:256-304) for the tests:
brute force, plain loops over pixels and taps, its own gather tables. It calls nothing of cvlite or ops.

  tables(hand_hw, out_hw)         the nearest-resize indices of the hand padded to a square, per axis, -1 = padding
  extract(plane, hand, k)         (a, out, stats): the AND plane, the dilated and recoloured plane, the eight statistics words
  exact= / pad_end= / logical= / symmetric= / count_after=
                                  the same with ONE rule wrong each: what the inputs of the tests have to tell apart
  planes(shape, rng) / hands(...)  the inputs shared by the CPU and the GPU tests
  make_tree(root) ...             a generated sequence tree with one sequence of every kind, for the dataset_build tests
"""
import numpy as np

TILE_H, TILE_W = 16, 64            # one output tile of csrc/affordance_extract.hip: where the seams are
SHAPES = [(1, 1), (1, 9), (3, 5), (7, 7), (16, 64), (17, 65), (37, 131), (40, 132)]
KS = (1, 2, 3, 4, 7, 31)
HAND_FLAG, GREY_FLAG = 1, 2


def nearest_index(x, D, S, exact=False):
    """resizeNN: min(floor(x * (1.0 / (D / S))), S - 1) in doubles; exact=True is the MISTAKE, the rational floor."""
    if exact:
        return min((x * S) // D, S - 1)
    scale = float(D) / float(S)
    inv = 1.0 / scale
    return min(int(np.floor(float(x) * inv)), S - 1)


def tables(hand_hw, out_hw, exact=False, pad_end=False):
    """(col, row) as Python lists. pad_end=True is the MISTAKE: padding on the right / bottom instead of the left / top."""
    Hh, Wh = hand_hw
    H, W = out_hw
    S = max(Hh, Wh)
    pad_c = S - Wh if Hh > Wh else 0
    pad_r = 0 if Hh > Wh else S - Hh
    if pad_end:
        pad_c = pad_r = 0
    col, row = [], []
    for x in range(W):
        p = nearest_index(x, W, S, exact) - pad_c
        col.append(p if 0 <= p < Wh else -1)
    for y in range(H):
        p = nearest_index(y, H, S, exact) - pad_r
        row.append(p if 0 <= p < Hh else -1)
    return col, row


def and_plane(plane, hand, exact=False, pad_end=False, logical=False):
    """a = plane & hand gathered (bitwise on the grey values). logical=True is the MISTAKE: the plane's value wherever both are on."""
    plane = np.asarray(plane)
    if hand is None:
        return plane.copy()
    H, W = plane.shape
    col, row = tables(hand.shape, plane.shape, exact, pad_end)
    h = np.zeros((H, W), np.uint8)                      # the padded, resized hand, row by row
    for y in range(H):
        if row[y] >= 0:
            h[y] = [int(hand[row[y], c]) if c >= 0 else 0 for c in col]
    if logical:
        return np.where((plane != 0) & (h != 0), plane, 0).astype(np.uint8)
    return plane & h


def dilate_white(a, k, symmetric=False):
    """255 where the k x k window around the pixel holds a non-zero value. Window [p - k // 2, p + k - 1 - k // 2] per axis, taps
    outside the image left out. symmetric=True is the MISTAKE: [p - (k - 1) // 2, p + k // 2], the mirror image for even k."""
    H, W = a.shape
    lo = (k - 1) // 2 if symmetric else k // 2
    on = a != 0
    out = np.zeros((H, W), np.uint8)
    ys, xs = np.nonzero(on)
    for y, x in zip(ys.tolist(), xs.tolist()):          # a set pixel at p' turns on every p with p' in [p - lo, p + k - 1 - lo]
        y_from, y_to = max(y - (k - 1 - lo), 0), min(y + lo, H - 1)
        x_from, x_to = max(x - (k - 1 - lo), 0), min(x + lo, W - 1)
        out[y_from:y_to + 1, x_from:x_to + 1] = 255
    return out


def dilate_white_taps(a, k):
    """The same rule the other way round, tap by tap (for the small fixtures): a second formulation to check the first."""
    H, W = a.shape
    lo = k // 2
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            hit = False
            for yy in range(y - lo, y + k - lo):
                for xx in range(x - lo, x + k - lo):
                    if 0 <= yy < H and 0 <= xx < W and a[yy, xx] != 0:
                        hit = True
            out[y, x] = 255 if hit else 0
    return out


def stats_of(a, out, hand_given, count_after=False):
    """The eight statistics words. count_after=True is the MISTAKE: the emptiness count (word 0) taken after the dilation. As a
    yes / no answer the two agree (a dilation neither empties nor fills an empty plane); as the count the kernel reports they do not."""
    H, W = a.shape
    ys, xs = np.nonzero(out)
    box = [int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())] if len(ys) else [H, -1, W, -1]
    grey = bool(((a != 0) & (a != 255)).any())
    return [int(((out if count_after else a) != 0).sum()), int((out != 0).sum()), int(a.astype(np.int64).sum())] + box + \
           [(HAND_FLAG if hand_given else 0) | (GREY_FLAG if grey else 0)]


def extract(plane, hand, k, **wrong):
    """(a, out, stats) of one item. wrong: exact / pad_end / logical for the AND, symmetric for the window, count_after for word 0."""
    sym, after = wrong.pop("symmetric", False), wrong.pop("count_after", False)
    a = and_plane(plane, hand, **wrong)
    out = dilate_white(a, k, symmetric=sym)
    return a, out, stats_of(a, out, hand is not None, after)


def process(mask, k):
    """process_affordances on one mask: None when delete_empty_masks removes it (all zero BEFORE the dilation), else the dilated
    and recoloured plane."""
    mask = np.asarray(mask)
    if not (mask != 0).any():
        return None
    return dilate_white(mask, k)


def seams(n, tile):
    """both sides of every tile seam along an axis of length n, plus the ends"""
    s = {0, n - 1}
    for t in range(tile, n, tile):
        s |= {t - 1, t}
    return sorted(s)


def planes(shape, rng):
    """[(name, uint8 plane)]: all zero, all 255, lone pixels in each corner and on both sides of every tile seam, sparse random,
    the values 1 and 2 only, one-pixel stripes at the seams."""
    H, W = shape
    out = [("zeros", np.zeros(shape, np.uint8)), ("full", np.full(shape, 255, np.uint8))]
    ys, xs = seams(H, TILE_H), seams(W, TILE_W)
    for y in ys:
        for x in xs:
            p = np.zeros(shape, np.uint8)
            p[y, x] = 255
            out.append((f"lone_{y}_{x}", p))
    out.append(("sparse", (rng.random(shape) < 0.02).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)))
    out.append(("sparse255", (rng.random(shape) < 0.05).astype(np.uint8) * 255))
    out.append(("ones_twos", rng.integers(1, 3, shape).astype(np.uint8)))
    for y in ys:
        p = np.zeros(shape, np.uint8)
        p[y, :] = 255
        out.append((f"hstripe_{y}", p))
    for x in xs:
        p = np.zeros(shape, np.uint8)
        p[:, x] = 255
        out.append((f"vstripe_{x}", p))
    return out


def hands(shape, rng):
    """[(name, hand or None)]: none, the same shape, a landscape and a portrait hand that need the pad, 6 wide into the plane (34 wide
    planes are in the CPU fixtures; here whatever the plane's width is), a hand larger than the plane. Values 255 / 0 in blobs, and
    one hand of the values 2 and 3 (the bitwise AND with 1 and 2 differs from the logical one)."""
    H, W = shape

    def blob(hw, p=0.6):
        return (rng.random(hw) < p).astype(np.uint8) * 255

    return [("none", None), ("same", blob((H, W))), ("landscape", blob((max(H // 2, 1), W + 3))),
            ("portrait", blob((H + 5, max(W // 3, 1)))), ("six", blob((6, 6))), ("larger", blob((2 * H + 1, 2 * W + 3))),
            ("twos_threes", rng.integers(2, 4, (H, W)).astype(np.uint8))]


# ---- a generated sequence tree for the dataset_build tests ---------------------------------------------------------------------------

TREE_HW = (48, 64)
TREE_K, TREE_LIMIT, TREE_CATEGORIES = 3, 700.0, ["cup", "pan"]
VERB_CSV = ("id,key,instances\n"
            "0,take,\"['take', 'pick-up', 'grab']\"\n"
            "1,put,\"['put', 'put-down', 'place']\"\n"
            "2,eat,\"['eat', 'taste']\"\n"
            "3,cut,\"['cut', 'slice']\"\n")
# name: (kind, what is_valid answers) in the order of the sorted folders
TREE_KINDS = {
    "s00_bimanual": "valid", "s01_left_only": "valid", "s02_right_only": "valid", "s03_empty_after_and": "missing_file",
    "s04_too_few": "threshold", "s05_too_many": "threshold", "s06_invalid_verb": "verb_class", "s07_wrong_category": "category",
    "s08_missing_frame": "missing_file", "s09_zero_object": "empty_object", "s10_resized_hand": "valid", "s11_substring_verb": "valid",
    "s12_null_noun": "null_annotation", "s13_unknown_verb": "verb_class", "s14_right_only_first_zero": "missing_file",
}


def _rect(hw, y0, y1, x0, x1, value=255):
    p = np.zeros(hw, np.uint8)
    p[y0:y1, x0:x1] = value
    return p


def make_tree(root):
    """Writes the tree `dataset_build build` reads under root (C, H, O, S as its docstring names them) plus verbs.csv, about a
    dozen sequences at 48 x 64 with at least one of every kind of TREE_KINDS. Returns the paths."""
    import json
    import os
    from PIL import Image
    H, W = TREE_HW
    paths = {k: os.path.join(str(root), k) for k in ("C", "H", "O", "S")}
    for k in ("C", "H", "O"):
        for side in ("left", "right"):
            os.makedirs(os.path.join(paths[k], side))

    def put(kind, side, name, plane):
        Image.fromarray(plane).save(os.path.join(paths[kind], side, name + ".png"))

    ring = _rect((H, W), 8, 30, 6, 30)
    ring[14:24, 12:24] = 0                                   # a hole no 3 x 3 dilation closes
    full_hand = np.full((H, W), 255, np.uint8)
    small = _rect((H, W), 10, 20, 40, 52)                    # 120 pixels, 168 after a 3 x 3 dilation
    obj = _rect((H, W), 4, 40, 2, 60)
    rng = np.random.default_rng(7)
    for name, kind in TREE_KINDS.items():
        ann = {"taxonomy": [1, 0, 0, 0], "noun": "cup", "verb": "take", "narration": "take the cup", "obj_left": "cup", "obj_right": None,
               "vector": None}
        sides = ("left",)
        comp = {"left": ring, "right": small}
        hand = {"left": full_hand, "right": full_hand}
        objs = {"left": obj, "right": obj}
        if name == "s00_bimanual":
            sides, ann["taxonomy"], ann["obj_right"] = ("left", "right"), [0, 0, 1, 0], "pan"
        elif name == "s02_right_only":
            # is_valid takes taxonomy[0] == 0 for the bimanual case, so a right-only sequence passes only with a non-zero first entry
            sides, ann["obj_left"], ann["obj_right"] = ("right",), None, "pan"
        elif name == "s14_right_only_first_zero":
            sides, ann["taxonomy"], ann["obj_left"], ann["obj_right"] = ("right",), [0, 1, 0, 0], None, "pan"
        elif name == "s03_empty_after_and":
            hand = {"left": _rect((H, W), 40, 48, 40, 64)}   # nowhere near the ring
        elif name == "s04_too_few":
            hand = {"left": _rect((H, W), 8, 9, 6, 8)}       # 2 pixels: 12 after the dilation, not over 20
        elif name == "s05_too_many":
            comp = {"left": _rect((H, W), 2, 40, 2, 40)}     # 1444 pixels: over the limit of 700
        elif name == "s06_invalid_verb":
            ann["verb"] = "eat"
        elif name == "s07_wrong_category":
            ann["obj_left"] = "knife"
        elif name == "s09_zero_object":
            objs = {"left": np.zeros((H, W), np.uint8)}
        elif name == "s10_resized_hand":
            sides, ann["taxonomy"], ann["obj_right"] = ("left", "right"), [0, 0, 0, 1], "cup"
            hand = {"left": (rng.random((60, 40)) < 0.9).astype(np.uint8) * 255,      # portrait: padded on the left, then resized
                    "right": (rng.random((40, 50)) < 0.9).astype(np.uint8) * 255}     # landscape: padded on the top
            hand["left"][:, :4] = 255
        elif name == "s11_substring_verb":
            ann["verb"] = "up"                               # a substring of 'pick-up' in the FIRST row: class take
        elif name == "s12_null_noun":
            ann["noun"] = None
        elif name == "s13_unknown_verb":
            ann["verb"] = "juggle"
        for side in sides:
            put("C", side, name, comp[side])
            put("H", side, name, hand[side])
            put("O", side, name, objs[side])
        seq = os.path.join(paths["S"], name)
        os.makedirs(seq)
        with open(os.path.join(seq, "annotation.json"), "w") as fh:
            json.dump(ann, fh)
        if name != "s08_missing_frame":
            Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(seq, "inpainted_frame.png"))
    put("C", "left", "zz_no_partner", ring)                  # a completed mask without a hand mask: skipped with the message
    paths["csv"] = os.path.join(str(root), "verbs.csv")
    with open(paths["csv"], "w") as fh:
        fh.write(VERB_CSV)
    return paths


def assemble_sequences(paths, aff_dir, out_dir):
    """The sequence folders create_dataset reads, from the processed affordance PNGs, the object PNGs and S: what the reference's
    pipeline does between process_affordances and create_dataset."""
    import os
    import shutil
    for name in sorted(os.listdir(paths["S"])):
        dst = os.path.join(out_dir, name)
        shutil.copytree(os.path.join(paths["S"], name), dst)
        for side in ("left", "right"):
            for kind, src in (("aff", aff_dir), ("obj", paths["O"])):
                f = os.path.join(src, side, name + ".png")
                if os.path.isfile(f):
                    shutil.copy(f, os.path.join(dst, f"{kind}_{side}.png"))
    return out_dir


def tree_files(root):
    """{relative path: bytes} of every file under root"""
    import os
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def fill_holes(plane):
    """plane != 0 with every background region that does not reach the frame (4-connected) turned on"""
    on = np.asarray(plane) != 0
    H, W = on.shape
    outside = np.zeros((H + 2, W + 2), bool)
    free = np.ones((H + 2, W + 2), bool)
    free[1:-1, 1:-1] = ~on
    stack = [(0, 0)]
    outside[0, 0] = True
    while stack:
        y, x = stack.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < H + 2 and 0 <= xx < W + 2 and free[yy, xx] and not outside[yy, xx]:
                outside[yy, xx] = True
                stack.append((yy, xx))
    return ~outside[1:-1, 1:-1]
