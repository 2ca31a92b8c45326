"""Building 2HANDS records from masks, host side: the hand-derived fixtures of the exact semantics, checked on the brute-force
restatement (tests/extract_ref.py) and on cvlite / ops.nearest_pad_tables; cvlite against the restatement on everything the GPU test
uses; five one-mistake variants of the restatement, each failing on these inputs; create_dataset's is_valid rule by rule; the
file-writing subcommands on the host route; the entry point's declaration. Nothing here computes on a GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import haff
from haff import cvlite, dataset_build, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/extract_ref.py
import extract_ref as E   # noqa: E402


def _lone(shape, y, x, v=255):
    p = np.zeros(shape, np.uint8)
    p[y, x] = v
    return p


def _on_cols(out, row=0):
    return np.nonzero(out[row])[0].tolist()


def _dilations(a, k):
    """the three statements of the window, which must agree: the restatement's two formulations and cvlite"""
    got = E.dilate_white(a, k)
    assert np.array_equal(got, E.dilate_white_taps(a, k))
    assert np.array_equal(got, np.where(cvlite.dilate_rect(a, k) != 0, 255, 0))
    assert np.array_equal(got, cvlite.process_affordance(a, k)) if a.any() else cvlite.process_affordance(a, k) is None
    return got


def test_lone_pixel_windows():
    """A lone pixel at column 5 turns on 4..7 for k = 4 and 4..6 for k = 3; at column 0 it turns on 0..2 for k = 4; rows likewise;
    every border and corner."""
    assert _on_cols(_dilations(_lone((1, 12), 0, 5), 4)) == [4, 5, 6, 7]
    assert _on_cols(_dilations(_lone((1, 12), 0, 5), 3)) == [4, 5, 6]
    assert _on_cols(_dilations(_lone((1, 12), 0, 0), 4)) == [0, 1, 2]
    assert _on_cols(_dilations(_lone((1, 12), 0, 0), 3)) == [0, 1]
    assert _on_cols(_dilations(_lone((1, 12), 0, 11), 4)) == [10, 11]
    assert _on_cols(_dilations(_lone((1, 12), 0, 11), 3)) == [10, 11]
    for k, rows in ((4, [4, 5, 6, 7]), (3, [4, 5, 6])):
        out = _dilations(_lone((12, 12), 5, 5), k)
        assert np.nonzero(out.any(axis=1))[0].tolist() == rows and np.nonzero(out.any(axis=0))[0].tolist() == rows
        assert int((out != 0).sum()) == k * k and set(np.unique(out)) == {0, 255}
    out = _dilations(_lone((12, 12), 0, 0, v=3), 4)           # the top-left corner, a grey value: recoloured
    assert np.argwhere(out).max(axis=0).tolist() == [2, 2] and out[0, 0] == 255
    out = _dilations(_lone((12, 12), 11, 11), 4)              # the bottom-right corner
    assert np.argwhere(out).min(axis=0).tolist() == [10, 10]
    assert np.array_equal(_dilations(_lone((5, 5), 2, 2, v=9), 1), _lone((5, 5), 2, 2))     # k = 1 is the recolour alone
    assert cvlite.dilate_rect(_lone((5, 5), 2, 2, v=9), 3)[1, 1] == 9                     # dilate_rect itself is the grey maximum
    both = _lone((1, 9), 0, 2, v=9) + _lone((1, 9), 0, 4, v=200)
    assert cvlite.dilate_rect(both, 3)[0].tolist() == [0, 9, 9, 200, 200, 200, 0, 0, 0]


def test_nearest_index_is_opencvs_double_not_the_rational_floor():
    col, _ = E.tables((6, 6), (34, 34))
    assert col[17] == 2 and (17 * 6) // 34 == 3
    assert E.tables((6, 6), (34, 34), exact=True)[0][17] == 3
    c, r = ops.nearest_pad_tables((6, 6), (34, 34))
    assert c.dtype == torch.int32 and c.tolist() == col and r.tolist() == col
    src = np.arange(6, dtype=np.uint8)[None, :].repeat(6, 0)
    assert cvlite.resize_nearest(src, (34, 34))[0].tolist() == col
    differing = 0
    for S in range(1, 200):
        for D in range(1, 200):
            inv = 1.0 / (D / S)
            p = np.minimum(np.floor(np.arange(D) * inv), S - 1).astype(np.int64)
            differing += bool((p != np.minimum(np.arange(D) * S // D, S - 1)).any())
            if D == S:
                assert np.array_equal(p, np.arange(S))        # an unchanged length reads itself
    assert differing == 1701


def test_padding_sides():
    wide = np.arange(1, 11, dtype=np.uint8).reshape(2, 5)     # landscape: padded on the TOP to 5 x 5
    sq = cvlite.pad_to_square(wide)
    assert sq.shape == (5, 5) and not sq[:3].any() and np.array_equal(sq[3:], wide)
    assert E.tables((2, 5), (5, 5)) == ([0, 1, 2, 3, 4], [-1, -1, -1, 0, 1])
    tall = wide.T.copy()                                      # portrait: padded on the LEFT
    sq = cvlite.pad_to_square(tall)
    assert sq.shape == (5, 5) and not sq[:, :3].any() and np.array_equal(sq[:, 3:], tall)
    assert E.tables((5, 2), (5, 5)) == ([-1, -1, -1, 0, 1], [0, 1, 2, 3, 4])
    square = np.arange(1, 26, dtype=np.uint8).reshape(5, 5)   # a square hand is unchanged, and not resized at its own size
    assert np.array_equal(cvlite.pad_to_square(square), square)
    assert E.tables((5, 5), (5, 5)) == ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4])
    full = np.full((5, 5), 255, np.uint8)
    assert np.array_equal(cvlite.extract_affordance(full, square), square)
    for hw in ((2, 5), (5, 2), (5, 5), (3, 7), (9, 4)):
        for out_hw in ((5, 5), (7, 9), (12, 3)):
            c, r = ops.nearest_pad_tables(hw, out_hw)
            assert (c.tolist(), r.tolist()) == E.tables(hw, out_hw), (hw, out_hw)


def test_and_is_bitwise():
    one, two, three = (np.full((2, 2), v, np.uint8) for v in (1, 2, 3))
    assert not cvlite.extract_affordance(one, two).any() and not E.and_plane(one, two).any()        # 1 & 2 = 0
    assert (cvlite.extract_affordance(three, two) == 2).all() and (E.and_plane(three, two) == 2).all()
    assert (E.and_plane(one, two, logical=True) == 1).all()
    assert cvlite.process_affordance(cvlite.extract_affordance(one, two), 3) is None                # empty before the dilation


@pytest.mark.parametrize("shape", E.SHAPES, ids=lambda s: "%dx%d" % s)
def test_cvlite_equals_the_restatement(shape):
    """every shape, k and hand geometry of tests/test_extract_kernels_gpu.py"""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    planes, hands = E.planes(shape, rng), E.hands(shape, rng)
    for hname, hand in hands:
        for pname, plane in planes:
            if hname not in ("none", "same") and pname.startswith("lone"):
                continue
            a = E.and_plane(plane, hand)
            assert np.array_equal(a, plane if hand is None else cvlite.extract_affordance(plane, hand)), (pname, hname)
            for k in E.KS:
                want = E.process(a, k)
                got = cvlite.process_affordance(a, k)
                assert (got is None) == (want is None) and (want is None or np.array_equal(got, want)), (pname, hname, k)
                out, stats = dataset_build.HostRoute.host_item(plane, hand, k)
                assert stats == E.stats_of(a, E.dilate_white(a, k), hand is not None), (pname, hname, k)


def test_one_mistake_variants_differ_on_these_inputs():
    """each variant of the restatement, one rule wrong, is told apart by inputs the tests use: the inputs have teeth"""
    lone = _lone((12, 12), 5, 5)
    for k in (2, 4):                                          # a symmetric window for even k
        assert not np.array_equal(E.dilate_white(lone, k), E.dilate_white(lone, k, symmetric=True))
    for k in (1, 3, 7, 31):                                   # (odd k has one window only)
        assert np.array_equal(E.dilate_white(lone, k), E.dilate_white(lone, k, symmetric=True))
    stripes = np.zeros((6, 6), np.uint8)                      # the exact-rational nearest index
    stripes[:, 2] = 255
    full34 = np.full((9, 34), 255, np.uint8)
    assert not np.array_equal(E.and_plane(full34, stripes), E.and_plane(full34, stripes, exact=True))
    for hw in ((2, 5), (5, 2)):                               # padding on the bottom or right
        hand = np.full(hw, 255, np.uint8)
        full = np.full((5, 5), 255, np.uint8)
        assert not np.array_equal(E.and_plane(full, hand), E.and_plane(full, hand, pad_end=True))
    rng = np.random.default_rng(12)                           # a logical AND
    told_apart = []
    for shape in E.SHAPES:                                    # (a flat plane reads only the padding of a hand of its own shape)
        planes = dict(E.planes(shape, np.random.default_rng(shape[0] * 1000 + shape[1])))
        hands = dict(E.hands(shape, np.random.default_rng(shape[0] * 1000 + shape[1])))
        if not np.array_equal(E.and_plane(planes["ones_twos"], hands["twos_threes"]),
                              E.and_plane(planes["ones_twos"], hands["twos_threes"], logical=True)):
            told_apart.append(shape)
    assert set(told_apart) >= {(7, 7), (16, 64), (17, 65), (37, 131), (40, 132)}
    ones_twos = rng.integers(1, 3, (7, 7)).astype(np.uint8)
    assert not np.array_equal(E.and_plane(ones_twos, np.full((7, 7), 2, np.uint8)),
                              E.and_plane(ones_twos, np.full((7, 7), 2, np.uint8), logical=True))
    a, out, stats = E.extract(lone, None, 3)                  # emptiness counted after the dilation
    assert stats[0] == 1 and E.extract(lone, None, 3, count_after=True)[2][0] == 9
    assert stats[:3] == [1, 9, 255] and stats[3:7] == [4, 6, 4, 6] and stats[7] == 0
    assert E.extract(np.zeros((3, 4), np.uint8), None, 3)[2] == [0, 0, 0, 3, -1, 4, -1, 0]      # an empty plane: min > max
    assert E.extract(_lone((3, 4), 1, 1, v=7), np.full((3, 4), 5, np.uint8), 1)[2] == [1, 1, 5, 1, 1, 1, 1, 3]


# ---- create_dataset's rules --------------------------------------------------------------------------------------------------------

VERBS = [{"id": "0", "key": "take", "instances": "['take', 'pick-up', 'grab']"}, {"id": "1", "key": "put", "instances": "['put', 'place']"},
         {"id": "2", "key": "eat", "instances": "['eat', 'taste']"}, {"id": "3", "key": "uplift", "instances": "['up', 'raise']"}]
ALL4 = {"annotation.json", "inpainted_frame.png", "aff_left.png", "aff_right.png", "obj_left.png", "obj_right.png"}
LEFT = {"annotation.json", "inpainted_frame.png", "aff_left.png", "obj_left.png"}
RIGHT = {"annotation.json", "inpainted_frame.png", "aff_right.png", "obj_right.png"}
OK_SUM = 255 * 100


def _ann(**kw):
    a = {"taxonomy": [1, 0, 0, 0], "noun": "cup", "verb": "take", "narration": "take the cup", "obj_left": "cup", "obj_right": "pan"}
    a.update(kw)
    return a


def _valid(files, ann, sums, limit=30000, categories=("cup",)):
    return dataset_build.is_valid(set(files), ann, sums, limit, list(categories), VERBS, log=lambda *a: None)


def test_is_valid_rule_by_rule():
    both = {"left": OK_SUM, "right": OK_SUM}
    bi = _ann(taxonomy=[0, 0, 1, 0])
    assert _valid(LEFT, _ann(), both) == (True, "valid")
    assert _valid(ALL4, bi, both) == (True, "valid")
    assert _valid(LEFT - {"annotation.json"}, None, both) == (False, "missing_file")
    assert _valid(LEFT - {"inpainted_frame.png"}, _ann(), both) == (False, "missing_file")
    for key in ("noun", "verb", "narration"):
        assert _valid(LEFT, _ann(**{key: None}), both) == (False, "null_annotation")
    assert _valid(LEFT, _ann(verb="eat"), both) == (False, "verb_class")            # in the invalid list
    assert _valid(LEFT, _ann(verb="juggle"), both) == (False, "verb_class")         # in no row: the empty class
    # the substring rule: 'up' is an instance of row 3 but a SUBSTRING of 'pick-up' in row 0, and the first row wins
    assert dataset_build.map_verb_to_class("up", VERBS) == "take"
    assert dataset_build.map_verb_to_class("a", VERBS) == "take" and dataset_build.map_verb_to_class("tast", VERBS) == "eat"
    assert _valid(LEFT, _ann(verb="tast"), both) == (False, "verb_class")
    # bimanual: all four files, either object in the categories, both thresholds
    for f in ("aff_left.png", "aff_right.png", "obj_left.png", "obj_right.png"):
        assert _valid(ALL4 - {f}, bi, both) == (False, "missing_file")
    assert _valid(ALL4, bi, both, categories=("pan",)) == (True, "valid")
    assert _valid(ALL4, bi, both, categories=("knife",)) == (False, "category")
    assert _valid(ALL4, bi, both, categories=("knife", "all")) == (True, "valid")
    assert _valid(ALL4, bi, {"left": OK_SUM, "right": 255 * 20}) == (False, "threshold")
    assert _valid(ALL4, bi, {"left": 255 * 30000, "right": OK_SUM}) == (False, "threshold")
    # taxonomy[0] == 0 IS the bimanual case: a right-only annotation [0, 1, 0, 0] with the right pair alone is incomplete
    assert _valid(RIGHT, _ann(taxonomy=[0, 1, 0, 0]), both) == (False, "missing_file")
    # one hand: the left hand alone is tested when the left pair exists
    assert _valid(ALL4, _ann(), {"left": OK_SUM, "right": 0}) == (True, "valid")
    assert _valid(ALL4, _ann(obj_left="knife"), both) == (False, "category")
    assert _valid(RIGHT, _ann(obj_left="knife"), both, categories=("pan",)) == (True, "valid")
    assert _valid(RIGHT, _ann(), both, categories=("cup",)) == (False, "category")
    assert _valid(RIGHT, _ann(), both, categories=("all",)) == (True, "valid")
    assert _valid({"annotation.json", "inpainted_frame.png", "aff_left.png", "obj_right.png"}, _ann(), both) == (False, "missing_file")
    # check_threshold: 20 < white < limit, strict on both sides, white = sum / 255 as a float
    assert _valid(LEFT, _ann(), {"left": 255 * 20}) == (False, "threshold")
    assert _valid(LEFT, _ann(), {"left": 255 * 20 + 1}) == (True, "valid")
    assert _valid(LEFT, _ann(), {"left": 255 * 29999 + 254}) == (True, "valid")
    assert _valid(LEFT, _ann(), {"left": 255 * 30000}) == (False, "threshold")
    assert dataset_build.check_threshold(255 * 21, 30000) == (True, 21.0)


# ---- the subcommands on the host route ---------------------------------------------------------------------------------------------

def _run(argv, capsys):
    assert dataset_build.main(argv) == 0
    return capsys.readouterr().out


def test_subcommands_on_the_host_route(tmp_path, capsys):
    p = E.make_tree(tmp_path)
    aff = str(tmp_path / "A")
    out = _run(["extract_affordances", p["C"], p["H"], aff, "--route", "host"], capsys)
    assert f"Skipping zz_no_partner.png: No corresponding file in {os.path.join(p['H'], 'left')}" in out
    assert "Resizing s10_resized_hand.png to match dimensions of" in out
    assert f"Updated mask saved: {os.path.join(aff, 'left', 's00_bimanual.png')}" in out
    assert not os.path.exists(os.path.join(aff, "left", "zz_no_partner.png"))
    for side in ("left", "right"):
        for name in sorted(os.listdir(os.path.join(aff, side))):
            c, h = (np.array(Image.open(os.path.join(p[k], side, name))) for k in ("C", "H"))
            got = Image.open(os.path.join(aff, side, name))
            assert got.mode == "L" and np.array_equal(np.array(got), E.and_plane(c, h)), (side, name)
    before = {(s, n): np.array(Image.open(os.path.join(aff, s, n))) for s in ("left", "right") for n in os.listdir(os.path.join(aff, s))}
    out = _run(["process_affordances", aff, str(E.TREE_K), "--route", "host"], capsys)
    assert "1 empty masks deleted" in out
    assert not os.path.exists(os.path.join(aff, "left", "s03_empty_after_and.png"))
    for (side, name), a in before.items():
        want = E.process(a, E.TREE_K)
        path = os.path.join(aff, side, name)
        assert os.path.exists(path) == (want is not None)
        if want is not None:
            assert np.array_equal(np.array(Image.open(path)), want), (side, name)
    seq = E.assemble_sequences(p, aff, str(tmp_path / "seq"))
    args = ["--out", str(tmp_path / "out_c"), "--name", "set", "--limit", str(E.TREE_LIMIT), "--categories"] + E.TREE_CATEGORIES + \
           ["--verb-class-file", p["csv"], "--route", "host"]
    out = _run(["create_dataset", "--dir", seq] + args, capsys)
    n_valid = sum(v == "valid" for v in E.TREE_KINDS.values())
    assert f"Valid Frames Total:  {n_valid}" in out and f"Invalid Frames Total:  {len(E.TREE_KINDS) - n_valid}" in out
    assert f"{round(n_valid / len(E.TREE_KINDS) * 100, 2)}% were valid frames" in out
    assert "Verb not found" in out and "found invalid verb_class:  eat" in out and "h5 file is not written" in out
    assert "host_extracts" not in out and "host_walks" not in out
    with open(tmp_path / "out_c" / "jsons" / "set.json") as fh:
        data = json.load(fh)
    valid = [n for n, v in E.TREE_KINDS.items() if v == "valid"]
    assert list(data) == [str(i) for i in range(n_valid)]
    records = torch.load(tmp_path / "out_c" / "records" / "set.pt", weights_only=False)
    assert len(records) == n_valid
    for i, name in enumerate(valid):
        entry, rec = data[str(i)], records[i]
        assert list(entry) == ["original_size", "aff_left", "aff_right", "obj_left", "obj_right"] and entry["original_size"] == list(E.TREE_HW)
        with open(os.path.join(p["S"], name, "annotation.json")) as fh:
            ann = json.load(fh)
        assert rec["narration"] == ann["narration"] and rec["taxonomy"] == ann["taxonomy"] and rec["noun"] == ann["noun"]
        assert rec["verb"] == ann["verb"] and rec["obj_id_left"] == (ann["obj_left"] or "") and rec["obj_id_right"] == (ann["obj_right"] or "")
        assert np.array_equal(rec["image"], np.array(Image.open(os.path.join(p["S"], name, "inpainted_frame.png")).convert("RGB")))
        assert rec["masks"]["original_size"] == E.TREE_HW
        for side in ("left", "right"):
            f = os.path.join(seq, name, f"aff_{side}.png")
            for kind in ("aff", "obj"):
                key = f"{kind}_{side}"
                assert rec["masks"][key] == entry[key]
                if not os.path.exists(f):
                    assert entry[key] == []                   # a missing hand
                    continue
                plane = np.array(Image.open(os.path.join(seq, name, f"{kind}_{side}.png")))
                want = [c.reshape(-1, 2).tolist() for c in cvlite.find_contours_external(plane)]
                assert entry[key] == want and want
                assert np.array_equal(cvlite.draw_contours_filled(E.TREE_HW, entry[key], 1) != 0, E.fill_holes(plane))
    # the whole chain in one pass writes the same two files
    _run(["build", "--completed", p["C"], "--hand", p["H"], "--objects", p["O"], "--sequences", p["S"], "--k", str(E.TREE_K)] +
         ["--out", str(tmp_path / "out_b")] + args[2:] + ["--batch", "4"], capsys)
    assert E.tree_files(tmp_path / "out_b") == E.tree_files(tmp_path / "out_c")
    # OUT may be COMPLETED (misc/determine_mask_overlap.py): the completed masks are overwritten by the AND planes
    _run(["extract_affordances", p["C"], p["H"], p["C"], "--route", "host"], capsys)
    assert np.array_equal(np.array(Image.open(os.path.join(p["C"], "left", "s04_too_few.png"))), before[("left", "s04_too_few.png")])


def test_cli_refuses_bad_arguments(tmp_path):
    for argv in (["process_affordances", str(tmp_path), "0"], ["process_affordances", str(tmp_path), "32"],
                 ["process_affordances", str(tmp_path), "3", "--batch", "0"]):
        with pytest.raises(SystemExit):
            dataset_build.main(argv + ["--route", "host"])
    with pytest.raises(ValueError):
        dataset_build.make_route("cloud")


def test_entry_point_is_declared_and_exported():
    assert "haff_affordance_extract" in haff.EXPORTED_SYMBOLS
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "haff_hip.h")).read()
    assert "int haff_affordance_extract(" in text and "haff_extract_item" in text
    assert ops.AFF_EXTRACT_ITEM_WORDS * 8 == 64 and len(ops.AFF_EXTRACT_STATS) == 8
