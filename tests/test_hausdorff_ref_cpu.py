"""The device Hausdorff route, host side (no GPU): the expected values the GPU tests compare against (tests/hausdorff_ref.py) agree
with evaluation.calculate_hausdorff and with the start-pixel rule the kernels implement; the new flag's parsing and refusals; the
two entry points' declarations; every host-side refusal of haff_contour_hausdorff."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

import haff

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/hausdorff_ref.py
import hausdorff_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("haff_contour_hausdorff", "haff_contour_hausdorff_workspace")


def test_integer_distances_with_the_empty_rules_equal_calculate_hausdorff():
    """math.sqrt(d2) on the integer distances, with the two empty rules, is evaluation.calculate_hausdorff to the bit."""
    seen = set()
    for bench, pred in R.cpu_pairs():
        row = R.expected_row(R.vertices(bench), R.vertices(pred))
        got, want = R.distances(row, bench.shape), R.calculate_hausdorff(bench, pred)
        assert got == want and [type(v) for v in got] == [type(v) for v in want], (bench.shape, row, got, want)
        seen.add((row[0] > 0, row[1] > 0))
        assert row[2] <= 2 * 4095 ** 2 and row[3] <= 2 * 4095 ** 2
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    wide = R.wide_planes()
    assert R.expected_row(R.vertices(wide[0]), R.vertices(wide[1]))[2:4] == [4095 ** 2 + 1, 4095 ** 2 + 1]


def test_start_pixel_rule_reproduces_the_first_contour():
    """[0] is the outer border of the component found by the rule (maximum over the candidates of their component's raster-first
    pixel), on every fixture; the walk from that pixel is cvlite._follow's."""
    from haff import cvlite
    n_with = 0
    for name, m in R.all_cpu_fixtures():
        v = R.vertices(m)
        start = R.start_by_rule(m)
        assert (start is None) == (len(v) == 0), name
        if start is None:
            continue
        n_with += 1
        assert R.component_first_pixel(m, tuple(v[0])) == start, name
        pts, _ = cvlite._follow(np.pad(m != 0, 1), start[0] + 1, start[1] + 1)
        assert [(x - 1, y - 1) for x, y in pts] == [tuple(p) for p in v.tolist()], name
    assert n_with > 80


def test_fixtures_are_what_their_names_say():
    p = R.small_planes()
    assert R.vertices(p["full"]).tolist() == [[0, 0], [0, 4], [6, 4], [6, 0]]
    assert R.vertices(p["one_on"]).tolist() == [[0, 0]] and len(R.vertices(p["one_off"])) == 0 and len(R.vertices(p["empty"])) == 0
    assert R.vertices(p["pixel_last"]).tolist() == [[6, 4]] and R.vertices(p["row_1x7"]).tolist() == [[0, 0], [6, 0]]
    assert R.vertices(p["column_7x1"]).tolist() == [[0, 0], [0, 6]]
    assert R.start_by_rule(p["two_blobs"]) == (5, 6)
    trap = p["trap"]
    assert R.start_by_rule(trap) == (6, 3)                     # A, although ...
    ys, xs = np.nonzero(trap)
    assert R.component_first_pixel(trap, (int(xs[-1]), int(ys[-1]))) == (1, 1)   # ... the last pixel in raster order is on B
    assert R.start_by_rule(p["ring_with_blob"]) == (1, 1) and R.start_by_rule(p["ring"]) == (1, 1)
    assert R.vertices(p["ring"]).tolist() == R.vertices(p["ring_with_blob"]).tolist()
    assert R.start_by_rule(p["corner_touch"]) == (1, 1) and R.start_by_rule(p["diamond_with_pixel"]) == (4, 1)
    t = R.TILE
    for h, w in ((t - 1, t - 1), (t, t), (t + 1, t + 1), (t + 1, 2 * t + 1), (2 * t + 3, 4 * t + 1)):
        assert len(R.vertices(p[f"spiral_centre_{h}x{w}"])) == 1              # the pixel at the end of the channel is external ...
        assert R.start_by_rule(p[f"spiral_sealed_{h}x{w}"]) == (0, 0)         # ... unless the channel's mouth is closed
        assert R.start_by_rule(p[f"comb_{h}x{w}"]) == (0, 0) and R.start_by_rule(p[f"comb_down_{h}x{w}"]) == (0, 0)
    c = R.CHUNK
    d = R.distance_planes()
    assert [len(R.vertices(d[f"v{v}"])) for v in (1, 2, c - 1, c, c + 1, 3 * c + 1)] == [1, 2, c - 1, c, c + 1, 3 * c + 1]
    assert len(R.vertices(R.many_vertices(26, (8, 128)))) == 26
    tie = R.vertices(d["tie"])[0]
    assert len({int(((tie - q) ** 2).sum()) for q in R.vertices(d["v2"])}) == 1


def test_flag_parsing_and_refusals():
    from haff import inference
    base = ["--benchmark-dir", "b"]
    a = inference.parse_args(base)
    assert a.score_hausdorff_device is False
    a = inference.parse_args(base + ["--score_only", "--score_hausdorff_device"])
    assert a.score and a.score_only and a.score_hausdorff_device and not a.score_hausdorff
    a = inference.parse_args(base + ["--score", "--score_hausdorff_device", "--score_cropped"])
    assert a.score and not a.score_only and a.score_hausdorff_device
    a = inference.parse_args(base + ["--score", "--score_hausdorff"])
    assert a.score_hausdorff and not a.score_hausdorff_device
    with pytest.raises(SystemExit, match="--score_hausdorff_device modifies --score"):
        inference.parse_args(base + ["--score_hausdorff_device"])
    with pytest.raises(SystemExit, match="--score_hausdorff_device and --score_hausdorff"):
        inference.parse_args(base + ["--score", "--score_hausdorff", "--score_hausdorff_device"])
    with pytest.raises(SystemExit, match="--benchmark-dir"):
        inference.parse_args(["--score_only", "--score_hausdorff_device"])


def test_scorer_options_without_a_device():
    from haff import scoring
    s = scoring.BenchmarkScorer("b", "cpu", hausdorff="device", max_vertices=7)
    assert s.hausdorff and s.hausdorff_device and s._pool is None and s.host_walks == 0 and s.max_vertices == 7
    s = scoring.BenchmarkScorer("b", "cpu", hausdorff=True)
    assert s.hausdorff and not s.hausdorff_device and s._pool is not None
    s.close()
    s = scoring.BenchmarkScorer("b", "cpu")
    assert not s.hausdorff and not s.hausdorff_device and s._pool is None
    with pytest.raises(ValueError):
        scoring.BenchmarkScorer("b", "cpu", hausdorff="host")


def test_declarations_equal_the_ctypes_prototypes():
    from haff import lib as hlib
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name in NAMES:
        m = re.search(r"^int " + name + r"\((.*?)\);", text, flags=re.M | re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctype[p.replace("const ", "").split()[0]] for p in params]
        assert hlib._PROTOS[name] == want, (name, params)
        assert name in haff.EXPORTED_SYMBOLS
    assert len(hlib._PROTOS[NAMES[0]]) == 12


def _tables(shapes, pairs):
    """Host tables as ops.contour_hausdorff lays them out: 16-byte plane descriptors (never-dereferenced plane pointers), int32
    pairs. Returns (keep-alive array, planes address, pairs address)."""
    n = len(shapes)
    buf = np.zeros((2 * n + len(pairs) + 1,), np.int64)
    i32 = buf.view(np.int32)
    for i, (h, w) in enumerate(shapes):
        buf[2 * i] = 0x1000
        i32[4 * i + 2], i32[4 * i + 3] = h, w
    i32[4 * n:4 * n + 2 * len(pairs)] = np.asarray(pairs, np.int32).reshape(-1)
    return buf, buf.ctypes.data, buf.ctypes.data + 16 * n


def test_host_side_refusals_before_any_launch():
    """No GPU and never-dereferenced device pointers: every refusal has to come from the host checks."""
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    lib = haff.load_library()
    f = 0x1000

    def need(shapes, max_vertices=64):
        keep, planes, _ = _tables(shapes, [(0, 0)])
        out = ctypes.c_long(-7)
        rc = int(lib.haff_contour_hausdorff_workspace(planes, len(shapes), max_vertices, ctypes.addressof(out)))
        return rc, out.value

    def call(shapes=((5, 7), (5, 7)), pairs=((0, 1),), max_vertices=64, ws=f, ws_bytes=None, verts=None, result=f, planes_dev=f,
             pairs_dev=f, n_planes=None, n_pairs=None, null_host=None, shift_planes=0, shift_pairs=0):
        keep, planes, prs = _tables(shapes, pairs)
        if ws_bytes is None:
            ws_bytes = need(shapes, max_vertices)[1] if need(shapes, max_vertices)[0] == 0 else 1 << 30
        planes, prs = planes + shift_planes, prs + shift_pairs
        if null_host == "planes":
            planes = None
        if null_host == "pairs":
            prs = None
        return int(lib.haff_contour_hausdorff(planes, planes_dev, len(shapes) if n_planes is None else n_planes, prs, pairs_dev,
                                              len(pairs) if n_pairs is None else n_pairs, max_vertices, ws, ws_bytes, verts, result,
                                              None))

    rc, size = need(((5, 7), (5, 7)))
    assert rc == 0 and size >= 2 * 5 * 7 * 4 + 2 * 64 * 4 + 2 * 4 and size % 16 == 0
    assert need(((5, 7),), 64)[1] < need(((5, 7),), 128)[1] < need(((5, 7), (9, 9)), 128)[1]
    assert need(((4096, 4096),))[0] == 0 and need(((4097, 5),))[0] == -2 and need(((5, 4097),))[0] == -2
    assert need(((0, 5),))[0] == -1 and need(((5, -1),))[0] == -1
    assert need(((5, 7),), 0)[0] == -1 and need(((5, 7),), (1 << 22) + 1)[0] == -1 and need(((5, 7),), 1 << 22)[0] == 0
    assert int(lib.haff_contour_hausdorff_workspace(_tables(((5, 7),), [(0, 0)])[1], 1, 64, None)) == -1
    assert int(lib.haff_contour_hausdorff_workspace(None, 1, 64, ctypes.addressof(ctypes.c_long()))) == -1
    # NULL tables, workspace or result
    assert call(null_host="planes") == -1 and call(null_host="pairs") == -1 and call(planes_dev=None) == -1
    assert call(pairs_dev=None) == -1 and call(result=None) == -1 and call(ws=None) == -1
    # counts out of range
    assert call(n_planes=0) == -1 and call(n_planes=-1) == -1 and call(n_planes=4097) == -1
    assert call(n_pairs=0) == -1 and call(n_pairs=-3) == -1 and call(n_pairs=65536) == -1
    # sides
    assert call(shapes=((0, 7), (0, 7))) == -1 and call(shapes=((5, -2), (5, -2))) == -1
    assert call(shapes=((4097, 2), (4097, 2))) == -2 and call(shapes=((2, 4097), (2, 4097))) == -2
    # max_vertices
    assert call(max_vertices=0) == -1 and call(max_vertices=-5) == -1 and call(max_vertices=(1 << 22) + 1) == -1
    # workspace size and alignment
    assert call(ws_bytes=size - 1) == -1 and call(ws_bytes=0) == -1 and call(ws=f + 8) == -1
    # misaligned result, tables and vertex buffer
    assert call(result=f + 2) == -1 and call(planes_dev=f + 4) == -1 and call(pairs_dev=f + 2) == -1 and call(verts=f + 2) == -1
    assert call(shift_planes=4) == -1 and call(shift_pairs=2) == -1
    # pairs: an index outside the table, two shapes
    assert call(pairs=((0, 2),)) == -1 and call(pairs=((-1, 1),)) == -1 and call(pairs=((0, 1), (2, 0))) == -1
    assert call(shapes=((5, 7), (7, 5))) == -1 and call(shapes=((5, 7), (5, 8))) == -1


def test_empty_rules_by_hand():
    assert R.distances([0, 0, 0, 0, 0, 0], (3, 4)) == (5.0, 5.0) and R.distances([4, 0, 0, 0, 0, 0], (3, 4)) == (5.0, 5.0)
    assert R.distances([0, 4, 0, 0, 0, 0], (3, 4)) == (0, 0)
    assert R.distances([2, 2, 9, 16, 0, 0], (3, 4)) == (3.0, 4.0) and R.distances([2, 2, 16, 9, 0, 0], (3, 4)) == (4.0, 4.0)
    assert R.distances([2, 2, 2, 1, 0, 0], (3, 4)) == (math.sqrt(2), math.sqrt(2))
