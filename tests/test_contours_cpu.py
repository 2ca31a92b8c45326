"""Contour records, host side (no GPU): the two facts the extraction kernels rest on, on every fixture of tests/contours_ref.py; the
two entry points' declarations and every host-side refusal of haff_contour_extract; prediction_record through AffRecordsDataset;
the new flags' parsing, refusals and file protocol with a stub model."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import haff

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/contours_ref.py, tests/hausdorff_ref.py
import contours_ref as C   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("haff_contour_extract", "haff_contour_extract_workspace")


def test_start_rule_gives_every_contour_and_its_order():
    """One contour per component whose raster-first pixel is a start pixel, in descending raster order of that pixel, each the walk
    cvlite._follow makes from it."""
    from haff import cvlite
    most = 0
    for name, m in C.cpu_planes():
        found = C.contours(m)
        starts = C.starts_by_rule(m)
        assert len(starts) == len(found), name
        fg = np.pad(np.asarray(m) != 0, 1)
        for (x, y), c in zip(starts, found):
            pts, _ = cvlite._follow(fg, x + 1, y + 1)
            assert [(px - 1, py - 1) for px, py in pts] == [tuple(p) for p in c.reshape(-1, 2).tolist()], name
        most = max(most, len(found))
    assert most == 1024


def test_filled_contours_are_the_plane_with_its_holes_filled():
    from haff import cvlite
    for name, m in C.cpu_planes():
        if name.startswith("v"):
            continue                                            # hausdorff_ref's distance planes add nothing to this fact
        assert np.array_equal(cvlite.draw_contours_filled(m.shape, C.contours(m)), C.holes_filled(m)), name


def test_fixtures_are_what_their_names_say():
    p = C.new_planes()
    count = {name: len(C.contours(m)) for name, m in p.items()}
    assert count["nested"] == 1 and count["nested_255"] == 1 and count["four_edges"] == 5 and count["corners"] == 4
    assert count["seam_pair"] == 3 and count["seam_diagonal"] == 3 and count["isolated_grid"] == 1024
    assert count["empty"] == 0 and count["full"] == 1 and count["full_tile"] == 1 and count["over_lds"] == 3
    assert p["over_lds"].size > 1 << 20
    assert C.starts_by_rule(p["four_edges"])[0] == (10, 19) and (0, 8) in C.starts_by_rule(p["four_edges"])
    assert all(len(c) == 1 for c in C.contours(p["isolated_grid"]))
    s, o, v = C.expected(p["corners"])
    assert s.tolist() == [4, 4, 0, 0] and o.tolist() == [0, 1, 2, 3, 4] and v.tolist() == [[6, 5], [0, 5], [6, 0], [0, 0]]
    s, o, v = C.expected(p["empty"])
    assert s.tolist() == [0, 0, 0, 0] and o.tolist() == [0] and v.shape == (0, 2)


def test_declarations_equal_the_ctypes_prototypes():
    from haff import lib as hlib
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long}
    for name in NAMES:
        m = re.search(r"^int " + name + r"\((.*?)\);", text, flags=re.M | re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctype[p.replace("const ", "").split()[0]] for p in params]
        assert hlib._PROTOS[name] == want, (name, params)
        assert name in haff.EXPORTED_SYMBOLS
    assert len(hlib._PROTOS[NAMES[0]]) == 11 and len(hlib._PROTOS[NAMES[1]]) == 5


def _table(shapes):
    buf = np.zeros((2 * len(shapes) + 1,), np.int64)
    i32 = buf.view(np.int32)
    for i, (h, w) in enumerate(shapes):
        buf[2 * i] = 0x1000
        i32[4 * i + 2], i32[4 * i + 3] = h, w
    return buf, buf.ctypes.data


def test_host_side_refusals_before_any_launch():
    """No GPU and never-dereferenced device pointers: every refusal has to come from the host checks."""
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    lib = haff.load_library()
    f = 0x1000

    def need(shapes, max_contours=8, max_vertices=64):
        keep, planes = _table(shapes)
        out = ctypes.c_long(-7)
        rc = int(lib.haff_contour_extract_workspace(planes, len(shapes), max_contours, max_vertices, ctypes.addressof(out)))
        return rc, out.value

    def call(shapes=((5, 7), (9, 4)), max_contours=8, max_vertices=64, ws=f, ws_bytes=None, verts=f, offsets=f, summary=f,
             planes_dev=f, n_planes=None, null_host=False, shift_planes=0):
        keep, planes = _table(shapes)
        if ws_bytes is None:
            rc, size = need(shapes, max_contours, max_vertices)
            ws_bytes = size if rc == 0 else 1 << 30
        return int(lib.haff_contour_extract(None if null_host else planes + shift_planes, planes_dev,
                                            len(shapes) if n_planes is None else n_planes, max_contours, max_vertices, ws, ws_bytes,
                                            verts, offsets, summary, None))

    rc, size = need(((5, 7), (9, 4)))
    assert rc == 0 and size >= (5 * 7 + 9 * 4) * 4 + 2 * 2 * 8 * 4 and size % 16 == 0
    assert need(((5, 7),), 8)[1] < need(((5, 7),), 64)[1] < need(((5, 7), (9, 9)), 64)[1]
    assert need(((4096, 4096),))[0] == 0 and need(((4097, 5),))[0] == -2 and need(((5, 4097),))[0] == -2
    assert need(((0, 5),))[0] == -1 and need(((5, -1),))[0] == -1
    assert need(((5, 7),), 8, 0)[0] == -1 and need(((5, 7),), 8, (1 << 22) + 1)[0] == -1 and need(((5, 7),), 8, 1 << 22)[0] == 0
    assert need(((5, 7),), 0)[0] == -1 and need(((5, 7),), -3)[0] == -1 and need(((5, 7),), (1 << 22) + 1)[0] == -1
    assert need(((5, 7),), 1)[0] == 0 and need(((5, 7),), 1 << 22)[0] == 0
    assert int(lib.haff_contour_extract_workspace(_table(((5, 7),))[1], 1, 8, 64, None)) == -1
    assert int(lib.haff_contour_extract_workspace(None, 1, 8, 64, ctypes.addressof(ctypes.c_long()))) == -1
    # NULL table, workspace or outputs
    assert call(null_host=True) == -1 and call(planes_dev=None) == -1 and call(ws=None) == -1
    assert call(verts=None) == -1 and call(offsets=None) == -1 and call(summary=None) == -1
    # counts out of range
    assert call(n_planes=0) == -1 and call(n_planes=-1) == -1 and call(n_planes=4097) == -1
    # sides
    assert call(shapes=((0, 7),)) == -1 and call(shapes=((5, -2),)) == -1
    assert call(shapes=((4097, 2),)) == -2 and call(shapes=((2, 4097),)) == -2
    # capacities
    assert call(max_vertices=0) == -1 and call(max_vertices=-5) == -1 and call(max_vertices=(1 << 22) + 1) == -1
    assert call(max_contours=0) == -1 and call(max_contours=-1) == -1 and call(max_contours=(1 << 22) + 1) == -1
    # workspace size and alignment
    assert call(ws_bytes=size - 1) == -1 and call(ws_bytes=0) == -1 and call(ws=f + 8) == -1
    # misaligned outputs and tables
    assert call(verts=f + 2) == -1 and call(offsets=f + 2) == -1 and call(summary=f + 1) == -1 and call(planes_dev=f + 4) == -1
    assert call(shift_planes=4) == -1


# ---- records ----------------------------------------------------------------------------------------------------------------

def test_prediction_record_reads_back_as_the_hole_filled_planes():
    from haff import aff_dataset, config as hcfg, contours
    p = C.new_planes()
    left, right = p["nested"], np.zeros((21, 23), np.uint8)
    right[2:8, 0:5] = 1
    right[3:6, 1:3] = 0                                         # a hole: filled on the way back
    right[15:21, 18:23] = 1
    assert left.shape == right.shape == (21, 23)
    image = np.random.default_rng(3).integers(0, 256, (21, 23, 3), dtype=np.uint8)
    rec = contours.prediction_record("open the jar", image, 2, C.contours(left), C.contours(right), left.shape)
    assert rec["narration"] == "open the jar" and rec["taxonomy"] == 2 and rec["masks"]["original_size"] == (21, 23)
    assert rec["image"] is not None and np.array_equal(rec["image"], image)
    assert rec["masks"]["aff_left"] == [c.reshape(-1, 2).tolist() for c in C.contours(left)]
    assert all(type(v) is int for c in rec["masks"]["aff_right"] for pt in c for v in pt)
    gated = contours.prediction_record("x", image, 0, C.contours(left), [], left.shape)
    assert gated["masks"]["aff_right"] == []
    ds = aff_dataset.AffRecordsDataset([rec], hcfg.tiny(), seed=1)
    assert ds.original_size == (21, 23)
    item = ds[0]
    assert np.array_equal(item[4][0].numpy(), C.holes_filled(left)) and np.array_equal(item[5][0].numpy(), C.holes_filled(right))
    assert item[6] == [0.0, 0.0, 1.0, 0.0] and item[10] == ["open the jar"]
    assert np.array_equal(aff_dataset.recreate_mask_from_contours(gated["masks"]["aff_right"], (21, 23)), np.zeros((21, 23), np.uint8))


def test_reader_refuses_capacities_below_one():
    from haff import contours
    with pytest.raises(ValueError):
        contours.ContourReader(0, 5)
    with pytest.raises(ValueError):
        contours.ContourReader(5, 0)
    r = contours.ContourReader()
    assert (r.max_contours, r.max_vertices, r.host_walks) == (1024, 65536, 0) and r.read([]) == []


# ---- the flags ----------------------------------------------------------------------------------------------------------------

def test_inference_flag_parsing_and_refusals():
    from haff import inference
    base = ["--benchmark-dir", "b"]
    a = inference.parse_args(base)
    assert a.write_records is None and a.records_threshold == 0.5
    a = inference.parse_args(base + ["--write_records", "r.pt"])
    assert a.write_records == "r.pt" and a.records_threshold == 0.5 and not a.score
    a = inference.parse_args(base + ["--write_records", "r.pt", "--records_threshold", "0.3", "--score_only"])
    assert a.records_threshold == 0.3 and a.score and a.score_only
    a = inference.parse_args(base + ["--write_records", "r.pt", "--score"])
    assert a.score and not a.score_only
    with pytest.raises(SystemExit, match="--records_threshold modifies --write_records"):
        inference.parse_args(base + ["--records_threshold", "0.5"])
    with pytest.raises(SystemExit, match="--records_threshold 0.4: one of"):
        inference.parse_args(base + ["--write_records", "r.pt", "--records_threshold", "0.4"])
    with pytest.raises(SystemExit, match="--write_records needs --benchmark-dir"):
        inference.parse_args(["--write_records", "r.pt"])


class _HostReader:
    """ContourReader with the host walk in place of the kernels: what a flagged plane goes through."""
    made = []

    def __init__(self, *a, **kw):
        self.host_walks, self.reads = 0, []
        _HostReader.made.append(self)

    def read(self, planes):
        planes = list(planes)
        self.reads.append(len(planes))
        self.host_walks += len(planes)
        return [C.contours(p.numpy()) for p in planes]


class _Model:
    device = torch.device("cpu")

    def __init__(self, taxonomy):
        self.taxonomy, self.calls = taxonomy, 0

    def evaluate(self, images_clip, images, input_ids, resize_list, original_size_list, **kw):
        g = torch.Generator().manual_seed(5 + self.calls)
        self.calls += 1
        left = [torch.randn((1,) + tuple(s), generator=g) for s in original_size_list]
        right = [torch.randn((1,) + tuple(s), generator=g) - 1 for s in original_size_list]
        return input_ids, left, right, [torch.tensor([self.taxonomy]) for _ in original_size_list]


def _cpu_inference_planes(logits, taxonomy, side, thresholds):
    from haff import postprocess
    return torch.stack([(logits > postprocess.sigmoid_logit_threshold(t)).to(torch.uint8) * 255 for t in thresholds])


def _bench(folder, rng, n=3):
    from PIL import Image
    images = []
    for k in range(n):
        leaf = folder / "video" / f"{k:04d}"
        leaf.mkdir(parents=True)
        images.append(rng.integers(0, 256, (12 + k, 17, 3), dtype=np.uint8))
        Image.fromarray(images[-1]).save(leaf / "inpainting.png")
        (leaf / "annotation.json").write_text(json.dumps({"narration": f"action {k}"}))
    return images


@pytest.mark.parametrize("taxonomy,open_hands", [([0.1, 0.2, 0.6, 0.1], ("left", "right")), ([0.7, 0.1, 0.1, 0.1], ("left",)),
                                                 ([0.1, 0.7, 0.1, 0.1], ("right",))])
def test_write_records_with_a_stub_model(tmp_path, monkeypatch, taxonomy, open_hands):
    from PIL import Image
    from haff import aff_dataset, config as hcfg, contours, inference, postprocess
    from haff.checkpoint import ByteTokenizer
    cfg = hcfg.tiny()
    monkeypatch.setattr(inference, "build_model_and_tokenizer", lambda args: (_Model(taxonomy), ByteTokenizer(cfg), cfg, torch.float32))
    monkeypatch.setattr(postprocess, "inference_planes", _cpu_inference_planes)
    monkeypatch.setattr(contours, "ContourReader", _HostReader)
    del _HostReader.made[:]
    images = _bench(tmp_path / "bench", np.random.default_rng(4))
    path, vis = str(tmp_path / "records.pt"), str(tmp_path / "out" / "th")
    inference.main(["--benchmark-dir", str(tmp_path / "bench"), "--vis_save_path", vis, "--batch-size", "2", "--write_records", path,
                    "--records_threshold", "0.3"])
    assert len(_HostReader.made) == 1 and _HostReader.made[0].reads == [2 * len(open_hands), len(open_hands)]   # one read per chunk
    records = torch.load(path, weights_only=False)
    assert len(records) == 3
    for k, rec in enumerate(records):
        assert rec["narration"] == f"action {k}" and np.array_equal(rec["image"], images[k])
        assert rec["taxonomy"] == int(np.argmax(taxonomy)) and tuple(rec["masks"]["original_size"]) == (12 + k, 17)
        for side in ("left", "right"):
            png = os.path.join(vis + "0.3", "video", f"{k:04d}", f"aff_{side}.png")
            if side not in open_hands:
                assert rec["masks"]["aff_" + side] == [] and not os.path.exists(png)
                continue
            plane = np.asarray(Image.open(png))
            assert rec["masks"]["aff_" + side] == [c.reshape(-1, 2).tolist() for c in C.contours(plane)]
            assert len(rec["masks"]["aff_" + side]) > 0
    ds = aff_dataset.AffRecordsDataset(records, cfg, seed=0)
    assert ds.size == 3 and len(ds[0]) == 12
    # without the flag: the same PNGs, no records, no reader
    del _HostReader.made[:]
    inference.main(["--benchmark-dir", str(tmp_path / "bench"), "--vis_save_path", str(tmp_path / "plain" / "th"), "--batch-size", "2"])
    assert _HostReader.made == []
    for th in postprocess.THRESHOLDS:
        for k in range(3):
            for side in open_hands:
                a, b = (os.path.join(str(tmp_path / d / "th") + str(th), "video", f"{k:04d}", f"aff_{side}.png") for d in ("out", "plain"))
                assert open(a, "rb").read() == open(b, "rb").read()


def test_robot_demo_contours_flag_with_a_stub_model(tmp_path, monkeypatch):
    from PIL import Image
    import robot_ref
    from haff import config as hcfg, contours, postprocess, robot_demo
    from haff.checkpoint import ByteTokenizer
    cfg = hcfg.tiny()
    assert robot_demo.CONTOURS_FLAG == "--contours"
    with pytest.raises(SystemExit):
        robot_demo.parse_args(["--contours"])                   # an option of the loop, not of parse_args

    def planes(logits, th, margins, and_masks, on_value=255):
        heat = np.stack([robot_ref.heatmap(x) for x in logits.numpy()])
        masks = np.stack([robot_ref.pad_and_mask(x, th, margins, m.numpy()) for x, m in zip(logits.numpy(), and_masks)])
        return torch.from_numpy(heat), torch.from_numpy(masks)
    monkeypatch.setattr(robot_demo, "build_model_and_tokenizer", lambda args: (_Model([0.1, 0.6, 0.2, 0.1]), ByteTokenizer(cfg), cfg,
                                                                               torch.float32))
    monkeypatch.setattr(postprocess, "robot_planes", planes)
    monkeypatch.setattr(contours, "ContourReader", _HostReader)
    outs = {}
    for flag in ((), ("--contours",)):
        inp, out = tmp_path / ("in" + str(len(flag))), tmp_path / ("out" + str(len(flag)))
        inp.mkdir()
        Image.fromarray(np.full((20, 24, 3), 7, np.uint8)).save(inp / "img.png")
        (inp / "prompt.txt").write_text("pick up the cup\n")
        (inp / "margins.txt").write_text("2,-1,3,4")
        for side in ("left", "right"):
            Image.fromarray(np.random.default_rng(9).integers(0, 256, (23, 29), dtype=np.uint8)).save(inp / f"mask_{side}.png")
        del _HostReader.made[:]
        robot_demo.main(["--zed2_img_path", str(inp), "--vis_save_path", str(out), "--poll-interval", "0", "--force_both", "--th", "0"]
                        + list(flag), max_requests=1)
        outs[len(flag)] = out
        assert len(_HostReader.made) == len(flag)
    base = {"cropped_img.png", "aff_left.png", "aff_right.png", "aff_left_heat.png", "aff_right_heat.png"}
    assert set(os.listdir(outs[0])) == base and set(os.listdir(outs[1])) == base | {"aff_left.json", "aff_right.json"}
    for name in base:
        assert open(outs[0] / name, "rb").read() == open(outs[1] / name, "rb").read()
    for side in ("left", "right"):
        plane = np.asarray(Image.open(outs[1] / f"aff_{side}.png"))
        got = json.load(open(outs[1] / f"aff_{side}.json"))
        assert got == {"original_size": [23, 29], "contours": [c.reshape(-1, 2).tolist() for c in C.contours(plane)]}
        assert len(got["contours"]) > 0
