"""haff_contour_extract (csrc/contour_hausdorff.hip, ops.contour_extract, haff.contours.ContourReader) against the host route
(tests/contours_ref.py: cvlite.find_contours_external flattened), exact equality everywhere; the capacities' edges; and the two CLIs'
new outputs against the host contours of the PNGs the same run wrote."""
import itertools
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/contours_ref.py, tests/hausdorff_ref.py
import contours_ref as C   # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")
FILL = 0x5A
_EXPECTED = {}


def _expected():
    """[(name, plane, (summary, offsets, verts))] of the mixed-shape call, computed once."""
    if "all" not in _EXPECTED:
        _EXPECTED["all"] = [(name, m, C.expected(m)) for name, m in C.device_planes()]
    return _EXPECTED["all"]


def _buffers(torch, dev, n, max_contours, max_vertices, guard=0):
    """0x5A-filled (summary, offsets, verts) for n planes, each a view `guard` rows inside a larger filled buffer; and the buffers."""
    whole = [torch.full((n + 2 * guard,) + tail, FILL, dtype=torch.uint8, device=dev)
             for tail in ((16,), (4 * (max_contours + 1),), (4 * max_vertices,))]
    s = whole[0][guard:guard + n].view(torch.int32)
    o = whole[1][guard:guard + n].view(torch.int32)
    v = whole[2][guard:guard + n].view(torch.int16).reshape(n, max_vertices, 2)
    return (s, o, v), whole


def _check_plane(name, want, summary, offsets, verts):
    """One plane's rows (numpy, offsets and verts as uint8 views too) against the expectation: the used prefixes equal it and
    everything past them still holds the fill."""
    ws, wo, wv = want
    assert summary.tolist() == ws.tolist(), (name, summary.tolist(), ws.tolist())
    nc, nv = int(ws[0]), int(ws[1])
    assert offsets[:nc + 1].tolist() == wo.tolist(), name
    assert np.array_equal(verts[:nv], wv), name
    assert (offsets[nc + 1:].view(np.uint8) == FILL).all(), name
    assert (verts[nv:].reshape(-1).view(np.uint8) == FILL).all(), name


def test_every_contour_of_every_fixture_in_one_call(dev):
    import torch
    from haff import ops
    exp = _expected()
    n = len(exp)
    max_contours = max(int(e[0][0]) for _, _, e in exp) + 1
    max_vertices = max(int(e[0][1]) for _, _, e in exp) + 1
    assert max_contours == 1025 and len({m.shape for _, m, _ in exp}) > 10
    planes = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for _, m, _ in exp]
    runs = []
    for _ in range(2):
        out, whole = _buffers(torch, dev, n, max_contours, max_vertices)
        got = ops.contour_extract(planes, max_contours, max_vertices, out=out)
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        runs.append([w.cpu().numpy() for w in whole])
    summary = runs[0][0].view(np.int32)
    offsets = runs[0][1].view(np.int32)
    verts = runs[0][2].view(np.int16).reshape(n, max_vertices, 2)
    for i, (name, _, want) in enumerate(exp):
        _check_plane(name, want, summary[i], offsets[i], verts[i])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                              # a second run is bitwise equal
    # the default buffers: the same through the allocating path
    s, o, v = ops.contour_extract(planes[:12], max_contours, max_vertices)
    assert np.array_equal(s.cpu().numpy(), summary[:12])


@pytest.mark.parametrize("name", ["four_edges", "noise1"])
def test_capacities_at_their_edges(dev, name):
    import torch
    from haff import contours, ops
    m = dict((k, p) for k, p, _ in _expected())[name]
    want = dict((k, e) for k, _, e in _expected())[name]
    n_c, n_v = int(want[0][0]), int(want[0][1])
    assert n_c >= 3 and n_v > n_c
    plane = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
    host = C.contours(m)
    for max_contours, max_vertices in itertools.product((n_c - 1, n_c, n_c + 1), (n_v - 1, n_v, n_v + 1)):
        out, whole = _buffers(torch, dev, 1, max_contours, max_vertices, guard=2)
        ops.contour_extract([plane], max_contours, max_vertices, out=out)
        s, o, v = (w.cpu().numpy() for w in whole)
        for w in (s, o, v):
            assert (w[:2] == FILL).all() and (w[3:] == FILL).all(), (max_contours, max_vertices)   # nothing outside the plane's rows
        summary = s[2].view(np.int32)
        if max_contours < n_c:
            # too many contours: none is walked, so the vertex total is not taken and bit 0 stays clear
            assert summary.tolist() == [n_c, summary[1], C.TOO_MANY, 0], (max_contours, max_vertices, summary.tolist())
        elif max_vertices < n_v:
            assert summary.tolist() == [n_c, n_v, C.OVERFLOW, 0], (max_contours, max_vertices, summary.tolist())
            assert (o[2].view(np.int32)[n_c + 1:].view(np.uint8) == FILL).all()
        else:
            _check_plane(name, want, summary, o[2].view(np.int32), v[2].view(np.int16).reshape(max_vertices, 2))
        reader = contours.ContourReader(max_contours, max_vertices)
        got = reader.read([plane, plane])
        assert reader.host_walks == (2 if max_contours < n_c or max_vertices < n_v else 0)
        for g in got:
            assert len(g) == len(host) and all(a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b)
                                               for a, b in zip(g, host))


# ---- the CLIs -----------------------------------------------------------------------------------------------------------------

@pytest.fixture
def forced(monkeypatch):
    """Random-init models never emit [SEG]; force one so the mask branch of the CLIs runs (as tests/test_hausdorff_cli_gpu.py)."""
    import torch
    import haff  # noqa: F401
    from haff import lisa
    orig = lisa.LisaMI355.evaluate

    def evaluate(self, *a, **kw):
        B = a[2].shape[0]
        kw["forced_answer"] = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]]).expand(B, -1)
        kw["max_new_tokens"] = 3
        return orig(self, *a, **kw)
    monkeypatch.setattr(lisa.LisaMI355, "evaluate", evaluate)


def _lists(plane):
    return [c.reshape(-1, 2).tolist() for c in C.contours(plane)]


@pytest.mark.timeout(600)
def test_inference_write_records(dev, tmp_path, forced):
    import torch
    from PIL import Image
    from haff import aff_dataset, config as hcfg, inference
    bench = tmp_path / "bench"
    leaves = (("P14_05", "0001413"), ("8f91bc0d-9ce7-4b31-aba7-dd59791917df", "00000029"))
    for sub, leaf in leaves:
        shutil.copytree(os.path.join(SAMPLE, sub, leaf), bench / sub / leaf)
    common = ["--synthetic", "tiny", "--benchmark-dir", str(bench), "--image_size", "224", "--batch-size", "3"]
    path, vis = str(tmp_path / "records.pt"), str(tmp_path / "out" / "th")
    assert inference.main(common + ["--vis_save_path", vis, "--write_records", path, "--records_threshold", "0.3"]) is None
    records = torch.load(path, weights_only=False)
    assert len(records) == 2
    walked = 0
    for rec, (sub, leaf) in zip(records, sorted(leaves)):     # the directory walk's order
        frame = np.asarray(Image.open(bench / sub / leaf / "inpainting.png").convert("RGB"))
        assert rec["narration"] == json.load(open(bench / sub / leaf / "annotation.json"))["narration"]
        assert np.array_equal(rec["image"], frame) and tuple(rec["masks"]["original_size"]) == frame.shape[:2]
        assert rec["taxonomy"] in (0, 1, 2, 3)
        for side, blank in (("left", 1), ("right", 0)):
            png = os.path.join(vis + "0.3", sub, leaf, f"aff_{side}.png")
            assert os.path.exists(png) == (rec["taxonomy"] != blank), (side, rec["taxonomy"])
            if rec["taxonomy"] == blank:
                assert rec["masks"]["aff_" + side] == []       # a gated hand
                continue
            assert rec["masks"]["aff_" + side] == _lists(np.asarray(Image.open(png))), (sub, side)
            walked += 1
    assert walked >= 2
    ds = aff_dataset.AffRecordsDataset(records, hcfg.tiny(), seed=0)
    item = ds[0]
    assert ds.size == 2 and item[4].shape[1:] == item[5].shape[1:] and item[4].dtype == torch.uint8
    # --score_only: the same records and no PNG
    path2 = str(tmp_path / "records_only.pt")
    rep = inference.main(common + ["--vis_save_path", str(tmp_path / "none" / "th"), "--write_records", path2, "--records_threshold",
                                   "0.3", "--score_only"])
    assert rep is not None and not os.path.exists(tmp_path / "none")
    again = torch.load(path2, weights_only=False)
    assert len(again) == len(records)
    for a, b in zip(again, records):
        assert a["narration"] == b["narration"] and a["taxonomy"] == b["taxonomy"] and a["masks"] == b["masks"]
        assert np.array_equal(a["image"], b["image"])


@pytest.mark.timeout(600)
def test_robot_demo_contours(dev, tmp_path, forced):
    from PIL import Image
    from haff import robot_demo
    rng = np.random.default_rng(12)
    H, W, margins = 150, 224, (3, -2, 5, 1)
    Ho, Wo = H + margins[1] + margins[3], W + margins[0] + margins[2]
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks = {s: rng.integers(0, 256, (Ho, Wo), dtype=np.uint8) for s in ("left", "right")}
    outs = []
    for k, flag in enumerate(([], ["--contours"])):
        inp, out = tmp_path / f"in{k}", tmp_path / f"out{k}"
        inp.mkdir()
        Image.fromarray(img).save(inp / "img.png")
        (inp / "prompt.txt").write_text("open the drawer\n")
        (inp / "margins.txt").write_text("3,-2,5,1\n")
        for s, m in masks.items():
            Image.fromarray(m).save(inp / f"mask_{s}.png")
        robot_demo.main(["--synthetic", "tiny", "--zed2_img_path", str(inp), "--vis_save_path", str(out), "--force_both",
                         "--image_size", "224", "--poll-interval", "0"] + flag, max_requests=1)
        outs.append(out)
    pngs = {"cropped_img.png", "aff_left.png", "aff_right.png", "aff_left_heat.png", "aff_right_heat.png"}
    assert set(os.listdir(outs[0])) == pngs and set(os.listdir(outs[1])) == pngs | {"aff_left.json", "aff_right.json"}
    for name in pngs:
        assert open(outs[0] / name, "rb").read() == open(outs[1] / name, "rb").read(), name
    for side in ("left", "right"):
        plane = np.asarray(Image.open(outs[1] / f"aff_{side}.png"))
        assert plane.shape == (Ho, Wo)
        assert json.load(open(outs[1] / f"aff_{side}.json")) == {"original_size": [Ho, Wo], "contours": _lists(plane)}, side
