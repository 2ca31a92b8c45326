"""dataset_build on the device route against its host route on a generated tree (tests/extract_ref.py make_tree: about a dozen
sequences at 48 x 64, one of every kind): `build` and the three subcommands write byte-equal files, nothing goes through the host
fallbacks, the records load in AffRecordsDataset with the object crop on, and a record's contours re-fill to the dilated plane."""
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/extract_ref.py
import extract_ref as E   # noqa: E402

pytestmark = pytest.mark.gpu


def _records_equal(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert list(ra) == list(rb)
        for key in ra:
            if key == "image":
                assert ra[key].dtype == rb[key].dtype and np.array_equal(ra[key], rb[key])
            else:
                assert ra[key] == rb[key], key


def _chain(D, p, root, route_name, dataset_args):
    """extract -> process -> (assemble the sequence folders) -> create_dataset under root, one route object per step"""
    aff = os.path.join(root, "A")
    routes = [D.make_route(route_name) for _ in range(3)]
    D.extract_affordances(p["C"], p["H"], aff, routes[0], batch=5, log=lambda *a: None)
    and_planes = E.tree_files(aff)
    D.process_affordances(aff, E.TREE_K, routes[1], batch=5)
    seq = E.assemble_sequences(p, aff, os.path.join(root, "seq"))
    res = D.create_dataset(seq, os.path.join(root, "out_c"), "set", *dataset_args, routes[2], batch=5, log=lambda *a: None)
    return and_planes, res, routes


def test_device_route_writes_what_the_host_route_writes(dev, tmp_path):
    import torch
    from haff import config as hcfg
    from haff import cvlite
    from haff import dataset_build as D
    from haff.aff_dataset import AffRecordsDataset
    p = E.make_tree(tmp_path / "tree")
    args = (E.TREE_LIMIT, E.TREE_CATEGORIES, p["csv"])
    out, routes = {}, {}
    for name in ("host", "device"):
        root = str(tmp_path / name)
        os.makedirs(root)
        routes[name] = D.make_route(name)
        res_b = D.build(p["C"], p["H"], p["O"], p["S"], E.TREE_K, os.path.join(root, "out_b"), "set", *args, routes[name], batch=5,
                        log=lambda *a: None)
        and_planes, res_c, chain_routes = _chain(D, p, root, name, args)
        routes[name + "_chain"] = chain_routes
        assert res_b == res_c
        out[name] = {"and": and_planes, "files": E.tree_files(root), "res": res_b}
    kinds = list(E.TREE_KINDS.values())
    assert out["host"]["res"]["reasons"] == {k: kinds.count(k) for k in sorted(set(kinds))}
    assert out["device"]["res"] == out["host"]["res"]
    # byte for byte: the AND PNGs, the processed PNGs, the assembled sequences, both JSON files, both record files
    assert sorted(out["device"]["files"]) == sorted(out["host"]["files"]) and out["device"]["and"] == out["host"]["and"]
    assert any(f.startswith(os.path.join("A", "left")) for f in out["host"]["files"])
    for f, data in out["host"]["files"].items():
        if not f.endswith(".pt"):
            assert out["device"]["files"][f] == data, f
    assert out["host"]["files"][os.path.join("out_b", "jsons", "set.json")] == out["host"]["files"][os.path.join("out_c", "jsons", "set.json")]
    loaded = {n: {o: torch.load(tmp_path / n / o / "records" / "set.pt", weights_only=False) for o in ("out_b", "out_c")}
              for n in ("host", "device")}
    for a, b in ((loaded["device"]["out_b"], loaded["host"]["out_b"]), (loaded["device"]["out_c"], loaded["host"]["out_c"]),
                 (loaded["device"]["out_b"], loaded["device"]["out_c"])):
        _records_equal(a, b)
    # nothing left the device
    for r in [routes["device"]] + routes["device_chain"]:
        assert r.host_extracts == 0 and r.host_walks == 0 and r.reader.host_walks == 0
    records = loaded["device"]["out_b"]
    assert len(records) == kinds.count("valid")
    sample = AffRecordsDataset(records, hcfg.tiny(), aug_crop=1.0, seed=0)[0]
    assert sample is not None and len(sample) == 12
    # a record's aff_left contours re-fill to the dilated plane with its holes filled (s00: a ring whose hole survives k = 3)
    first = records[0]
    plane = np.array(Image.open(tmp_path / "device" / "A" / "left" / "s00_bimanual.png"))
    c, h = (np.array(Image.open(os.path.join(p[k], "left", "s00_bimanual.png"))) for k in ("C", "H"))
    assert np.array_equal(plane, E.extract(c, h, E.TREE_K)[1])
    filled = cvlite.draw_contours_filled(first["masks"]["original_size"], first["masks"]["aff_left"], 1) != 0
    assert np.array_equal(filled, E.fill_holes(plane)) and not np.array_equal(filled, plane != 0)


def test_grey_and_planes_and_the_cli(dev, tmp_path, capsys):
    """extract_affordances keeps grey values: the kernel writes the recoloured plane, so an AND plane of other values than 0 / 255
    is written from cvlite and counted; the CLI prints the counter. A 0 / 255 tree prints none."""
    from haff import dataset_build as D
    trees = {}
    for name in ("host", "device"):
        for k in ("C", "H"):
            os.makedirs(tmp_path / name / k / "left")
            os.makedirs(tmp_path / name / k / "right")
        rng = np.random.default_rng(5)
        Image.fromarray(rng.integers(0, 4, (9, 13)).astype(np.uint8)).save(tmp_path / name / "C" / "left" / "g.png")
        Image.fromarray(np.full((13, 13), 7, np.uint8)).save(tmp_path / name / "H" / "left" / "g.png")
        Image.fromarray((rng.random((9, 13)) < 0.5).astype(np.uint8) * 255).save(tmp_path / name / "C" / "right" / "w.png")
        Image.fromarray(np.full((5, 5), 255, np.uint8)).save(tmp_path / name / "H" / "right" / "w.png")
        assert D.main(["extract_affordances", str(tmp_path / name / "C"), str(tmp_path / name / "H"), str(tmp_path / name / "A"),
                       "--route", name]) == 0
        text = capsys.readouterr().out
        assert ("host_extracts: 1 planes" in text) == (name == "device") and "host_walks" not in text
        trees[name] = E.tree_files(tmp_path / name / "A")
    assert trees["host"] == trees["device"] and len(trees["host"]) == 2
    grey = np.array(Image.open(tmp_path / "device" / "A" / "left" / "g.png"))
    assert set(np.unique(grey)) <= {0, 1, 2, 3} and grey.max() > 1
