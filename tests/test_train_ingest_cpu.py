"""Device-side training ingest, the parts that need no GPU: the C-ABI wiring of haff_fill_contours_u8, the --device_ingest flag,
the rng order of raw_item, collate_fn after its text half moved into a shared helper (against values recorded before the move),
the Prefetcher, and the CPU restatement of the fill kernel (tests/contour_ref.py) against cvlite.draw_contours_filled."""
import json
import os
import re
import sys
import threading

import numpy as np
import pytest
import torch

import haff
from haff import aff_dataset, checkpoint, config as hcfg, cvlite, prompt as hprompt, train_ds

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/contour_ref.py
import contour_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "collate_fn_fixed_batch.npz")


# ---- C-ABI wiring ----------------------------------------------------------------------------------------------------------
def test_fill_contours_symbol_is_declared_exported_and_typed():
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    m = re.search(r"^int haff_fill_contours_u8\(([^;]*)\);", text, flags=re.M | re.S)
    assert m, "include/haff_hip.h does not declare haff_fill_contours_u8"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert "haff_fill_contours_u8" in haff.EXPORTED_SYMBOLS
    from haff import lib as hlib
    proto = hlib._PROTOS["haff_fill_contours_u8"]
    assert len(proto) == len(params) == 10
    for p, t in zip(params, proto):
        assert t is (hlib.c_void_p if "*" in p else hlib.c_int), (p, t)
    lib = haff.load_library()
    assert lib.haff_fill_contours_u8.argtypes == proto
    src = open(os.path.join(ROOT, "2handedafforder_amd", "csrc", "Makefile")).read()
    assert "contour_fill.hip" in src


def test_entry_point_refuses_bad_arguments_on_the_host():
    """Nothing is launched for these: the refusals are host arithmetic (no GPU here, and none needed)."""
    import ctypes
    lib = haff.load_library()

    def call(polys, plane_of, n_planes, hw=(8, 8), out=1):
        off = np.zeros(len(polys) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(p) for p in polys])
        pts = np.asarray([v for p in polys for v in p], dtype=np.int32).reshape(-1, 2)
        pl = np.asarray(plane_of, dtype=np.int32)
        return int(lib.haff_fill_contours_u8(pts.ctypes.data, off.ctypes.data, pl.ctypes.data, ctypes.c_void_p(64), len(polys),
                                             n_planes, ctypes.c_void_p(out), hw[0], hw[1], None))
    tri = [[1, 1], [5, 1], [3, 5]]
    assert call([tri], [0], 0) == -1 and call([tri], [0], 1, hw=(0, 8)) == -1 and call([tri], [0], 1, out=0) == -1
    assert call([tri], [1], 1) == -1 and call([tri], [-1], 1) == -1                       # plane out of range
    assert call([[[0, 0]] * (R.MAX_VERTS + 1)], [0], 1) == -1                              # too many vertices
    assert call([[[1, 1], [R.MAX_COORD, 1], [3, 5]]], [0], 1) == -1                        # coordinate out of range
    assert call([[[1, 1], [5, -R.MAX_COORD], [3, 5]]], [0], 1) == -1


# ---- the flag --------------------------------------------------------------------------------------------------------------
def test_device_ingest_defaults_to_off():
    assert train_ds.parse_args([]).device_ingest is False
    assert train_ds.parse_args(["--device_ingest"]).device_ingest is True


def test_device_ingest_is_refused_with_synthetic_by_name(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device before refusing the flags")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(SystemExit) as e:
        train_ds.main(["--device_ingest", "--synthetic", "tiny"])
    assert "--device_ingest" in str(e.value) and "--synthetic" in str(e.value)


# ---- datasets --------------------------------------------------------------------------------------------------------------
def _records(n=5, hw=(48, 64), seed=0):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        x, y = 4 + 3 * i, 5 + 2 * i
        recs.append({"narration": f"Action Number {i} with the tool", "inpainted": rng.integers(0, 255, hw + (3,), dtype=np.uint8),
                     "taxonomy": i % 4, "masks": {"aff_left": [[[x, y], [x + 20, y + 2], [x + 12, y + 18]]],
                                                  "aff_right": [] if i % 2 else [[[30, 10], [50, 12], [45, 30], [28, 28]]],
                                                  "original_size": hw}})
    return recs


def test_raw_item_draws_from_the_rng_in_getitem_order():
    cfg = hcfg.tiny()
    a = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11)
    b = aff_dataset.AffRecordsDataset(_records(), cfg, seed=11)
    for i in range(6):
        item, raw = a[i], b.raw_item(i)
        assert raw["conversations"] == item[3] and raw["questions"] == item[9] and raw["texts"] == item[10]
        assert raw["inference"] is item[11] and raw["taxonomy"] == item[6]
        assert raw["mask_hw"] == tuple(item[4].shape[1:]) and raw["frame"].dtype == np.uint8 and raw["frame"].shape == (48, 64, 3)
        for side, plane in (("left", item[4]), ("right", item[5])):     # the record drawn is the same: its contours fill to the mask
            assert np.array_equal(cvlite.draw_contours_filled(raw["mask_hw"], raw["contours_" + side]), plane[0].numpy())
    assert a.rng.getstate() == b.rng.getstate()


def test_val_raw_item_draws_from_the_rng_in_getitem_order():
    cfg = hcfg.tiny()
    root = os.path.join(ROOT, "tests", "golden", "actaffordance_sample")
    a, b = aff_dataset.AffValDataset(root, cfg, seed=5), aff_dataset.AffValDataset(root, cfg, seed=5)
    for i in range(4):
        item, raw = a[i], b.raw_item(i)
        assert raw["conversations"] == item[3] and raw["questions"] == item[9] and raw["inference"] is True
        assert np.array_equal(raw["plane_left"], item[4][0].numpy()) and np.array_equal(raw["plane_right"], item[5][0].numpy())
        assert raw["mask_hw"] == tuple(item[4].shape[1:])


# ---- collate_fn keeps its output -----------------------------------------------------------------------------------------------
def _fixed_batch(conv_type, inference):
    """Hand-made 12-tuples (collate_fn does not care where they come from): small tensors, conversations of different lengths."""
    g = torch.Generator().manual_seed(21)
    batch = []
    for i, text in enumerate(["cut the bread", "open the very large bottle with both hands", "lift"]):
        convs = []
        for k in range(1 + (i == 1)):                      # the middle sample carries two conversations
            conv = hprompt.get_conv(conv_type)
            conv.append_message(conv.roles[0], aff_dataset.SHORT_QUESTION_LIST[(i + k) % 4].format(class_name=text))
            conv.append_message(conv.roles[1], aff_dataset.ANSWER_LIST[(2 * i + k) % 5])
            convs.append(conv.get_prompt())
        tax = [0.0] * 4
        tax[i] = 1.0
        label = {"left": torch.zeros(6, 7, dtype=torch.int64), "right": torch.zeros(6, 7, dtype=torch.int64)}
        batch.append((None if i else "a/b.png", torch.randn((3, 8, 8), generator=g), torch.randn((3, 4, 4), generator=g), convs,
                      (torch.rand((1, 6, 7), generator=g) > 0.5).to(torch.uint8), (torch.rand((1, 6, 7), generator=g) > 0.5).to(torch.uint8),
                      tax, label, (8, 6 + i), [text + "?"], [text], inference))
    return batch


COLLATE_CASES = [("llava_v1", False, 575), ("llava_v1", False, 400), ("llava_v1", True, 575), ("llava_llama_2", False, 575)]


def _collate_flat(case):
    conv_type, inference, max_len = case
    out = train_ds.collate_fn(_fixed_batch(conv_type, inference), checkpoint.ByteTokenizer(hcfg.tiny()), max_len, conv_type=conv_type)
    arrays, meta = {}, {}
    for k, v in out.items():
        if torch.is_tensor(v):
            arrays[k] = v.numpy()
            meta[k] = ["tensor", str(v.dtype)]
        elif k in ("masks_list_left", "masks_list_right"):
            arrays[k] = torch.stack(v).numpy()
            meta[k] = ["tensor_list", str(v[0].dtype)]
        elif k == "label_list":
            meta[k] = [{s: [list(t.shape), str(t.dtype)] for s, t in d.items()} for d in v]
        else:
            meta[k] = json.loads(json.dumps(v))
    return arrays, meta


def record_golden():
    """Run ONCE on the commit before the refactor: python tests/test_train_ingest_cpu.py"""
    blob = {}
    for n, case in enumerate(COLLATE_CASES):
        arrays, meta = _collate_flat(case)
        for k, a in arrays.items():
            blob[f"c{n}.{k}"] = a
        blob[f"c{n}.meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(GOLDEN, **blob)


@pytest.mark.parametrize("n", range(len(COLLATE_CASES)))
def test_collate_fn_output_is_what_it_was_before_the_text_half_moved(n):
    gold = np.load(GOLDEN)
    arrays, meta = _collate_flat(COLLATE_CASES[n])
    want_meta = json.loads(bytes(gold[f"c{n}.meta"]).decode())
    assert json.loads(json.dumps(meta, sort_keys=True)) == want_meta
    want_keys = {k.split(".", 1)[1] for k in gold.files if k.startswith(f"c{n}.") and not k.endswith(".meta")}
    assert set(arrays) == want_keys
    for k, a in arrays.items():
        w = gold[f"c{n}.{k}"]
        assert a.dtype == w.dtype and a.shape == w.shape and np.array_equal(a, w), k
    if COLLATE_CASES[n][2] == 400:
        assert arrays["input_ids"].shape[1] == 400 - 255          # the truncation is exercised


def test_collate_text_is_collate_fns_own_code():
    """The helper both paths call gives the text entries of collate_fn's dict."""
    tok = checkpoint.ByteTokenizer(hcfg.tiny())
    batch = _fixed_batch("llava_v1", False)
    full = train_ds.collate_fn(batch, tok, 400)
    text = train_ds.collate_text([c for b in batch for c in b[3]], tok, 400, inference=False, offsets=[0, 1, 3, 4])
    for k in ("input_ids", "labels", "attention_masks", "offset"):
        assert torch.equal(full[k], text[k]), k
    assert full["conversation_list"] == text["conversation_list"]


# ---- Prefetcher ------------------------------------------------------------------------------------------------------------
def _live_prefetch_threads():
    return [t for t in threading.enumerate() if t.name.startswith("haff-prefetch") and t.is_alive()]


def test_prefetcher_keeps_order_and_ends_its_thread():
    from haff.train_ingest import Prefetcher
    seen = []

    def fetch(i):
        seen.append(i)
        return ("item", i)
    pf = Prefetcher(fetch, start=7, batch_size=4, prepare=lambda raws: len(raws))
    got = []
    for _ in range(5):
        raws, prepared = pf.get()
        assert prepared == 4
        got += [r[1] for r in raws]
    assert got == list(range(7, 27))                      # 20 indices, in order
    assert seen[:20] == list(range(7, 27)) and seen == list(range(7, 7 + len(seen)))   # one producer: consecutive, never re-ordered
    assert len(seen) <= 20 + 3 * 4                        # two batches ahead (plus the one being made), not the whole epoch
    pf.close()
    assert not _live_prefetch_threads()
    pf.close()                                            # idempotent


def test_prefetcher_reraises_a_producer_exception_and_ends():
    from haff.train_ingest import Prefetcher

    def fetch(i):
        if i == 5:
            raise KeyError("record 5 is broken")
        return i
    pf = Prefetcher(fetch, start=0, batch_size=2)
    assert pf.get()[0] == [0, 1] and pf.get()[0] == [2, 3]
    with pytest.raises(KeyError, match="record 5 is broken"):
        pf.get()
    with pytest.raises(KeyError):                         # and stays failed
        pf.get()
    pf.close()
    assert not _live_prefetch_threads()


def test_prefetcher_close_unblocks_a_full_queue():
    from haff.train_ingest import Prefetcher
    pf = Prefetcher(lambda i: i, start=0, batch_size=1)   # nobody consumes: the producer fills the queue and blocks on it
    pf.close()
    assert not _live_prefetch_threads()
    with pytest.raises(RuntimeError):
        pf.get()


# ---- the kernel's algorithm on the CPU --------------------------------------------------------------------------------------------
def test_closed_form_line_equals_line8_for_every_small_offset():
    for dx in range(-40, 41):
        for dy in range(-40, 41):
            img = np.zeros((100, 100), np.uint8)
            cvlite._line8(img, 50, 50, 50 + dx, 50 + dy, 1)
            img2 = np.zeros((100, 100), np.uint8)
            px = R.line_pixels(50, 50, 50 + dx, 50 + dy)
            assert len(px) == max(abs(dx), abs(dy)) + 1
            for x, y in px:
                img2[y, x] = 1
            assert np.array_equal(img, img2), (dx, dy)


def test_row_parallel_fill_equals_cvlite_on_random_and_named_cases():
    cases = R.random_cases(300, 0)
    assert len(cases) == 300 and {hw for hw, _ in cases} == {(48, 64), (33, 47), (64, 64)}
    for hw, cs in cases + list(R.named_cases().values()):
        assert np.array_equal(R.fill_planes([cs], hw)[0], cvlite.draw_contours_filled(hw, cs)), (hw, cs)
    hw, planes = R.MULTI_PLANE
    got = R.fill_planes(planes, hw)
    for i, cs in enumerate(planes):
        assert np.array_equal(got[i], cvlite.draw_contours_filled(hw, cs))
    assert max(len(R.row_spans([tuple(p) for p in R.comb()], y)) for y in range(5, 36)) == 40      # 80 crossings on a row


if __name__ == "__main__":
    record_golden()
