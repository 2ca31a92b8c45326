"""The mask and contour family's host-side contract (no GPU): which inputs each entry point refuses, and with WHICH code — -1 (bad
argument) or -2 (a geometry the kernels do not serve) — and how much workspace the two contour entry points ask for. The order of the
checks is part of the contract: an input that breaks a -1 rule and a -2 rule at once gets the code of the rule checked first. Every
call below is refused before anything is launched (the host descriptor tables are real, the device addresses fake and never
dereferenced); no case would pass validation. The expected codes and byte counts were recorded from the library as it stood before the
host halves of contour_hausdorff.hip, mask_score.hip, affordance_extract.hip, robot_post.hip and mask_smooth.hip were reorganised
around one plane plan and one alignment helper; they are not derived from the code under test."""
import ctypes
import os

import numpy as np
import pytest

import haff

F = 0x10000         # 16-byte aligned, never dereferenced
BAD, UNS = -1, -2
_KEEP = []          # the host tables of the cases below: alive for the module's lifetime


def host(words, dtype=np.int64, skew=0):
    """The address of a host table holding `words` (16-byte aligned, or `skew` bytes past such a boundary)"""
    raw = np.zeros(np.asarray(words, dtype=dtype).nbytes + 32, dtype=np.uint8)
    _KEEP.append(raw)
    off = (-raw.ctypes.data) % 16 + skew
    raw[off:off + raw.size - 32] = np.asarray(words, dtype=dtype).view(np.uint8).reshape(-1)
    return raw.ctypes.data + off


def planes(*hw, skew=0):
    """haff_contour_plane [n]: {plane, H, W}"""
    t = np.zeros((len(hw), 2), dtype=np.int64)
    for i, (h, w) in enumerate(hw):
        t[i, 0] = F + 0x1000000 * i
        t[i].view(np.int32)[2:4] = (h, w)
    return host(t, skew=skew)


def score_frames(*frames, skew=0):
    """haff_score_frame [n] from dicts: logit / tax / gt / obj / out pointers, Hs Ws Hb Wb n_tax, gt_hw obj_hw"""
    t = np.zeros((len(frames), 16), dtype=np.int64)
    for i, over in enumerate(frames):
        f = dict(logit=(F, F), tax=F, gt=(F, F), obj=(0, 0), out=F, Hs=64, Ws=48, Hb=32, Wb=24, n_tax=4, gt_hw=None, obj_hw=(0, 0, 0, 0))
        f.update(over)
        t[i, :8] = list(f["logit"]) + [f["tax"]] + list(f["gt"]) + list(f["obj"]) + [f["out"]]
        gt_hw = f["gt_hw"] or (f["Hb"], f["Wb"]) * 2
        t[i].view(np.int32)[16:29] = [f["Hs"], f["Ws"], f["Hb"], f["Wb"], f["n_tax"]] + list(gt_hw) + list(f["obj_hw"])
    return host(t, skew=skew)


def items(*its, skew=0):
    """haff_extract_item [n] from dicts: in hand col row out, H W Hh Wh"""
    t = np.zeros((len(its), 8), dtype=np.int64)
    for i, over in enumerate(its):
        it = dict({"in": F, "hand": 0, "col": 0, "row": 0, "out": 2 * F, "H": 32, "W": 24, "Hh": 0, "Wh": 0}, **over)
        t[i, :5] = [it["in"], it["hand"], it["col"], it["row"], it["out"]]
        t[i].view(np.int32)[10:14] = [it["H"], it["W"], it["Hh"], it["Wh"]]
    return host(t, skew=skew)


HAND = dict(hand=F, col=F, row=F, Hh=20, Wh=30)
PAIRS = host([0, 1], np.int32)
TRI_PTS, TRI_OFF, TRI_PLANE = host([0, 0, 5, 0, 0, 5], np.int32), host([0, 3], np.int32), host([0], np.int32)
CROP_DESC = host(np.zeros(24, dtype=np.int32), np.int32)     # two samples, neither cropped nor mirrored
BYTES = host([0])

# entry point -> (argument order, a base argument set that every case below spoils)
ENTRY = {
    "haff_contour_hausdorff": (("planes_host", "planes_dev", "n_planes", "pairs_host", "pairs_dev", "n_pairs", "max_vertices", "workspace",
                                "workspace_bytes", "verts_out", "result", "stream"),
                               dict(planes_host=planes((32, 24), (32, 24)), planes_dev=F, n_planes=2, pairs_host=PAIRS, pairs_dev=F, n_pairs=1,
                                    max_vertices=64, workspace=F, workspace_bytes=1 << 30, verts_out=None, result=F, stream=None)),
    "haff_contour_hausdorff_workspace": (("planes_host", "n_planes", "max_vertices", "bytes_out"),
                                         dict(planes_host=planes((32, 24), (32, 24)), n_planes=2, max_vertices=64, bytes_out=BYTES)),
    "haff_contour_extract": (("planes_host", "planes_dev", "n_planes", "max_contours", "max_vertices", "workspace", "workspace_bytes", "verts",
                              "offsets", "summary", "stream"),
                             dict(planes_host=planes((32, 24), (7, 3)), planes_dev=F, n_planes=2, max_contours=8, max_vertices=64, workspace=F,
                                  workspace_bytes=1 << 30, verts=F, offsets=F, summary=F, stream=None)),
    "haff_contour_extract_workspace": (("planes_host", "n_planes", "max_contours", "max_vertices", "bytes_out"),
                                       dict(planes_host=planes((32, 24), (7, 3)), n_planes=2, max_contours=8, max_vertices=64, bytes_out=BYTES)),
    "haff_score_masks": (("frames_host", "frames_dev", "n_frames", "thresholds_host", "n_th", "counts", "stream"),
                         dict(frames_host=score_frames({}, {}), frames_dev=F, n_frames=2, thresholds_host=host([0.0, 0.5], np.float32), n_th=2,
                              counts=F, stream=None)),
    "haff_affordance_extract": (("items_host", "items_dev", "n_items", "k", "stats", "stream"),
                                dict(items_host=items({}, HAND), items_dev=F, n_items=2, k=5, stats=F, stream=None)),
    "haff_fill_contours_u8": (("pts", "poly_off", "poly_plane", "desc_dev", "n_poly", "n_planes", "out", "H", "W", "stream"),
                              dict(pts=TRI_PTS, poly_off=TRI_OFF, poly_plane=TRI_PLANE, desc_dev=F, n_poly=1, n_planes=1, out=F, H=32, W=24,
                                   stream=None)),
    "haff_crop_resample_u8": (("in", "out", "B", "H", "W", "C", "desc_host", "desc_dev", "desc_words", "stream"),
                              {"in": F, "out": 0x4000000, "B": 2, "H": 32, "W": 24, "C": 3, "desc_host": CROP_DESC, "desc_dev": F,
                               "desc_words": 24, "stream": None}),
    "haff_robot_heatmap": (("logits", "n", "H", "W", "jet_rgb", "workspace", "workspace_floats", "out", "stream"),
                           dict(logits=F, n=2, H=32, W=24, jet_rgb=F, workspace=F, workspace_floats=1024, out=F, stream=None)),
    "haff_robot_mask": (("logits", "H0", "W0", "left", "top", "right", "bottom", "th", "mask", "mask_h", "mask_w", "on_value", "out", "stream"),
                        dict(logits=F, H0=32, W0=24, left=1, top=2, right=3, bottom=4, th=0.5, mask=F, mask_h=38, mask_w=28, on_value=255,
                             out=F, stream=None)),
    "haff_mask_quantile7": (("logits", "n", "H", "W", "need", "out", "stream"), dict(logits=F, n=2, H=32, W=24, need=32768, out=2 * F, stream=None)),
}

PLANE_TABLE = [
    (dict(planes_host=None), BAD), (dict(planes_host=planes((32, 24), (32, 24), skew=4)), BAD), (dict(n_planes=0), BAD),
    (dict(n_planes=4097), BAD), (dict(max_vertices=0), BAD), (dict(max_vertices=(1 << 22) + 1), BAD),
    (dict(planes_host=planes((32, 24), (0, 24))), BAD), (dict(planes_host=planes((32, 0), (32, 24))), BAD),
    (dict(planes_host=planes((4097, 24), (4097, 24))), UNS), (dict(planes_host=planes((32, 24), (32, 4097))), UNS),
    # a -1 rule and a -2 rule at once: the counts come before the planes, and the planes are read in order
    (dict(planes_host=planes((4097, 24), (4097, 24)), max_vertices=0), BAD), (dict(planes_host=planes((4097, 24), (4097, 24)), n_planes=4097), BAD),
    (dict(planes_host=planes((4097, 24), (0, 24))), UNS), (dict(planes_host=planes((0, 24), (4097, 24))), BAD)]
TOO_TALL = dict(planes_host=planes((4097, 24), (4097, 24)))
CASES = {
    "haff_contour_hausdorff_workspace": PLANE_TABLE + [(dict(bytes_out=None), BAD), (dict(TOO_TALL, bytes_out=None), BAD)],
    "haff_contour_extract_workspace": PLANE_TABLE + [
        (dict(bytes_out=None), BAD), (dict(max_contours=0), BAD), (dict(max_contours=(1 << 22) + 1), BAD), (dict(TOO_TALL, max_contours=0), UNS)],
    "haff_contour_hausdorff": PLANE_TABLE + [
        (dict(planes_dev=None), BAD), (dict(pairs_host=None), BAD), (dict(pairs_dev=None), BAD), (dict(result=None), BAD),
        (dict(workspace=None), BAD), (dict(n_pairs=0), BAD), (dict(n_pairs=65536), BAD), (dict(planes_dev=F + 4), BAD),
        (dict(pairs_host=PAIRS + 2), BAD), (dict(pairs_dev=F + 2), BAD), (dict(result=F + 2), BAD), (dict(workspace=F + 8), BAD),
        (dict(verts_out=F + 2), BAD), (dict(workspace_bytes=6928 - 1), BAD), (dict(workspace_bytes=0), BAD),
        (dict(pairs_host=host([0, 2], np.int32)), BAD), (dict(pairs_host=host([-1, 0], np.int32)), BAD),
        (dict(planes_host=planes((32, 24), (24, 32))), BAD),
        # the plane table is judged before the other operands' alignment, the pair count before the plane table
        (dict(TOO_TALL, workspace=F + 8), UNS), (dict(TOO_TALL, workspace_bytes=0), UNS), (dict(TOO_TALL, n_pairs=0), BAD),
        (dict(TOO_TALL, result=None), BAD)],
    "haff_contour_extract": PLANE_TABLE + [
        (dict(planes_dev=None), BAD), (dict(workspace=None), BAD), (dict(verts=None), BAD), (dict(offsets=None), BAD), (dict(summary=None), BAD),
        (dict(max_contours=0), BAD), (dict(max_contours=(1 << 22) + 1), BAD), (dict(planes_dev=F + 4), BAD), (dict(workspace=F + 8), BAD),
        (dict(verts=F + 2), BAD), (dict(offsets=F + 2), BAD), (dict(summary=F + 2), BAD), (dict(workspace_bytes=3600 - 1), BAD),
        (dict(TOO_TALL, max_contours=0), UNS), (dict(TOO_TALL, verts=F + 2), UNS), (dict(TOO_TALL, verts=None), BAD)],
    "haff_score_masks": [
        (dict(frames_host=None), BAD), (dict(frames_dev=None), BAD), (dict(thresholds_host=None), BAD), (dict(counts=None), BAD),
        (dict(n_frames=0), BAD), (dict(n_frames=65536), BAD), (dict(n_th=0), BAD), (dict(n_th=9), BAD),
        (dict(frames_host=score_frames({}, {}, skew=4)), BAD), (dict(frames_dev=F + 4), BAD), (dict(counts=F + 2), BAD),
        (dict(frames_host=score_frames({}, dict(Hs=0))), BAD), (dict(frames_host=score_frames(dict(Wb=0), {})), BAD),
        (dict(frames_host=score_frames({}, dict(Hb=4097))), UNS), (dict(frames_host=score_frames(dict(Ws=4097), {})), UNS),
        (dict(frames_host=score_frames({}, dict(n_tax=0))), BAD), (dict(frames_host=score_frames({}, dict(n_tax=1025))), BAD),
        (dict(frames_host=score_frames({}, dict(logit=(F, F + 2)))), BAD), (dict(frames_host=score_frames({}, dict(tax=F + 2))), BAD),
        (dict(frames_host=score_frames({}, dict(gt_hw=(32, 24, 32, 25)))), BAD),
        (dict(frames_host=score_frames({}, dict(obj=(F, 0), obj_hw=(24, 32, 0, 0)))), BAD),
        # a frame's sides are judged before its pointers, the frames in order, and the threshold count before any frame
        (dict(frames_host=score_frames({}, dict(Hb=4097, logit=(F + 2, F)))), UNS), (dict(frames_host=score_frames({}, dict(Hb=4097, Ws=0))), BAD),
        (dict(frames_host=score_frames(dict(Hb=4097), dict(Hs=0))), UNS), (dict(frames_host=score_frames(dict(Hs=0), dict(Hb=4097))), BAD),
        (dict(frames_host=score_frames({}, dict(Hb=4097)), n_th=9), BAD), (dict(frames_host=score_frames({}, dict(Hb=4097)), counts=F + 2), BAD)],
    "haff_affordance_extract": [
        (dict(items_host=None), BAD), (dict(items_dev=None), BAD), (dict(stats=None), BAD), (dict(n_items=0), BAD), (dict(n_items=65536), BAD),
        (dict(items_host=items({}, HAND, skew=4)), BAD), (dict(items_dev=F + 4), BAD), (dict(stats=F + 4), BAD), (dict(k=0), UNS), (dict(k=32), UNS),
        (dict(items_host=items({}, {"in": 0})), BAD), (dict(items_host=items({}, dict(H=0))), BAD), (dict(items_host=items(dict(out=F), {})), BAD),
        (dict(items_host=items({}, dict(HAND, col=0))), BAD), (dict(items_host=items({}, dict(HAND, row=0))), BAD),
        (dict(items_host=items({}, dict(HAND, Hh=0))), BAD), (dict(items_host=items({}, dict(HAND, col=F + 2))), BAD),
        (dict(items_host=items({}, dict(HAND, Wh=4097))), UNS), (dict(items_host=items({}, dict(W=4097))), UNS),
        # the window's side is judged after the table's own operands and before any item; an item's own -1 rules before its sides
        (dict(k=32, stats=F + 4), BAD), (dict(k=0, n_items=0), BAD), (dict(k=32, items_host=items(dict(out=F), {})), UNS),
        (dict(items_host=items({}, dict(W=4097, out=F))), BAD), (dict(items_host=items({}, dict(HAND, col=0, H=4097))), BAD),
        (dict(items_host=items({}, dict(HAND, Wh=4097, H=0))), BAD), (dict(items_host=items(dict(W=4097), dict(H=0))), UNS)],
    "haff_fill_contours_u8": [
        (dict(n_poly=-1), BAD), (dict(n_planes=0), BAD), (dict(H=0), BAD), (dict(W=0), BAD), (dict(H=32769), BAD), (dict(W=32769), BAD),
        (dict(out=None), BAD), (dict(pts=None), BAD), (dict(poly_off=None), BAD), (dict(poly_plane=None), BAD), (dict(desc_dev=None), BAD),
        (dict(poly_off=host([1, 3], np.int32)), BAD), (dict(poly_off=host([0, -1], np.int32)), BAD), (dict(poly_off=host([0, 4097], np.int32)), BAD),
        (dict(poly_plane=host([1], np.int32)), BAD), (dict(poly_plane=host([-1], np.int32)), BAD),
        (dict(pts=host([0, 0, 32768, 0, 0, 5], np.int32)), BAD), (dict(pts=host([0, 0, 5, -32768, 0, 5], np.int32)), BAD)],
    "haff_crop_resample_u8": [
        ({"in": None}, BAD), (dict(out=None), BAD), (dict(desc_host=None), BAD), (dict(desc_dev=None), BAD), (dict(B=0), BAD), (dict(B=65536), BAD),
        (dict(H=0), BAD), (dict(W=0), BAD), (dict(C=2), BAD), (dict(desc_host=CROP_DESC + 2), BAD), (dict(desc_dev=F + 2), BAD),
        (dict(desc_words=23), BAD), (dict(H=4096, W=4097), UNS), (dict(H=1048561, W=1), UNS), (dict(out=F), BAD), (dict(out=F + 4607), BAD),
        (dict(desc_host=host([0] * 7 + [2] + [0] * 16, np.int32)), BAD),
        (dict(desc_host=host([0, 0, 25, 32, 0, 0, 32, 4] + [0] * 16, np.int32)), BAD),         # a box wider than the frame
        (dict(desc_host=host([0, 0, 24, 32, 0, 0, 24, 4] + [0] * 16, np.int32)), BAD),         # S is not the longer side
        (dict(desc_host=host([0, 0, 24, 32, 0, 0, 32, 4, 24, 1, 24, 1] + [0] * 12, np.int32)), BAD),   # tables past the descriptor
        (dict(H=4, W=4, desc_host=host([0, 0, 1, 4, 0, 0, 4, 4] + [0] * 16, np.int32)), BAD),   # a served box, tables of no taps
        (dict(H=32, W=7, desc_host=host([0, 0, 7, 32, 0, 0, 32, 4] + [0] * 16, np.int32)), UNS),   # S > 4 W
        # the frame's size is judged before the overlap and the descriptor, after the operands
        (dict(H=4096, W=4097, out=F), UNS), (dict(H=4096, W=4097, C=2), BAD), (dict(H=4096, W=4097, desc_words=23), BAD),
        (dict(H=32, W=7, desc_host=host([0, 0, 8, 32, 0, 0, 32, 4] + [0] * 16, np.int32)), BAD)],
    "haff_robot_heatmap": [
        (dict(logits=None), BAD), (dict(jet_rgb=None), BAD), (dict(workspace=None), BAD), (dict(out=None), BAD), (dict(n=0), BAD),
        (dict(n=65536), BAD), (dict(H=0), BAD), (dict(W=0), BAD), (dict(workspace_floats=1023), BAD), (dict(logits=F + 2), BAD),
        (dict(H=1048561), UNS), (dict(H=1048561, workspace_floats=1023), BAD), (dict(H=1048561, logits=F + 2), BAD), (dict(H=1048561, n=0), BAD)],
    "haff_robot_mask": [
        (dict(logits=None), BAD), (dict(out=None), BAD), (dict(H0=0), BAD), (dict(W0=0), BAD), (dict(on_value=-1), BAD), (dict(on_value=256), BAD),
        (dict(top=-40, mask=None), BAD), (dict(left=-30, mask=None), BAD), (dict(mask_h=37), BAD), (dict(mask_w=29), BAD), (dict(out=F + 2), BAD),
        (dict(mask=F + 2), BAD)],
    "haff_mask_quantile7": [
        (dict(logits=None), BAD), (dict(out=None), BAD), (dict(out=F), BAD), (dict(n=0), BAD), (dict(H=0), BAD), (dict(W=0), BAD), (dict(need=0), BAD),
        (dict(need=65537), BAD), (dict(logits=F + 2), BAD), (dict(out=F + 2), BAD), (dict(H=4097), UNS), (dict(W=4097), UNS),
        (dict(H=4097, out=F), BAD), (dict(W=4097, logits=F + 2), BAD), (dict(H=4097, need=0), BAD)],
}

# the plane sets of tools/data_dispatch_dump.cpp, (H, W): bytes for max_vertices = 1 and 65536 / for max_contours = 1, 4, 5 and 1024
SETS = {
    ((1, 1),): ((80, 262224), (128, 128, 160, 8288)),
    ((1, 64),): ((320, 262464), (368, 368, 400, 8528)),
    ((32, 32),): ((4272, 266416), (4432, 4432, 4464, 12592)),
    ((33, 65), (7, 3)): ((9056, 533344), (9376, 9408, 9440, 25728)),
    ((1024, 1024),): ((4325424, 4587568), (4456528, 4456528, 4456560, 4464688)),
    ((1025, 1024),): ((4329648, 4591792), (4460880, 4460880, 4460912, 4469040)),
    ((4096, 4096),): ((69206064, 69468208), (71303248, 71303248, 71303280, 71311408)),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    return haff.load_library()


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusals_and_their_codes(lib, name):
    order, base = ENTRY[name]
    assert all(want in (BAD, UNS) for _, want in CASES[name])      # nothing here may get as far as a launch
    wrong = []
    for over, want in CASES[name]:
        assert set(over) <= set(base), (name, over)
        args = dict(base, **over)
        got = int(getattr(lib, name)(*[args[k] for k in order]))
        if got != want:
            wrong.append((over, got, want))
    assert not wrong, wrong


def test_both_codes_and_a_doubly_wrong_input_are_recorded_where_the_entry_point_has_them():
    """haff_fill_contours_u8 and haff_robot_mask have no -2 rule; every other entry point has a -2 case."""
    for name, cases in CASES.items():
        codes = {want for _, want in cases}
        assert codes == ({BAD} if name in ("haff_fill_contours_u8", "haff_robot_mask") else {BAD, UNS}), name


@pytest.mark.parametrize("shapes", sorted(SETS))
def test_workspace_sizes(lib, shapes):
    table, n = planes(*shapes), len(shapes)
    need = ctypes.c_long(-1)
    hausdorff, extract = SETS[shapes]
    for mv, want in zip((1, 65536), hausdorff):
        assert lib.haff_contour_hausdorff_workspace(table, n, mv, ctypes.addressof(need)) == 0
        assert need.value == want, (shapes, mv, need.value)
        for mc, want_ext in zip((1, 4, 5, 1024), extract):        # the extract stages lie where the Hausdorff vertices would
            assert lib.haff_contour_extract_workspace(table, n, mc, mv, ctypes.addressof(need)) == 0
            assert need.value == want_ext, (shapes, mc, mv, need.value)
