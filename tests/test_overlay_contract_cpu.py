"""haff_score_masks' host contract for overlay records (haff_score_vis behind the frame table): every refusal with its code, their
order, and that frames with vis = 0 keep the codes and the order they had. Nothing is launched: the host tables are real, the device
addresses fake and never dereferenced, and no call below would pass validation. CPU only."""
import ctypes

import numpy as np
import pytest

import haff

import score_ref as R

BAD, UNS = -1, -2
F = 0x10000          # a fake, 16-byte aligned device address


def vis_record(**over):
    """haff_score_vis as 16 int64 words (include/haff_hip.h): rgb row col out[2] stride[2] | Hf Wf t | alpha[2] beta[2] gamma | color."""
    v = dict(rgb=F + 0x100001, row=F + 0x200000, col=F + 0x300000, out=(F + 0x400000, F + 0x400000 + 3 * 34), stride=(6 * 34, 6 * 34),
             Hf=7, Wf=34, t=0)
    v.update(over)
    t = np.zeros((1, 16), np.int64)
    t[0, :7] = [v["rgb"], v["row"], v["col"], *v["out"], *v["stride"]]
    t.view(np.int32).reshape(1, 32)[0, 14:17] = [v["Hf"], v["Wf"], v["t"]]
    t.view(np.float32).reshape(1, 32)[0, 17:22] = [0.5, 1.0, 0.5, 0.5, 0.0]
    t.view(np.int32).reshape(1, 32)[0, 22:28] = [255, 0, 0, 0, 255, 0]
    return t


def frame(vis=0, **over):
    t = R.descriptor_table(**over)        # (Hs, Ws) = (5, 7), (Hb, Wb) = (13, 11)
    t.view(np.int32).reshape(1, 32)[0, 29] = vis
    return t


def call(lib, frames, records, n_th=2):
    table = np.ascontiguousarray(np.concatenate(list(frames) + list(records)))
    th = (ctypes.c_float * 8)(*([0.0] * 8))
    return int(lib.haff_score_masks(table.ctypes.data, 0x20000, len(frames), ctypes.cast(th, ctypes.c_void_p), n_th, 0x30000, None))


@pytest.fixture(scope="module")
def lib():
    return haff.load_library()


IDENTITY = dict(row=0, col=0, Hf=13, Wf=11, out=(F + 0x400000, 0), stride=(33, 0))

REFUSALS = [
    ("vis above n_frames", dict(vis=2), {}, BAD),
    ("vis negative", dict(vis=-1), {}, BAD),
    ("null rgb", dict(vis=1), dict(rgb=0), BAD),
    ("both out null", dict(vis=1), dict(out=(0, 0)), BAD),
    ("row without col", dict(vis=1), dict(col=0), BAD),
    ("col without row", dict(vis=1), dict(row=0), BAD),
    ("no tables, other rows", dict(vis=1), dict(IDENTITY, Hf=12), BAD),
    ("no tables, other columns", dict(vis=1), dict(IDENTITY, Wf=12, stride=(36, 0)), BAD),
    ("misaligned row", dict(vis=1), dict(row=F + 0x200002), BAD),
    ("misaligned col", dict(vis=1), dict(col=F + 0x300001), BAD),
    ("t negative", dict(vis=1), dict(t=-1), BAD),
    ("t == n_th", dict(vis=1), dict(t=2), BAD),
    ("stride 0 short", dict(vis=1), dict(stride=(3 * 34 - 1, 6 * 34)), BAD),
    ("stride 1 short", dict(vis=1), dict(stride=(6 * 34, 3 * 34 - 1)), BAD),
    ("stride negative", dict(vis=1), dict(stride=(-6 * 34, 6 * 34)), BAD),
    ("Hf 0", dict(vis=1), dict(Hf=0), BAD),
    ("Wf 0", dict(vis=1), dict(Wf=0), BAD),
    ("Wf negative", dict(vis=1), dict(Wf=-34), BAD),
    ("Hf 4097", dict(vis=1), dict(Hf=4097), UNS),
    ("Wf 4097", dict(vis=1), dict(Wf=4097, stride=(6 * 4097, 6 * 4097)), UNS),
    # a record's sides are judged before its pointers, as a frame's are
    ("Hf 4097 and null rgb", dict(vis=1), dict(Hf=4097, rgb=0), UNS),
    ("Hf 0 and Wf 4097", dict(vis=1), dict(Hf=0, Wf=4097), BAD),
    # the frame's own checks come first
    ("frame side 4097 and null rgb", dict(vis=1, hb=4097, gt=(0, 0), obj=(0, 0)), dict(rgb=0), UNS),
    ("frame n_tax and Hf 4097", dict(vis=1, n_tax=0), dict(Hf=4097), BAD),
    ("frame gt shape and Wf 4097", dict(vis=1, gt_hw=((12, 11), (0, 0))), dict(Wf=4097), BAD),
]


@pytest.mark.parametrize("name,frame_over,vis_over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(lib, name, frame_over, vis_over, code):
    assert call(lib, [frame(**frame_over)], [vis_record(**vis_over)]) == code


def test_the_threshold_bound_is_the_calls(lib):
    assert call(lib, [frame(vis=1)], [vis_record(t=1)], n_th=1) == BAD                  # in range for two thresholds, not for one
    assert call(lib, [frame(vis=1)], [vis_record(t=1, Hf=4097)], n_th=1) == UNS         # a record's sides come before its t
    assert call(lib, [frame(vis=1)], [vis_record(t=8)], n_th=8) == BAD


def test_a_canvas_that_is_not_drawn_needs_no_stride(lib):
    """out[0] NULL with stride[0] = 0 is no stride refusal: the record fails only on what the case breaks besides."""
    assert call(lib, [frame(vis=1)], [vis_record(out=(0, F + 0x400000), stride=(0, 102), t=5)]) == BAD       # t alone
    assert call(lib, [frame(vis=1)], [vis_record(out=(0, F + 0x400000), stride=(0, 101))]) == BAD            # the drawn one is short
    assert call(lib, [frame(vis=1)], [vis_record(out=(0, F + 0x400000), stride=(0, 102), Hf=4097)]) == UNS


def test_frames_are_judged_in_order_and_records_with_their_frame(lib):
    ok, rec = frame(), vis_record()
    # frame 0 draws through record 1 (vis = 2), frame 1 through record 0
    assert call(lib, [frame(vis=2), frame(vis=1)], [vis_record(Hf=4097), vis_record(rgb=0)]) == BAD          # frame 0's record is [1]
    assert call(lib, [frame(vis=2), frame(vis=1)], [vis_record(rgb=0), vis_record(Hf=4097)]) == UNS
    assert call(lib, [frame(vis=1), frame(hs=0)], [vis_record(Hf=4097)]) == UNS                              # record of frame 0 first
    assert call(lib, [frame(hb=4097, gt=(0, 0), obj=(0, 0)), frame(vis=1)], [vis_record(rgb=0)]) == UNS
    assert call(lib, [frame(vis=3), ok], [rec, rec, rec]) == BAD                                             # 1..n_frames
    assert call(lib, [frame(vis=1), frame(vis=1)], [vis_record(Hf=4097)]) == UNS                             # frame 0's record, then
    assert call(lib, [frame(vis=1, hs=0), frame(vis=1)], [rec]) == BAD
    # a record draws for one frame: the second frame that names it is refused, after that frame's own checks
    assert call(lib, [ok, frame(vis=2), frame(vis=2)], [rec, rec]) == BAD
    assert call(lib, [ok, frame(vis=2), frame(vis=2, hb=4097, gt=(0, 0), obj=(0, 0))], [rec, rec]) == UNS
    assert call(lib, [ok, frame(vis=2, ws=4097), frame(vis=2)], [rec, rec]) == UNS


def test_the_calls_own_checks_still_come_first(lib):
    th = (ctypes.c_float * 8)(*([0.0] * 8))
    table = np.ascontiguousarray(np.concatenate([frame(vis=1), vis_record(Hf=4097)]))
    args = dict(host=table.ctypes.data, dev=0x20000, n=1, n_th=2, counts=0x30000)

    def go(**over):
        a = dict(args, **over)
        return int(lib.haff_score_masks(a["host"], a["dev"], a["n"], ctypes.cast(th, ctypes.c_void_p), a["n_th"], a["counts"], None))
    assert go() == UNS
    assert go(n_th=9) == BAD and go(n_th=0) == BAD and go(counts=0x30002) == BAD and go(dev=0) == BAD and go(dev=0x20004) == BAD


def test_frames_without_a_record_keep_their_codes_and_order(lib):
    """vis = 0: the refusals tests/score_ref.py lists, and the order tests/test_data_contract_cpu.py pins, with a record behind the
    table that would be refused if anything looked at it."""
    got, big = R.score_refusals(lib)
    assert all(v == BAD for v in got.values()), {k: v for k, v in got.items() if v != BAD}
    assert all(v == UNS for v in big.values()), big
    junk = vis_record(rgb=0, Hf=-5, t=99)
    assert call(lib, [frame(hb=4097, gt=(0, 0), obj=(0, 0), left=0x10002)], [junk]) == UNS      # sides before pointers
    assert call(lib, [frame(hb=4097, ws=0, gt=(0, 0), obj=(0, 0))], [junk]) == BAD
    assert call(lib, [frame(hb=4097, gt=(0, 0), obj=(0, 0)), frame(hs=0)], [junk]) == UNS       # the frames in order
    assert call(lib, [frame(hs=0), frame(hb=4097, gt=(0, 0), obj=(0, 0))], [junk]) == BAD
    assert call(lib, [frame(n_tax=1025)], [junk]) == BAD and call(lib, [frame(tax=0x18003)], [junk]) == BAD
    assert call(lib, [frame(obj_hw=((0, 0), (11, 13)))], [junk]) == BAD
