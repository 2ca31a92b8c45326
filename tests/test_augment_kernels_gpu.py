"""csrc/frame_augment.hip on the GPU: haff_jitter_stats_u8, haff_augment_u8 and haff_flip_planes_u8 against Pillow at run time, bit
for bit, at the smallest shapes that can go wrong (rows of 3 W bytes that are and are not multiples of 4 and 16, one lane's 16-pixel
piece exactly, one pixel more, more than one block), and their refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/augment_ref.py
import augment_ref as A   # noqa: E402

pytestmark = pytest.mark.gpu

F1 = (A.fp32(0.47), A.fp32(1.52), A.fp32(0.81))
F2 = (A.fp32(1.33), A.fp32(0.66), A.fp32(1.6))
F3 = (A.fp32(0.9), A.fp32(1.21), A.fp32(0.4))


def _aug(flip, factors):
    return {"flip": bool(flip), "jitter": factors}


def _pil_sum(frame, fb):
    """S as Pillow computes it: the sum of the L plane of the brightness-enhanced frame."""
    from PIL import Image, ImageEnhance
    return int(np.asarray(ImageEnhance.Brightness(Image.fromarray(frame, "RGB")).enhance(fb).convert("L"), dtype=np.int64).sum())


def _check(dev, frames, augs):
    """frames uint8 [B,H,W,3] through ops.augment_frames against Pillow per frame; the input stays as it was."""
    from haff import ops
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    got = ops.augment_frames(x, augs).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == frames.shape and np.array_equal(x.cpu().numpy(), frames)
    for b, a in enumerate(augs):
        want = A.pil_augment(frames[b], a["flip"], a["jitter"]) if a else frames[b]
        bad = int((got[b] != want).sum())
        assert bad == 0, f"frame {b} of {frames.shape} with {a}: {bad} bytes differ, first at {np.argwhere(got[b] != want)[0].tolist()}"
    return got


@pytest.mark.parametrize("W", [1, 2, 3, 5, 21, 64, 65, 67])
def test_every_flag_combination_at_the_edge_widths(dev, W):
    for H in (1, 2, 33):
        frames = np.stack([A.random_frame((H, W), 10 * W + H + k, ("plain", "dark", "bright", "plain")[k]) for k in range(4)])
        _check(dev, frames, [None, _aug(True, None), _aug(False, F1), _aug(True, F2)])


def test_one_300_by_400_frame(dev):
    frame = A.random_frame((300, 400), 3)
    got = _check(dev, frame[None], [_aug(True, F3)])
    assert not np.array_equal(got[0], frame)
    _check(dev, frame[None], [_aug(False, F1)])


def test_batch_of_three_with_per_frame_flags_and_factors(dev):
    """[flip, none, flip | jitter] with three different factor triples: a per-frame indexing slip shows, the unflagged frame comes
    back equal to its input, and the factors of frames without the jitter bit are not applied."""
    from haff import ops
    frames = np.stack([A.random_frame((37, 53), 40 + k) for k in range(3)])
    x = torch.from_numpy(frames).to(dev)
    flags = torch.tensor([ops.AUG_FLIP, 0, ops.AUG_FLIP | ops.AUG_JITTER], dtype=torch.int32, device=dev)
    factors = torch.tensor([F1, F2, F3], dtype=torch.float32, device=dev)
    sums = ops.jitter_stats(x, flags, factors)
    assert sums.cpu().tolist() == [0, 0, _pil_sum(frames[2], F3[0])]
    got = ops.augment_u8(x, flags, factors, sums).cpu().numpy()
    assert np.array_equal(got[0], A.pil_flip(frames[0])) and np.array_equal(got[1], frames[1])
    assert np.array_equal(got[2], A.pil_augment(frames[2], True, F3))
    _check(dev, frames, [_aug(True, None), None, _aug(True, F3)])


@pytest.mark.parametrize("f,d,i,separate,fused", A.FMA_TRIPLES)
def test_the_blend_rounds_product_and_sum_separately(dev, f, d, i, separate, fused):
    """The triple staged as a real frame: its contrast-stage mean is d and pixel (0, 0) holds i, so a fused multiply-add in the
    kernel gives `fused` there and Pillow gives `separate`."""
    frame = A.staged_frame(d, i)
    for flip in (False, True):
        got = _check(dev, frame[None], [_aug(flip, (1.0, f, 1.0))])
        assert got[0, 0, -1 if flip else 0, 0] == separate != fused


def test_tie_zero_full_and_identity_frames(dev):
    from haff import ops
    tie = A.tie_frame()
    got = _check(dev, tie[None], [_aug(False, (1.0, A.fp32(0.4), 1.0))])
    assert got[0, 0, :, 0].tolist() == [10, 11]                         # m = 11: the tie rounds up
    x = torch.from_numpy(tie[None]).to(dev)
    flags, factors = ops.augment_table([_aug(False, (1.0, 1.0, 1.0))], dev)
    assert ops.jitter_stats(x, flags, factors).cpu().tolist() == [21]
    zero, full = np.zeros((9, 19, 3), np.uint8), np.full((9, 19, 3), 255, np.uint8)
    top = (A.fp32(1.6),) * 3
    got = _check(dev, np.stack([zero, full]), [_aug(True, top), _aug(True, top)])
    assert not got[0].any()
    assert (A.blend(0, full, top[0]) == 255).all()                      # every channel clips in the brightness stage
    frame = A.random_frame((33, 21), 8)
    got = _check(dev, frame[None], [_aug(False, (1.0, 1.0, 1.0))])
    assert np.array_equal(got[0], frame)                                # factor 1.0 returns the input's bytes


def test_stats_zero_a_dirty_buffer_and_repeat_bitwise(dev):
    from haff import ops
    frames = np.stack([A.random_frame((64, 67), 70 + k, ("plain", "dark", "bright")[k]) for k in range(3)])
    x = torch.from_numpy(frames).to(dev)
    flags, factors = ops.augment_table([_aug(False, F1), _aug(True, None), _aug(True, F2)], dev)
    want = [_pil_sum(frames[0], F1[0]), 0, _pil_sum(frames[2], F2[0])]
    assert want == [A.jitter_sum(frames[0], F1[0]), 0, A.jitter_sum(frames[2], F2[0])]
    sums = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    for _ in range(3):                                                  # the second and third runs start from the first one's sums
        assert ops.jitter_stats(x, flags, factors, out=sums).cpu().tolist() == want
    big = A.random_frame((300, 400), 9)                                  # more than one block adds into the slot
    xb = torch.from_numpy(big[None]).to(dev)
    flags, factors = ops.augment_table([_aug(False, F3)], dev)
    assert ops.jitter_stats(xb, flags, factors).cpu().tolist() == [_pil_sum(big, F3[0])]


def test_refusals_return_their_codes_and_touch_nothing(dev):
    from haff import lib as hlib, ops
    lib = hlib.load_library()
    x = torch.from_numpy(A.random_frame((8, 8), 1)[None]).to(dev)
    keep = x.clone()
    out = torch.full_like(x, 0x5A)
    flags, factors = ops.augment_table([_aug(True, F1)], dev)
    sums = torch.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    args = (flags.data_ptr(), factors.data_ptr(), sums.data_ptr(), stream)
    assert lib.haff_augment_u8(x.data_ptr(), x.data_ptr(), 1, 8, 8, *args) == -1                       # out == in
    assert lib.haff_augment_u8(x.data_ptr(), out.data_ptr(), 1, 4097, 4096, *args) == -2               # H W > 2^24: host check only
    assert lib.haff_jitter_stats_u8(x.data_ptr(), 1, 4097, 4096, *args) == -2
    assert lib.haff_augment_u8(x.data_ptr(), out.data_ptr(), 0, 8, 8, *args) == -1
    assert lib.haff_augment_u8(x.data_ptr(), out.data_ptr(), 1, 8, 8, flags.data_ptr(), factors.data_ptr(), None, stream) == -1
    with pytest.raises(hlib.HaffLibraryError, match="code -1"):
        ops.augment_u8(x, flags, factors, sums, out=x)
    planes = torch.full((2, 8, 8), 3, dtype=torch.uint8, device=dev)
    pout = torch.full_like(planes, 0x5A)
    pflags = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    assert lib.haff_flip_planes_u8(planes.data_ptr(), planes.data_ptr(), 2, 8, 8, pflags.data_ptr(), stream) == -1
    assert lib.haff_flip_planes_u8(planes.data_ptr(), pout.data_ptr(), 2, 0, 8, pflags.data_ptr(), stream) == -1
    assert lib.haff_flip_planes_u8(planes.data_ptr(), pout.data_ptr(), 2, 8, 8, ctypes.c_void_p(pflags.data_ptr() + 2), stream) == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((pout == 0x5A).all()) and torch.equal(x, keep) and bool((planes == 3).all())
    assert sums.cpu().tolist() == [0x5A5A5A5A5A5A5A5A]
    assert ops.augment_frames_supported((4096, 4096)) and not ops.augment_frames_supported((4097, 4096))


def test_flip_planes_mirrors_only_the_flagged_planes(dev):
    from haff import ops
    planes = np.random.default_rng(2).integers(0, 256, (5, 33, 47), dtype=np.uint8)
    x = torch.from_numpy(planes).to(dev)
    flags = torch.tensor([1, 0, 1, 0, 1], dtype=torch.int32, device=dev)
    got = ops.flip_planes(x, flags).cpu().numpy()
    for p in range(5):
        want = A.pil_flip(planes[p]) if p % 2 == 0 else planes[p]
        assert np.array_equal(got[p], want), p
    assert np.array_equal(x.cpu().numpy(), planes)
    for W in (1, 15, 16, 17, 32):                                       # below, at and past one lane's 16 bytes
        small = np.random.default_rng(W).integers(0, 256, (2, 3, W), dtype=np.uint8)
        got = ops.flip_planes(torch.from_numpy(small).to(dev), torch.tensor([1, 0], dtype=torch.int32, device=dev)).cpu().numpy()
        assert np.array_equal(got[0], small[0][:, ::-1]) and np.array_equal(got[1], small[1]), W
