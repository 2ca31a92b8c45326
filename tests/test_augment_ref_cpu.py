"""tests/augment_ref.py (the numpy restatement the GPU tests lean on for staging their cases, and the arithmetic
csrc/frame_augment.hip implements) against Pillow itself, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/augment_ref.py
import augment_ref as A   # noqa: E402


@pytest.mark.parametrize("f,d,i,separate,fused", A.FMA_TRIPLES)
def test_blend_rounds_product_and_sum_separately_as_pillow_does(f, d, i, separate, fused):
    assert A.pil_blend_1x1(d, i, f) == separate
    assert int(A.blend(d, i, f)) == separate
    assert A.blend_fused(d, i, f) == fused != separate          # the triples do tell the two forms apart


@pytest.mark.parametrize("f,d,i,separate,fused", A.FMA_TRIPLES)
def test_staged_frames_carry_the_triples_through_the_contrast_stage(f, d, i, separate, fused):
    frame = A.staged_frame(d, i)
    got = A.pil_jitter(frame, (1.0, f, 1.0))
    assert got[0, 0, 0] == separate
    assert np.array_equal(A.jitter(frame, (1.0, f, 1.0)), got)


@pytest.mark.parametrize("factor", [0.4, 1.0, 1.6])
def test_single_factors_on_every_stage(factor):
    """<= 1 and > 1 are Pillow's two branches (the second clips); 1.0 returns the input's bytes."""
    f = A.fp32(factor)
    for seed, kind in enumerate(("plain", "dark", "bright")):
        frame = A.random_frame((17, 23), seed, kind)
        for stage in range(3):
            factors = tuple(f if k == stage else 1.0 for k in range(3))
            want = A.pil_jitter(frame, factors)
            assert np.array_equal(A.jitter(frame, factors), want), (kind, stage)
            if factor == 1.0:
                assert np.array_equal(want, frame)
        assert np.array_equal(A.jitter(frame, (f, f, f)), A.pil_jitter(frame, (f, f, f))), kind


def test_all_zero_and_all_255_frames():
    zero, full = np.zeros((5, 7, 3), np.uint8), np.full((5, 7, 3), 255, np.uint8)
    for factors in ((1.6, 1.6, 1.6), (0.4, 1.6, 0.4), (1.0, 1.0, 1.0)):
        factors = tuple(A.fp32(f) for f in factors)
        for frame in (zero, full):
            assert np.array_equal(A.jitter(frame, factors), A.pil_jitter(frame, factors))
    assert (A.blend(0, full, A.fp32(1.6)) == 255).all()          # every channel clips
    assert not A.jitter(zero, (A.fp32(1.6),) * 3).any()


def test_mean_tie_rounds_up():
    frame = A.tie_frame()
    assert A.jitter_sum(frame, 1.0) == 21 and A.jitter_mean(frame, 1.0) == 11
    f = A.fp32(0.4)                                               # contrast 0.4 towards 11 tells 10 from 11: 10.4 | 11.0 vs 10.0 | 10.6
    want = A.pil_jitter(frame, (1.0, f, 1.0))
    assert want[0, :, 0].tolist() == [10, 11]
    assert np.array_equal(A.jitter(frame, (1.0, f, 1.0)), want)


def _random_cases():
    rng = np.random.default_rng(5)
    cases = []
    for n in range(40):
        hw = (int(rng.integers(1, 70)), int(rng.integers(1, 70)))
        factors = tuple(A.fp32(v) for v in rng.uniform(0.4, 1.6, 3))
        cases.append((A.random_frame(hw, 100 + n, ("plain", "dark", "bright")[n % 3]), factors))
    return cases


def test_random_frames_equal_pillow_bit_for_bit():
    total = 0
    for frame, factors in _random_cases():
        want = A.pil_jitter(frame, factors)
        got = A.jitter(frame, factors)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (frame.shape, factors, int((got != want).sum()))
        total += frame.size
    assert total > 100000


def test_jitter_and_flip_commute_through_pillow():
    for frame, factors in _random_cases()[:12]:
        a = A.pil_jitter(np.ascontiguousarray(A.pil_flip(frame)), factors)
        b = A.pil_flip(np.ascontiguousarray(A.pil_jitter(frame, factors)))
        assert np.array_equal(a, b), frame.shape
        assert np.array_equal(A.augment(frame, True, factors), b)
        assert np.array_equal(A.pil_augment(frame, True, factors), b)
    x = A.random_frame((3, 5), 0)
    assert np.array_equal(A.pil_flip(x), x[:, ::-1]) and np.array_equal(A.augment(x, True, None), x[:, ::-1])
