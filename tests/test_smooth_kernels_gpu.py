"""haff_mask_quantile7 (csrc/mask_smooth.hip, ops.mask_quantile7) against the CPU restatement tests/smooth_ref.py: value-equal at
every pixel (torch.equal after adding +0.0: -0.0 and +0.0 may be exchanged), -inf where the restatement has it, never a NaN; the
output's surroundings keep their bits; the refusals write nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/smooth_ref.py
import smooth_ref as S   # noqa: E402

pytestmark = pytest.mark.gpu

# (1,1) .. (3,5): reflection with overshoot; (16,64): exactly one 64 x 16 tile; (17,65): one pixel into a second tile on both axes;
# (37,131): odd pitch, the element path; (40,132): the float4 path with a ragged last tile
SHAPES = [(1, 1), (1, 9), (2, 3), (3, 5), (7, 7), (16, 64), (17, 65), (37, 131), (40, 132)]
TAUS = (0.5, 0.25, 0.9)
GUARD_BITS = 0x7FC00ABC          # a NaN with a payload of its own
_CASES = {}


def _planes(shape):
    """[(name, float32 plane)] of one shape: the fields, the stripes at the tile seams, the index planes. Computed once."""
    if shape not in _CASES:
        rng = np.random.default_rng(shape[0] * 1000 + shape[1])
        planes = list(S.fields(shape, rng)) + [(n, p) for n, p, _ in S.stripes(shape)] + list(S.index_planes(shape, rng))
        _CASES[shape] = (planes, {})
    return _CASES[shape]


def _expected(shape, need):
    planes, cache = _planes(shape)
    if need not in cache:
        cache[need] = np.stack([S.quantile7(p, need) for _, p in planes])
    return planes, cache[need]


def _compare(torch, got, want, label):
    got = got.cpu()
    want = torch.from_numpy(want)
    assert not torch.isnan(got).any(), label
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)), label
    if not torch.equal(got + 0.0, want + 0.0):
        bad = ((got + 0.0) != (want + 0.0)).nonzero()
        raise AssertionError((label, int(bad.shape[0]), bad[:4].tolist()))


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_quantile_equals_the_restatement(dev, shape, tau):
    import torch
    from haff import ops, postprocess
    need = postprocess.smooth_need(tau)
    assert need == S.need(tau)
    planes, want = _expected(shape, need)
    x = torch.from_numpy(np.stack([p for _, p in planes])).to(dev)
    keep = x.clone()
    got = ops.mask_quantile7(x, need)
    assert got.shape == x.shape and got.dtype == torch.float32
    for k, (name, _) in enumerate(planes):
        _compare(torch, got[k], want[k], (shape, tau, name))
    assert torch.equal(x.view(torch.int32), keep.view(torch.int32))            # the input is only read
    again = ops.mask_quantile7(x, need)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))         # a second run is bitwise equal
    # the identity on the device's own output, at the logit thresholds the CLI compares with
    for lt in (postprocess.sigmoid_logit_threshold(0.5), -1.0):
        on = (got > lt).cpu().numpy().astype(np.uint8) * 255
        for k, (name, p) in enumerate(planes):
            assert np.array_equal(on[k], S.files_route(p, lt, tau)), (shape, tau, name, lt)


@pytest.mark.parametrize("tau", TAUS)
def test_three_planes_of_33x68(dev, tau):
    """the plane stride, with W % 4 == 0 and H * W % 16 != 0: planes 1 and 2 start 16-B aligned only because H * W % 4 == 0"""
    import torch
    from haff import ops
    need = S.need(tau)
    planes, want = _expected((33, 68), need)
    x = torch.from_numpy(np.stack([p for _, p in planes[:3]])).to(dev)
    got = ops.mask_quantile7(x, need)
    for k in range(3):
        _compare(torch, got[k], want[k], (tau, planes[k][0]))
        _compare(torch, ops.mask_quantile7(x[k:k + 1], need)[0], want[k], (tau, planes[k][0], "alone"))


def test_raw_need_and_its_ends(dev):
    """need is taken as given: 1 is the maximum of the 49 taps that are not NaN, 65536 the minimum (-inf with a NaN among them);
    one hot pixel weighs 72 * 72 = 5184 at its own position and goes at need = 5185."""
    import torch
    from haff import ops
    planes, _ = _planes((17, 65))
    x = torch.from_numpy(np.stack([p for _, p in planes])).to(dev)
    for need in (1, 64, 5184, 5185, 65535, 65536):
        got = ops.mask_quantile7(x, need)
        for k, (name, p) in enumerate(planes):
            _compare(torch, got[k], S.quantile7(p, need), (need, name))
    hot = np.full((1, 9, 9), -4.0, np.float32)
    hot[0, 4, 4] = 3.0
    h = torch.from_numpy(hot).to(dev)
    assert ops.mask_quantile7(h, 5184)[0, 4, 4].item() == 3.0 and (ops.mask_quantile7(h, 5185) == -4.0).all()


@pytest.mark.parametrize("shape,n,lead", [((1, 1), 1, 1), ((17, 65), 2, 70), ((40, 132), 2, 133), ((40, 132), 1, 136), ((16, 64), 3, 67)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_surroundings_keep_their_bits(dev, shape, n, lead):
    """Input and output are views `lead` floats into larger allocations (more than a row above, the same below; an odd lead leaves
    the base 4-B aligned only, so W % 4 == 0 must take the element path). The output's allocation is filled with a payload NaN:
    every word outside the n planes keeps its bits and no word inside keeps them."""
    import torch
    import haff
    H, W = shape
    planes, want = _expected(shape, 32768)
    total = n * H * W
    src = torch.full((total + 2 * lead,), GUARD_BITS, dtype=torch.int32, device=dev)
    dst = torch.full((total + 2 * lead,), GUARD_BITS, dtype=torch.int32, device=dev)
    src[lead:lead + total] = torch.from_numpy(np.stack([p for _, p in planes[:n]])).reshape(-1).view(torch.int32).to(dev)
    lib = haff.load_library()
    rc = lib.haff_mask_quantile7(src.data_ptr() + 4 * lead, n, H, W, 32768, dst.data_ptr() + 4 * lead,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    out = dst.cpu()
    assert (out[:lead] == GUARD_BITS).all() and (out[lead + total:] == GUARD_BITS).all()
    body = out[lead:lead + total]
    assert (body != GUARD_BITS).all()
    got = body.view(torch.float32).reshape(n, H, W)
    for k in range(n):
        _compare(torch, got[k], want[k], (shape, lead, planes[k][0]))


def test_refusals_write_nothing(dev):
    import torch
    import haff
    lib = haff.load_library()
    x = torch.randn((2, 8, 12), device=dev)
    out = torch.full((2, 8, 12), GUARD_BITS, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    p, q = x.data_ptr(), out.data_ptr()
    cases = [((None, 2, 8, 12, 32768, q), -1), ((p, 2, 8, 12, 32768, None), -1), ((p + 2, 1, 8, 12, 32768, q), -1),
             ((p, 1, 8, 12, 32768, q + 2), -1), ((q, 2, 8, 12, 32768, q), -1), ((p, 0, 8, 12, 32768, q), -1),
             ((p, 2, 0, 12, 32768, q), -1), ((p, 2, 8, 0, 32768, q), -1), ((p, 2, 8, 12, 0, q), -1), ((p, 2, 8, 12, 65537, q), -1),
             ((p, 1, 4097, 1, 32768, q), -2), ((p, 1, 1, 4097, 32768, q), -2)]
    for args, rc in cases:
        assert lib.haff_mask_quantile7(*args, s) == rc, args
    torch.cuda.synchronize()
    assert (out == GUARD_BITS).all()
    with pytest.raises(haff.HaffLibraryError):
        haff.ops.mask_quantile7(x, 0)
    with pytest.raises(RuntimeError):
        haff.ops.mask_quantile7(x.cpu(), 32768)
    with pytest.raises(AssertionError):
        haff.ops.mask_quantile7(x.double(), 32768)


def test_more_planes_than_one_grid_axis_holds(dev):
    """65537 planes of 1 x 2: past the 65535 workgroups of the grid's z axis, where a workgroup walks several planes"""
    import torch
    from haff import ops
    pats = np.array([[[1.0, -2.0]], [[np.nan, 5.0]], [[-0.0, 7.0]], [[np.inf, -np.inf]], [[3.0, 3.0]]], np.float32)
    n = 65537
    idx = np.arange(n) % len(pats)
    x = torch.from_numpy(pats[idx]).to(dev)
    want = np.stack([S.quantile7(p, 32768) for p in pats])
    got = ops.mask_quantile7(x, 32768)
    _compare(torch, got, want[idx], "65537 planes")
