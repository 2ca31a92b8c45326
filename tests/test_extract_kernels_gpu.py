"""haff_affordance_extract (csrc/affordance_extract.hip, ops.affordance_extract) against the brute-force restatement
tests/extract_ref.py: equal at every pixel and in every statistics word, for every listed shape, k and hand geometry; a mixed
batch in one call; the inputs only read; guard bytes around every output intact; a second run bitwise equal; a null `out` gives
the same statistics; every refusal raises and writes nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/extract_ref.py
import extract_ref as E   # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5
PAD = 67                          # an odd count of guard bytes in front of every output: outputs start at any alignment
_CASES = {}


def _items(shape):
    """[(label, plane, hand)] of one shape and their AND planes, computed once: every plane without a hand and with one of its
    shape; the fields and stripes with every other hand geometry."""
    if shape not in _CASES:
        rng = np.random.default_rng(shape[0] * 1000 + shape[1])
        planes, hands = E.planes(shape, rng), E.hands(shape, rng)
        items = []
        for hname, hand in hands:
            for pname, plane in planes:
                if hname not in ("none", "same") and pname.startswith("lone"):
                    continue
                items.append((f"{pname}/{hname}", plane, hand))
        _CASES[shape] = (items, [E.and_plane(p, h) for _, p, h in items], {})
    return _CASES[shape]


def _expected(shape, k):
    items, ands, cache = _items(shape)
    if k not in cache:
        outs = [E.dilate_white(a, k) for a in ands]
        cache[k] = (outs, [E.stats_of(a, o, h is not None) for a, o, (_, _, h) in zip(ands, outs, items)])
    return items, cache[k][0], cache[k][1]


def _upload(torch, ops, dev, items, with_out=True):
    """device tensors of a list of (label, plane, hand): (call items, input clones, guarded output buffers)"""
    tables = {}
    call, keep, bufs = [], [], []
    for _, plane, hand in items:
        p = torch.from_numpy(plane).to(dev)
        h = t = None
        if hand is not None:
            h = torch.from_numpy(hand).to(dev)
            key = (hand.shape, plane.shape)
            if key not in tables:                             # items of one geometry share their tables
                tables[key] = ops.nearest_pad_tables(hand.shape, plane.shape, device=dev)
            t = tables[key]
        out = None
        if with_out:
            buf = torch.full((PAD + plane.size + PAD,), GUARD, dtype=torch.uint8, device=dev)
            out = buf[PAD:PAD + plane.size].view(plane.shape)
            bufs.append(buf)
        call.append((p, h, t, out))
        keep.append((p.clone(), None if h is None else h.clone()))
    return call, keep, bufs


def _check(torch, call, keep, bufs, stats, items, outs, want_stats, label):
    stats = stats.cpu().numpy()
    assert stats.dtype == np.int64 and stats.shape == (len(items), 8)
    for i, (name, plane, _) in enumerate(items):
        assert stats[i].tolist() == want_stats[i], (label, name, stats[i].tolist(), want_stats[i])
        if bufs:
            buf = bufs[i].cpu().numpy()
            got = buf[PAD:PAD + plane.size].reshape(plane.shape)
            if not np.array_equal(got, outs[i]):
                bad = np.argwhere(got != outs[i])
                raise AssertionError((label, name, len(bad), bad[:4].tolist()))
            assert (buf[:PAD] == GUARD).all() and (buf[PAD + plane.size:] == GUARD).all(), (label, name)
        p, h = keep[i]
        assert torch.equal(call[i][0], p) and (h is None or torch.equal(call[i][1], h)), (label, name)   # inputs only read


@pytest.mark.parametrize("k", E.KS)
@pytest.mark.parametrize("shape", E.SHAPES, ids=lambda s: "%dx%d" % s)
def test_extract_equals_the_restatement(dev, shape, k):
    import torch
    from haff import ops
    items, outs, want = _expected(shape, k)
    call, keep, bufs = _upload(torch, ops, dev, items)
    stats = ops.affordance_extract(call, k)
    _check(torch, call, keep, bufs, stats, items, outs, want, (shape, k))
    first = [b.clone() for b in bufs]
    again = ops.affordance_extract(call, k)
    assert torch.equal(stats, again) and all(torch.equal(a, b) for a, b in zip(first, bufs))      # a second run is bitwise equal
    null = ops.affordance_extract([(p, h, t, None) for p, h, t, _ in call], k)
    assert torch.equal(stats, null)                                                                # statistics only: the same words


def test_mixed_shapes_in_one_call(dev):
    """Items of every shape in one launch (a workgroup past a small item's tiles leaves), plus the 6 -> 34 geometry whose column 17
    reads source column 2, and 4-byte stores next to byte stores (outputs at odd addresses, odd pitches)."""
    import torch
    from haff import ops
    k = 4
    items, outs, want = [], [], []
    for shape in E.SHAPES:
        its, o, w = _expected(shape, k)
        pick = [i for i, (name, _, _) in enumerate(its) if name.split("/")[0] in ("sparse", "ones_twos", "full")]
        items += [its[i] for i in pick]
        outs += [o[i] for i in pick]
        want += [w[i] for i in pick]
    rng = np.random.default_rng(34)
    hand = np.zeros((6, 6), np.uint8)
    hand[:, 2] = 255                                          # source column 2 alone: destination column 17 is on, 18 is not
    plane = np.full((9, 34), 255, np.uint8)
    a = E.and_plane(plane, hand)
    assert a[:, 17].all() and not a[:, 18].any() and not E.and_plane(plane, hand, exact=True)[:, 17].any()
    for p, h in ((plane, hand), (rng.integers(0, 2, (9, 34)).astype(np.uint8) * 255, (rng.random((6, 6)) < 0.5).astype(np.uint8) * 255)):
        aa, o, s = E.extract(p, h, k)
        items.append(("six_to_34", p, h))
        outs.append(o)
        want.append(s)
    order = rng.permutation(len(items)).tolist()
    items, outs, want = [items[i] for i in order], [outs[i] for i in order], [want[i] for i in order]
    call, keep, bufs = _upload(torch, ops, dev, items)
    stats = ops.affordance_extract(call, k)
    _check(torch, call, keep, bufs, stats, items, outs, want, "mixed")


def test_refusals_raise_and_write_nothing(dev):
    import torch
    from haff import ops
    H, W = 5, 9
    plane = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    hand = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    col, row = ops.nearest_pad_tables((H, W), (H, W), device=dev)
    out = torch.full((H, W), GUARD, dtype=torch.uint8, device=dev)
    stats = torch.full((1, 8), -7, dtype=torch.int64, device=dev)
    wide = torch.zeros((H, 2 * W), dtype=torch.uint8, device=dev)
    bad = [
        (TypeError, "uint8", [(plane.to(torch.int16), None, None, out)], 3),
        (TypeError, "uint8", [(plane, hand.to(torch.float32), (col, row), out)], 3),
        (TypeError, "uint8", [(plane, None, None, out.to(torch.int32))], 3),
        (TypeError, "int32", [(plane, hand, (col.to(torch.int64), row), out)], 3),
        (ValueError, "not contiguous", [(wide[:, ::2], None, None, out)], 3),
        (ValueError, "not contiguous", [(plane, wide[:, ::2], (col, row), out)], 3),
        (ValueError, "not contiguous", [(plane, None, None, wide[:, ::2])], 3),
        (RuntimeError, "HBM", [(plane.cpu(), None, None, out)], 3),
        (RuntimeError, "HBM", [(plane, hand.cpu(), (col, row), out)], 3),
        (RuntimeError, "HBM", [(plane, hand, (col.cpu(), row), out)], 3),
        (ValueError, "col table", [(plane, hand, (col[:-1].contiguous(), row), out)], 3),
        (ValueError, "row table", [(plane, hand, (col, torch.cat([row, row])), out)], 3),
        (ValueError, "tables", [(plane, hand, None, out)], 3),
        (ValueError, "out has shape", [(plane, None, None, wide)], 3),
        (ValueError, "outside 1..31", [(plane, None, None, out)], 0),
        (ValueError, "outside 1..31", [(plane, None, None, out)], 32),
        (ValueError, "no items", [], 3),
    ]
    for exc, text, items, k in bad:
        with pytest.raises(exc, match=text):
            ops.affordance_extract(items, k, stats=stats)
    # the entry point's own refusals, reached past the wrapper: out == in (-1), k out of range (-2)
    lib = haff_lib()
    host = torch.zeros((1, 8), dtype=torch.int64, pin_memory=True)
    h64 = host.numpy()
    h64[0, 0], h64[0, 4] = plane.data_ptr(), plane.data_ptr()
    h64.view("int32")[0, 10:12] = (H, W)
    devcopy = host.to(dev)
    assert lib.haff_affordance_extract(host.data_ptr(), devcopy.data_ptr(), 1, 3, stats.data_ptr(), 0) == -1
    h64[0, 4] = out.data_ptr()
    for k in (0, 32):
        assert lib.haff_affordance_extract(host.data_ptr(), devcopy.data_ptr(), 1, k, stats.data_ptr(), 0) == -2
    h64.view("int32")[0, 11] = 4097
    assert lib.haff_affordance_extract(host.data_ptr(), devcopy.data_ptr(), 1, 3, stats.data_ptr(), 0) == -2
    assert lib.haff_affordance_extract(host.data_ptr(), devcopy.data_ptr(), 0, 3, stats.data_ptr(), 0) == -1
    assert lib.haff_affordance_extract(0, devcopy.data_ptr(), 1, 3, stats.data_ptr(), 0) == -1
    torch.cuda.synchronize()
    assert (out == GUARD).all() and (stats == -7).all() and (plane == 255).all()


def haff_lib():
    import haff
    return haff.load_library()
