"""csrc/contour_hausdorff.hip against the host route (tests/hausdorff_ref.py: cvlite's vertex lists, integer distances): ordered
vertex lists, counts, flags and both squared distances, exact equality throughout. The fixtures assume the labelling kernel's
32 x 32 LDS tile (hausdorff_ref.TILE) and the distance kernel's 1024-point LDS chunk (hausdorff_ref.CHUNK)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/hausdorff_ref.py
import hausdorff_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

MAX_VERTICES = 4096            # above the 3 CHUNK + 1 fixture and the 855 x 855 pair


@pytest.fixture(scope="module")
def batch():
    """Every fixture in ONE call's worth of planes and pairs, with the host reference computed once:
    (planes, pairs, expected vertex lists, expected result rows)."""
    assert R.TILE == 32 and R.CHUNK == 1024
    planes, pairs = [], []

    def add(m):
        planes.append(np.array(m, dtype=np.uint8, order="C"))
        return len(planes) - 1
    small = R.small_planes()
    for m in small.values():                                 # every small plane against its point mirror
        pairs.append((add(m), add(m[::-1, ::-1])))
    e, f = add(small["empty"]), add(small["full"])            # the two empty rules' cases
    pairs += [(e, f), (f, e)]
    noise = [add(m * 255) for m in R.random_planes()]         # on is any non-zero byte
    pairs += [(noise[k], noise[(k + 7) % 40]) for k in range(40)]
    d = {k: add(m) for k, m in R.distance_planes().items()}
    pairs += [(d[a], d[b]) for a, b in R.DISTANCE_PAIRS]
    w = [add(m) for m in R.wide_planes()]
    pairs += [(w[0], w[1]), (w[1], w[0]), (w[0], w[0])]
    real = [add(m) for m in R.real_pair()]
    pairs += [(real[0], real[1]), (real[1], real[0])]
    verts = [R.vertices(m) for m in planes]
    assert max(len(v) for v in verts) <= MAX_VERTICES and len(verts[real[0]]) > 8 and len(verts[real[1]]) > 8
    rows = [R.expected_row(verts[b], verts[p]) for b, p in pairs]
    return planes, pairs, verts, rows


def _run(dev, planes, pairs, max_vertices, buffer=None):
    import torch
    import haff  # noqa: F401
    from haff import ops
    tensors = [torch.from_numpy(m).to(dev) for m in planes]
    res, v, n = ops.contour_hausdorff(tensors, pairs, max_vertices=max_vertices, return_vertices=True if buffer is None else buffer)
    torch.cuda.synchronize()
    return res.cpu().numpy(), v.cpu().numpy(), n.cpu().numpy()


def test_vertex_lists_counts_flags_and_distances_equal_the_host_route(dev, batch):
    import torch
    planes, pairs, verts, rows = batch
    n = len(planes)
    buf = torch.full((n * MAX_VERTICES * 4 + n * 4,), 0x5A, dtype=torch.uint8, device=dev)
    res, v, counts = _run(dev, planes, pairs, MAX_VERTICES, buf)
    assert counts.tolist() == [len(x) for x in verts]
    for i, want in enumerate(verts):
        assert v[i, :len(want)].tolist() == want.tolist(), (i, planes[i].shape)
        assert (v[i, len(want):] == 0x5A5A).all(), i                                  # nothing written past the list
    assert res.tolist() == rows
    big = max(max(r[2], r[3]) for r in rows)
    assert big == 4095 ** 2 + 1 and sum(r[2] != r[3] for r in rows) > 20 and sum(r[0] == 0 or r[1] == 0 for r in rows) >= 4
    # the same numbers without the vertex buffer (the lists then live in the workspace), and bit for bit on a second run
    from haff import ops
    tensors = [torch.from_numpy(m).to(dev) for m in planes]
    again = ops.contour_hausdorff(tensors, pairs, max_vertices=MAX_VERTICES)
    assert again.dtype == torch.int32 and again.cpu().numpy().tolist() == rows
    buf2 = torch.full_like(buf, 0x5A)
    res2, v2, counts2 = _run(dev, planes, pairs, MAX_VERTICES, buf2)
    assert res2.tobytes() == res.tobytes() and v2.tobytes() == v.tobytes() and counts2.tobytes() == counts.tobytes()


@pytest.mark.parametrize("spare", [-1, 0, 1])
def test_capacity_and_guard_words(dev, spare):
    """A contour of V = 26 vertices at max_vertices V - 1, V, V + 1: the overflow flag only at V - 1 (the count is still V, the
    first V - 1 vertices are written, the distances are 0), and no byte outside a plane's list changes."""
    import torch
    V = 26
    cap = R.many_vertices(V, (8, 128))
    planes = [cap, R._on(8, 128, [(70, 4)]), cap[::-1, ::-1].copy()]
    pairs = [(0, 2), (0, 1), (1, 2), (1, 1)]
    verts = [R.vertices(m) for m in planes]
    assert [len(x) for x in verts] == [V, 1, V]
    mv = V + spare
    body = 3 * mv * 4 + 3 * 4
    buf = torch.full((body + 64,), 0xA5, dtype=torch.uint8, device=dev)
    res, v, counts = _run(dev, planes, pairs, mv, buf)
    assert counts.tolist() == [V, 1, V]
    for i, want in enumerate(verts):
        kept = min(len(want), mv)
        assert v[i, :kept].tolist() == want[:kept].tolist()
        assert (v[i, kept:].view(np.uint16) == 0xA5A5).all()
    assert (buf[body:].cpu().numpy() == 0xA5).all()
    over = spare < 0
    flags = [R.OVERFLOW_BENCH | R.OVERFLOW_PRED, R.OVERFLOW_BENCH, R.OVERFLOW_PRED, 0] if over else [0, 0, 0, 0]
    assert res.tolist() == [R.expected_row(verts[b], verts[p], f) for (b, p), f in zip(pairs, flags)]
    assert all(r[2] == r[3] == 0 for r in res.tolist()[:3]) == over


def test_has_no_cpu_fallback():
    import torch
    import haff  # noqa: F401
    from haff import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.contour_hausdorff([torch.zeros((4, 4), dtype=torch.uint8)], [(0, 0)])
