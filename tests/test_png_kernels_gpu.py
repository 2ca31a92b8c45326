"""haff_png_measure / haff_png_emit (csrc/png_encode.hip) against tests/png_ref.py, byte for byte, on the smallest planes at which
each rule of the stream can go wrong (png_ref.fixture_planes), in one batch per call pair; the batch layout, repeatability, planes at
odd addresses and the refusals."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/png_ref.py
import png_ref as P   # noqa: E402

pytestmark = pytest.mark.gpu

PLANES = P.fixture_planes()


def _encode(dev, planes, canary=0):
    """(uint32 table, the output bytes, the bytes behind them) of one measure / emit pair over device planes."""
    import torch
    from haff import ops
    table_dev, job = ops.png_measure(planes)
    table = table_dev.cpu().numpy().view(np.uint32)
    total = int(table[-1, 0]) + (int(table[-1, 1]) + 3) // 4 * 4
    out = torch.full((total + canary,), 0xA5, dtype=torch.uint8, device=dev)
    assert ops.png_emit(job, table, out=out) is out
    got = out.cpu().numpy()
    return table, got[:total].tobytes(), got[total:].tobytes()


@pytest.fixture(scope="module")
def encoded(dev):
    """Every fixture plane through ONE call pair, and the restatement of that batch."""
    import torch
    names = list(PLANES)
    table, out, _ = _encode(dev, [torch.from_numpy(PLANES[n]).to(dev) for n in names])
    want_table, want_out = P.table_and_output([PLANES[n] for n in names])
    return names, table, out, want_table, want_out


@pytest.mark.parametrize("name", list(PLANES))
def test_plane_equals_the_restatement(encoded, name):
    names, table, out, want_table, want_out = encoded
    i = names.index(name)
    plane = PLANES[name]
    off, length, adler, zero = (int(v) for v in table[i])
    assert (off, length, zero) == (int(want_table[i, 0]), int(want_table[i, 1]), 0)
    assert adler == zlib.adler32(P.scanlines(plane).tobytes()) == int(want_table[i, 2])
    assert out[off:off + length] == want_out[off:off + length] == P.block(plane)


def test_whole_output_equals_the_restatement(encoded):
    _, table, out, want_table, want_out = encoded
    assert np.array_equal(table, want_table)
    assert out == want_out


def test_mixed_batch_layout_canary_and_repeatability(dev):
    import torch
    planes = [torch.from_numpy(p).to(dev) for p in P.mixed_batch()]
    table, out, behind = _encode(dev, planes, canary=64)
    want_table, want_out = P.table_and_output(P.mixed_batch())
    assert np.array_equal(table, want_table) and out == want_out
    assert behind == b"\xa5" * 64
    end = 0
    for off, length in table[:, :2].tolist():
        assert off % 4 == 0 and off == end
        end = off + (length + 3) // 4 * 4
        assert out[off + length:end] == b"\0" * (end - off - length)
    assert end == len(out)
    table2, out2, _ = _encode(dev, planes)
    assert np.array_equal(table2, table) and out2 == out


def test_planes_at_odd_addresses(dev):
    import torch
    rng = np.random.default_rng(7)
    big = (rng.integers(0, 2, (1 << 16) + 8) * 255).astype(np.uint8)
    big[1000:9000] = 255
    base = torch.from_numpy(big).to(dev)
    views, hosts = [], []
    for start, (H, W) in ((1, (37, 129)), (4803, (5, 515)), (7, (64, 67)), (30001, (1, 4096))):
        views.append(base[start:start + H * W].view(H, W))
        hosts.append(big[start:start + H * W].reshape(H, W))
        assert views[-1].data_ptr() % 2 == 1
    table, out, _ = _encode(dev, views)
    want_table, want_out = P.table_and_output(hosts)
    assert np.array_equal(table, want_table) and out == want_out


def test_refusals(dev):
    """The house codes, from the host tables and the pointers alone: nothing is launched."""
    import torch
    from haff import ops
    from haff.lib import load_library
    lib = load_library()
    stream = torch.cuda.current_stream().cuda_stream
    plane = torch.zeros((6, 10), dtype=torch.uint8, device=dev)
    table_dev, job = ops.png_measure([plane])
    planes, host, dev_planes, ws, _ = job
    table = np.ascontiguousarray(table_dev.cpu().numpy().view(np.uint32))
    total = int(table[0, 0]) + (int(table[0, 1]) + 3) // 4 * 4
    out = torch.full((total + 16,), 0xA5, dtype=torch.uint8, device=dev)

    def measure(host_table, n, table_ptr):
        return lib.haff_png_measure(host_table.data_ptr(), dev_planes.data_ptr(), n, ws.data_ptr(), ws.numel(), table_ptr, stream)

    def emit(n, table_host_ptr, table_dev_ptr, out_bytes):
        return lib.haff_png_emit(host.data_ptr(), dev_planes.data_ptr(), n, ws.data_ptr(), ws.numel(), table_host_ptr, table_dev_ptr,
                                 out.data_ptr(), out_bytes, stream)
    for shape in ((4097, 1), (1, 4097)):
        wide = ops._plane_table([plane])
        wide.numpy().view(np.int32)[2:4] = shape
        assert measure(wide, 1, table_dev.data_ptr()) == -2
        need = ctypes.c_long(0)
        assert lib.haff_png_workspace(wide.data_ptr(), 1, ctypes.addressof(need)) == -2
    assert measure(host, 1, 0) == -1
    assert measure(host, 1, table_dev.data_ptr() + 4) == -1
    assert measure(host, 0, table_dev.data_ptr()) == -1
    assert emit(1, 0, table_dev.data_ptr(), total) == -1
    assert emit(1, table.ctypes.data, 0, total) == -1
    assert emit(0, table.ctypes.data, table_dev.data_ptr(), total) == -1
    assert emit(1, table.ctypes.data, table_dev.data_ptr(), total - 1) == -1
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                        # no refused call wrote a byte
    assert emit(1, table.ctypes.data, table_dev.data_ptr(), total) == 0
    got = out.cpu().numpy()
    assert got[:total].tobytes() == P.table_and_output([np.zeros((6, 10), np.uint8)])[1] and bool((got[total:] == 0xA5).all())


def test_encoder_files_open_in_pillow(dev):
    import io
    import torch
    from PIL import Image
    from haff import png
    names = ["1x1_144", "row_259_0", "checkerboard_33x259", "stripes_7x1031", "rows_differ_40x300"]
    enc = png.PngEncoder()
    files = enc.encode([torch.from_numpy(PLANES[n]).to(dev) for n in names])
    assert enc.host_encodes == 0
    for n, data in zip(names, files):
        H, W = PLANES[n].shape
        assert data == png.wrap(H, W, P.block(PLANES[n]), P.adler_fast(PLANES[n])), n
        assert [k for k, _, ok in P.chunks(data) if ok] == [b"IHDR", b"IDAT", b"IEND"]
        im = Image.open(io.BytesIO(data))
        assert im.mode == "L" and np.array_equal(np.asarray(im), PLANES[n]), n
