"""The device PNG stream as tests/png_ref.py restates it (include/haff_io.h): the restated blocks inflate to the scanlines, png.wrap
makes files Pillow opens, the bit-cost anchors and the Adler formula hold; haff_io.h is locked beside the frozen hot-path ABI; the
flag refusal and the host path of PngEncoder. CPU only."""
import ctypes
import io
import json
import os
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/png_ref.py
import png_ref as P   # noqa: E402

import haff   # noqa: E402
from haff import lib as hlib, png   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = P.fixture_planes()
LETTER = {ctypes.c_void_p: "p", ctypes.c_long: "l", ctypes.c_int: "i", ctypes.c_float: "f"}


@pytest.mark.parametrize("name", list(PLANES))
def test_round_trip(name):
    plane = PLANES[name]
    H, W = plane.shape
    block = P.block(plane)
    raw = P.scanlines(plane).tobytes()
    assert len(block) <= P.bound(H, W)
    inflated = zlib.decompressobj(-15)
    assert inflated.decompress(block) == raw and inflated.eof and inflated.unused_data == b""
    assert P.adler(plane) == P.adler_fast(plane) == zlib.adler32(raw)
    data = png.wrap(H, W, block, P.adler(plane))
    found = P.chunks(data)
    assert [k for k, _, _ in found] == [b"IHDR", b"IDAT", b"IEND"] and all(ok for _, _, ok in found)
    assert found[0][1] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 0, 0, 0, 0])
    assert zlib.decompress(found[1][1]) == raw
    assert found[1][1][:2] == b"\x78\x01" and found[1][1][2:-4] == block and found[2][1] == b""
    im = Image.open(io.BytesIO(data))
    assert im.mode == "L" and im.size == (W, H)
    assert np.array_equal(np.asarray(im), plane)


def test_bit_cost_anchors():
    assert [P.run_bits(n) for n in (1, 2, 3, 4, 258, 259, 260)] == [8, 16, 24, 20, 26, 21, 29]
    assert P.run_bits(1, 143) == 8 and P.run_bits(1, 144) == 9 and P.run_bits(2, 255) == 18 and P.run_bits(4, 255) == 21
    blank = P.block(np.zeros((1024, 1024), np.uint8))
    assert P.run_bits(1025) == 65 and len(blank) == 8322 == (10 + 65 * 1024 + 7) // 8
    for name, plane in PLANES.items():
        assert len(P.block(plane)) <= P.bound(*plane.shape), name
    worst = np.full((3, 5), 200, np.uint8)
    worst[:, ::2] = 150                                     # every byte a 9-bit literal but the filter bytes
    assert len(P.block(worst)) == (10 + 3 * (8 + 9 * 5) + 7) // 8 <= P.bound(3, 5)


def test_adler_formula_is_zlibs():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (3, 7), (64, 67), (300, 257)):
        plane = rng.integers(0, 256, shape, dtype=np.uint8)
        assert P.adler(plane) == zlib.adler32(P.scanlines(plane).tobytes()), shape
    full = np.full((4096, 64), 255, np.uint8)               # sums far past 65521 and 2^32
    assert P.adler_fast(full) == zlib.adler32(P.scanlines(full).tobytes())


def test_io_header_is_locked_beside_the_frozen_abi():
    with open(os.path.join(ROOT, "tests", "golden", "abi_io_signatures.json")) as fh:
        locked = json.load(fh)
    assert sorted(locked) == ["haff_png_emit", "haff_png_measure", "haff_png_workspace"]
    with open(os.path.join(ROOT, "include", "haff_io.h")) as fh:
        protos = hlib.parse_header(fh.read())
    assert {k: "".join(LETTER[t] for t in v) for k, v in protos.items()} == locked
    assert hlib.IO_HEADER_PATH == os.path.join(ROOT, "include", "haff_io.h") and hlib.IO_SYMBOLS == tuple(sorted(locked))
    assert len(haff.EXPORTED_SYMBOLS) == 143 and not [n for n in haff.EXPORTED_SYMBOLS if n.startswith("haff_png")]
    assert not set(locked) & set(hlib._PROTOS)
    if not os.path.exists(hlib.LIB_PATH):
        hlib.build_library()
    lib = hlib.load_library()
    for name, sig in locked.items():
        fn = getattr(lib, name)
        assert "".join(LETTER[t] for t in fn.argtypes) == sig and fn.restype is ctypes.c_int, name
    src = open(os.path.join(ROOT, "2handedafforder_amd", "csrc", "png_encode.hip")).read()
    assert '#include "haff_common.h"' in src and '#include "haff_io.h"' in src
    makefile = open(os.path.join(ROOT, "2handedafforder_amd", "csrc", "Makefile")).read()
    assert " png_encode.hip" in makefile and "build/png_encode.o: ../../include/haff_io.h" in makefile


def test_host_side_refusals_need_no_device():
    """haff_png_workspace is host only: the house codes on a host table, without a GPU."""
    if not os.path.exists(hlib.LIB_PATH):
        hlib.build_library()
    lib = hlib.load_library()

    def workspace(shapes, n=None):
        table = np.zeros((max(len(shapes), 1), 2), dtype=np.int64)
        for i, (H, W) in enumerate(shapes):
            table[i, 0] = 4096                              # any non-null address: nothing is read through it
            table[i, 1:].view(np.int32)[:] = (H, W)
        need = ctypes.c_long(-1)
        rc = lib.haff_png_workspace(table.ctypes.data, len(shapes) if n is None else n, ctypes.addressof(need))
        return rc, need.value
    assert workspace([(3, 5), (7, 2)]) == (0, 3 * 4 * 2 * 7)
    assert workspace([(4096, 4096)])[0] == 0
    assert workspace([(4097, 1)])[0] == -2 and workspace([(1, 4097)])[0] == -2
    assert workspace([(0, 4)])[0] == -1 and workspace([(3, 5)], n=0)[0] == -1
    assert lib.haff_png_workspace(0, 1, 0) == -1


def test_device_png_refuses_score_only_by_name():
    from haff import inference
    with pytest.raises(SystemExit) as e:
        inference.parse_args(["--device_png", "--score_only", "--benchmark-dir", "somewhere"])
    assert "--device_png" in str(e.value) and "--score_only" in str(e.value)
    assert inference.parse_args(["--device_png", "--score", "--benchmark-dir", "somewhere"]).device_png is True
    assert inference.parse_args([]).device_png is False


def test_a_side_over_the_limit_is_encoded_on_the_host(monkeypatch):
    import torch
    from haff import ops

    def no_device(*a, **kw):
        raise AssertionError("a 4097-wide plane went to the device calls")
    monkeypatch.setattr(ops, "png_measure", no_device)
    monkeypatch.setattr(ops, "png_emit", no_device)
    plane = (np.arange(4097) % 251).astype(np.uint8).reshape(1, 4097)
    enc = png.PngEncoder()
    files = enc.encode([torch.from_numpy(plane)])
    assert enc.host_encodes == 1 and len(files) == 1
    want = io.BytesIO()
    Image.fromarray(plane).save(want, format="PNG")
    assert files[0] == want.getvalue()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[0]))), plane)
    assert png.PngEncoder().encode([]) == []
