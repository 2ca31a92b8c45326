"""uint8 greyscale planes leave the device as PNG streams (include/haff_io.h states the format, csrc/png_encode.hip makes it).

The planes the command lines write are 0/255 masks, so they are runs. The device turns each plane into one fixed-Huffman DEFLATE
block of "literal, then repeat the previous byte" tokens and its Adler-32; the host reads those few KB back instead of the plane and
puts the container around them: signature, IHDR, one IDAT, IEND, about 60 bytes and two zlib.crc32 calls over what came back. Every
PNG reader accepts the files; they decode to the same pixels as the default route's (Pillow's encoder), at a few times its size.
"""
import struct
import zlib

import numpy as np

from . import ops

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = ops.PNG_MAX_SIDE
_CALL_BYTES = 1 << 30          # worst-case block bytes one measure / emit pair is given: below the library's 2^31


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def wrap(H, W, block_bytes, adler):
    """The PNG file of an 8-bit greyscale H x W plane whose scanlines (filter byte 0, then the pixels) are the DEFLATE stream
    `block_bytes` with Adler-32 `adler`: signature, IHDR, one IDAT = zlib header 78 01 | block | Adler-32 big-endian, IEND."""
    ihdr = struct.pack(">IIBBBBB", int(W), int(H), 8, 0, 0, 0, 0)
    idat = b"\x78\x01" + bytes(block_bytes) + struct.pack(">I", int(adler) & 0xffffffff)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"")


def pillow_bytes(plane_u8):
    """The file Image.fromarray(plane).save(path) writes, as bytes."""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(plane_u8)).save(buf, format="PNG")
    return buf.getvalue()


class PngEncoder:
    """encode(planes) -> the PNG file of every plane, as bytes, in order. planes: uint8 CUDA tensors [H, W] of any shapes and values.
    One measure call, one read of the 16-byte-per-plane table, one emit call into an output of exactly the size the table says and
    one read of it; the size is known before anything is written, so there is no overflow case. A plane with a side above MAX_SIDE
    is read back whole and encoded by Pillow, and counted in `host_encodes`; there is no other fallback."""

    def __init__(self):
        self.host_encodes = 0

    def encode(self, planes):
        planes = list(planes)
        files = [None] * len(planes)
        batch, worst = [], 0
        for i, p in enumerate(planes):
            H, W = (int(s) for s in p.shape)
            if H > MAX_SIDE or W > MAX_SIDE:
                self.host_encodes += 1
                files[i] = pillow_bytes(p.cpu().numpy())
                continue
            bound = ops.png_block_bound(H, W)
            if batch and (worst + bound > _CALL_BYTES or len(batch) == ops.PNG_MAX_PLANES):   # past any CLI's chunk: a second pair of calls
                self._device(planes, batch, files)
                batch, worst = [], 0
            batch.append(i)
            worst += bound + 3
        if batch:
            self._device(planes, batch, files)
        return files

    def _device(self, planes, batch, files):
        table_dev, job = ops.png_measure([planes[i].contiguous() for i in batch])
        table = table_dev.cpu().numpy().view(np.uint32)
        out = ops.png_emit(job, table).cpu().numpy()
        for k, i in enumerate(batch):
            off, length, adler = (int(v) for v in table[k, :3])
            H, W = planes[i].shape
            files[i] = wrap(H, W, out[off:off + length].tobytes(), adler)


def report_host_encodes(encoder):
    """The line the command lines print when a plane was too large for the device route."""
    if encoder is not None and encoder.host_encodes:
        print(f"--device_png: {encoder.host_encodes} planes with a side above {MAX_SIDE} encoded by Pillow on the host")
