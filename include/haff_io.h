/*
 * haff_io.h — file-format helpers of libhaff_hip.so, beside the frozen hot-path ABI of haff_hip.h.
 *
 * Nothing here replaces an op of the reference's per-frame path: these entry points turn results that already sit in HBM into the
 * bytes of the files the reference's command lines write (inference.py:299,331 and robot_demo.py:300-327: cv2.imwrite of a mask
 * plane), so that the host reads back a compressed stream instead of the plane. Same conventions as haff_hip.h: plain pointers,
 * sizes, `stream` (a hipStream_t as void*, 0 = null stream) last, `int` return (0 ok, -1 bad argument, -2 unsupported shape,
 * -3 launch error), caller-owned DEVICE pointers unless marked "host", no internal allocation, kernels are only enqueued.
 *
 * ---- uint8 greyscale planes as PNG streams (csrc/png_encode.hip; the format is restated in png.py and tests/png_ref.py) ----
 * For a plane u8 [H][W] of any values: scanline y = the filter byte 0 then its W pixels (S = W + 1 bytes), N = H S bytes in all.
 * The stream is ONE DEFLATE block (RFC 1951) with the fixed Huffman code: header bits BFINAL = 1, BTYPE = 01, the tokens of
 * scanlines 0 .. H - 1, end-of-block, zero bits up to a byte. Tokens: for every maximal run of n equal bytes v inside one scanline
 * (runs never cross scanlines) the literal v, then with r = n - 1: r / 258 matches (length 258, distance 1), then for m = r % 258
 * one match (length m, distance 1) if m >= 3, else m literals v. Nothing else is emitted; the output is a function of the plane
 * alone (bitwise reproducible). The block of a plane is at most ceil((10 + 9 S H) / 8) bytes. The Adler-32 is that of the N
 * uncompressed bytes (RFC 1950). The PNG container (signature, IHDR, one IDAT = 78 01 | block | Adler-32 big-endian, IEND) is host
 * work: png.wrap.
 */
#ifndef HAFF_IO_H
#define HAFF_IO_H

#ifdef __cplusplus
extern "C" {
#endif

/* One plane of a haff_png_* batch: 16 bytes, `plane` a DEVICE pointer to u8 [H][W] at any address, rows contiguous. */
typedef struct haff_png_plane {
  const unsigned char* plane;
  int H, W;
} haff_png_plane;

/* Host only: *bytes_out = the workspace haff_png_measure and haff_png_emit need for these planes (a HOST table). n_planes < 1 or
 * above 4096, a null pointer, a side < 1: -1; a side above 4096, or planes whose blocks could pass 2^31 bytes in all: -2. */
int haff_png_workspace(const haff_png_plane* planes_host, int n_planes, long* bytes_out);

/* Measures every plane's block. planes_host / planes_dev: the same n_planes descriptors in host and in device memory. workspace:
 * device, 16-B aligned, at least haff_png_workspace's bytes; it carries every scanline's bit offset inside its plane's block to
 * haff_png_emit. table: DEVICE u32 [n_planes][4], 16-B aligned = {byte offset of the plane's block in the output (4-B aligned,
 * planes back to back in table order), byte length of the block, Adler-32 of the uncompressed data, 0}; every word is written.
 * Refusals as haff_png_workspace, and -1 for a null or misaligned table or workspace, or a workspace too small; before any launch. */
int haff_png_measure(const haff_png_plane* planes_host, const haff_png_plane* planes_dev, int n_planes, void* workspace,
                     long workspace_bytes, unsigned* table, void* stream);

/* Writes the blocks. table_host: the table haff_png_measure wrote for these planes, read back by the caller (HOST); table_dev: the
 * same table in device memory; workspace: as haff_png_measure left it. out: DEVICE, 4-B aligned, out_bytes >= the size the table
 * implies = offset + length of the last plane, rounded up to 4. The call zeroes that many bytes of out (a memset on the stream),
 * then ORs every token into place: bytes between a block's end and the next offset stay zero, nothing behind that size is touched.
 * Refusals as haff_png_measure, and -1 for a table_host that is not one haff_png_measure can have written for these planes
 * (offsets not back to back, a length above the plane's bound) or an `out` smaller than it says; before any launch. */
int haff_png_emit(const haff_png_plane* planes_host, const haff_png_plane* planes_dev, int n_planes, const void* workspace,
                  long workspace_bytes, const unsigned* table_host, const unsigned* table_dev, unsigned char* out, long out_bytes,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HAFF_IO_H */
