/*
 * sings_png.h -- K uint8 frames to K complete PNG files on the device, in four launches.
 *
 * Every picture the reference writes is a PNG (animate(keep_images=True), the training picture, the turntable, the progress sheets).
 * Here the uint8 frames a launch already produces (sg_frames_to_u8, sg_image_sheets) are encoded where they are; sings_amd/png.py
 * holds the numpy restatement the bytes are tested against.  Everything is integer arithmetic.
 *
 * The file.  The PNG signature; IHDR (width, height, bit depth 8, colour type 2, compression 0, filter 0, interlace 0); an IDAT whose
 * data is the zlib header 78 01; one IDAT per segment; an IDAT whose data is 03 00 (an empty final block of the fixed code) and the
 * big-endian Adler-32 of all scanline bytes; IEND.  No ancillary chunks.  `header` is the first SG_PNG_HEADER_BYTES bytes (signature
 * .. the first IDAT), built by the caller; every other chunk's CRC-32 is computed on the device.
 *
 * Scanlines.  A filter byte, then 3 * width bytes R G B (the frame's B G R swapped while reading with `bgr`); bpp = 3, the row above
 * the first is zeros.  filter: SG_PNG_FILTER_NONE .. SG_PNG_FILTER_PAETH for every row, or SG_PNG_FILTER_ADAPTIVE: per row the type
 * 0..4 with the smallest sum of |filtered byte read as int8| over the 3 * width bytes, ties to the lowest type.  Average is
 * floor((a + b) / 2); Paeth breaks ties in the order a, b, c.
 *
 * Segments.  rows_per_segment consecutive scanlines (the last segment may be short), n <= SG_PNG_MAX_SEGMENT_BYTES bytes, compressed
 * on their own.  Tokens: per maximal run of L equal bytes inside the segment the literal, then of the m = L - 1 further bytes
 * match(258, distance 1) while m >= 258, then match(m, 1) if m >= 3, else m literals; the segment ends with symbol 256.  Candidates:
 * table 0 is the fixed code (BTYPE 01), tables 1 .. SG_PNG_TABLES - 1 dynamic codes (BTYPE 10) whose whole block prefix is a constant
 * bit string in `tables`; candidate SG_PNG_TABLES is the stored form.  A coded segment is prefix, tokens, then an empty stored block
 * (bits 000, zeros to the byte boundary, 00 00 FF FF): ceil((prefix + tokens + 3) / 8) + 4 bytes.  A stored segment is 00, LEN, NLEN,
 * the n bytes: n + 5.  The smallest candidate is taken, ties to the lowest index -- or candidate `force` (0 .. SG_PNG_TABLES) for every
 * segment; force = -1 chooses.  Unforced, the largest file a frame can become is header_bytes + sum(n + 17) + 30.
 *
 * tables: SG_PNG_TABLE_WORDS 32-bit words on the device, the caller's (sings_amd/png.py device_tables):
 *     [SG_PNG_TABLE_STRIDE t, + 513)   per table t: value << 8 | bits of literal v at v, of end of block at 256, of a match of m bytes
 *                                      at 257 + m - 3 (the length symbol's code bit-reversed, its extra bits above it; `bits` counts
 *                                      the distance symbol 0 as well, whose bits are zeros)
 *     [SG_PNG_T_PREFIX + SG_PNG_PREFIX_STRIDE t, ..)   the bits of table t's block prefix, then the prefix itself, LSB first
 *     [SG_PNG_T_CRC, + 256)            the CRC-32 byte table (reflected, polynomial EDB88320)
 *     [SG_PNG_T_POW, + SG_PNG_POW_WORDS)   x^(8 * 2^j) modulo the CRC polynomial
 *
 * Output.  out: K rows of `capacity` bytes; sizes[k]: the bytes of frame k's file, or -needed when it needs more than `capacity`
 * -- such a frame writes nothing to `out` at all.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises or allocates (legal inside a graph capture).  Bitwise deterministic: integer
 * atomics on LDS only.  These functions are not part of SG_ABI_VERSION's table: a library either exports them or predates this header.
 */
#ifndef SINGS_PNG_H
#define SINGS_PNG_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_PNG_MAX_FRAMES 16            /* K per call */
#define SG_PNG_MAX_WIDTH 10922          /* a scanline, 1 + 3 * width bytes, must fit in a segment */
#define SG_PNG_MAX_HEIGHT 65535
#define SG_PNG_MAX_SEGMENT_BYTES 32768
#define SG_PNG_HEADER_BYTES 47
#define SG_PNG_TABLES 5                 /* T: the fixed code and four dynamic codes; candidate T is the stored form */
#define SG_PNG_TABLE_STRIDE 520
#define SG_PNG_PREFIX_STRIDE 48
#define SG_PNG_T_PREFIX 2600            /* SG_PNG_TABLES * SG_PNG_TABLE_STRIDE */
#define SG_PNG_T_CRC 2840               /* SG_PNG_T_PREFIX + SG_PNG_TABLES * SG_PNG_PREFIX_STRIDE */
#define SG_PNG_T_POW 3096               /* SG_PNG_T_CRC + 256 */
#define SG_PNG_POW_WORDS 20
#define SG_PNG_TABLE_WORDS 3120
#define SG_PNG_FILTER_NONE 0
#define SG_PNG_FILTER_SUB 1
#define SG_PNG_FILTER_UP 2
#define SG_PNG_FILTER_AVERAGE 3
#define SG_PNG_FILTER_PAETH 4
#define SG_PNG_FILTER_ADAPTIVE 5
#define SG_PNG_LAYOUT_WORDS 5
/* words of sg_png_layout's result */
#define SG_PNG_L_WS_BYTES 0             /* bytes of the workspace of K frames */
#define SG_PNG_L_SEGMENTS 1             /* segments per frame */
#define SG_PNG_L_SEGMENT_BYTES 2        /* n of every segment but the last */
#define SG_PNG_L_SLOT_PITCH 3           /* bytes of a segment's slot in the workspace (any forced candidate fits) */
#define SG_PNG_L_WORST_BYTES 4          /* the largest file a frame can become unforced: the default capacity */

/* Refused by both (status 1, before any HIP call): width outside 1..SG_PNG_MAX_WIDTH, height outside 1..SG_PNG_MAX_HEIGHT, K outside
 * 1..SG_PNG_MAX_FRAMES, rows_per_segment < 1 or a segment of more than SG_PNG_MAX_SEGMENT_BYTES bytes, header_bytes < 1, a frame
 * whose largest possible file reaches 2^31 bytes. */
int sg_png_layout(int width, int height, int K, int rows_per_segment, int header_bytes, size_t out[SG_PNG_LAYOUT_WORDS]);

/* frames: uint8 [K, height, width, 3], R G B per pixel (B G R with bgr).  ws: ws_bytes >= out[SG_PNG_L_WS_BYTES] of the same
 * arguments, 16-byte aligned.  Also refused: a NULL pointer, filter outside 0..5, force outside -1..SG_PNG_TABLES, capacity < 1 or
 * >= 2^31, a workspace too small or misaligned. */
int sg_png_encode_frames(int K, int width, int height, int rows_per_segment, int filter, int bgr, int force, const uint8_t *frames,
                         const void *tables, const uint8_t *header, int header_bytes, void *ws, size_t ws_bytes, uint8_t *out,
                         size_t capacity, int32_t *sizes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
