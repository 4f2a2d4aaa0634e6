/*
 * sings_jpeg.h -- K uint8 frames to K complete baseline JPEG files on the device, in four launches.
 *
 * The reference makes its videos by shelling out to ffmpeg (create_video, utils/general.py:36).  Here the uint8 frames an animation
 * launch already produces (sg_frames_to_u8) are encoded where they are; sings_amd/video.py wraps the files into a Motion-JPEG AVI.
 *
 * The stream.  Baseline sequential DCT (SOF0), 8 bit, Y/Cb/Cr at 4:4:4: an MCU is one 8 x 8 pixel block -- a Y, a Cb and a Cr
 * coefficient block.  `header` is every byte in front of the entropy-coded data (SOI .. SOS), built by the caller; the call appends
 * the entropy-coded segments -- restart_interval MCUs each, the last one short -- segment i followed by RST(i mod 8), the last by EOI.
 * A width or height that is no multiple of 8 repeats the last column / row.
 *
 * The arithmetic (fp32, every multiply and add rounded on its own, sums left to right; sings_amd/video.py jpeg_coefficients is the
 * numpy restatement, byte for byte):
 *     Y  = (0.299 R + 0.587 G) + 0.114 B - 128      Cb = ((-0.168736 R) + (-0.331264 G)) + 0.5 B
 *     Cr = (0.5 R + (-0.418688 G)) + (-0.081312 B)
 *     t[y][u] = sum_x C[u][x] s[y][x]   then   F[v][u] = sum_y C[v][y] t[y][u]      (x, y ascending from the x = 0 product)
 *     q = rint(F / Q), ties to even; DC clamped to [-1024, 1023], AC to [-1023, 1023]
 * Entropy coding as the standard writes it; the DC predictor is the previous block of the same component in the same restart
 * segment, 0 at a segment's start; a segment's last byte is padded with 1-bits; every 0xFF of entropy data is followed by 0x00.
 *
 * tables: SG_JPEG_TABLE_WORDS 32-bit words on the device, the caller's (sings_amd/video.py device_tables):
 *     [0, 64)      float    DCT basis C[u][x] at 8 u + x
 *     [64, 192)    float    quantisers of table 0 (Y) and table 1 (Cb, Cr), natural order (8 v + u)
 *     [192, 256)   int32    zig-zag position of natural index 8 v + u
 *     [256, 800)   uint32   per table class c (0: DC0 / AC0, 1: DC1 / AC1) at 256 + SG_JPEG_HUFF_STRIDE c: code << 8 | length of the
 *                           16 DC categories, then of the 256 AC run/size symbols
 *
 * Output.  out: K rows of `capacity` bytes; sizes[k]: the bytes of frame k's file, or -needed when it needs more than `capacity`
 * -- such a frame writes nothing to `out` at all; the caller grows the buffer and encodes again.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises or allocates (legal inside a graph capture).  Bitwise deterministic: integer
 * atomics on LDS only.  These functions are not part of SG_ABI_VERSION's table: a library either exports them or predates this header.
 */
#ifndef SINGS_JPEG_H
#define SINGS_JPEG_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_JPEG_MAX_FRAMES 16           /* K per call */
#define SG_JPEG_MAX_DIM 65535           /* width, height (a SOF0 dimension is 16 bit) */
#define SG_JPEG_TABLE_WORDS 800
#define SG_JPEG_HUFF_STRIDE 272
#define SG_JPEG_MCU_BYTES 1248          /* most bytes an MCU's entropy data takes, stuffing included: 3 blocks of at most 1664 bits, doubled */
#define SG_JPEG_LAYOUT_WORDS 6
/* words of sg_jpeg_layout's result */
#define SG_JPEG_L_WS_BYTES 0            /* bytes of the workspace of K frames */
#define SG_JPEG_L_MCUS 1                /* MCUs per frame */
#define SG_JPEG_L_SEGMENTS 2            /* restart segments per frame */
#define SG_JPEG_L_SLOT_PITCH 3          /* bytes of a segment's slot in the workspace (its worst case) */
#define SG_JPEG_L_WORST_BYTES 4         /* the largest file a frame can become */
#define SG_JPEG_L_DEFAULT_CAPACITY 5    /* header_bytes + width * height * 3 / 2 */

/* Refused by both (status 1, before any HIP call): width or height outside 1..SG_JPEG_MAX_DIM, K outside 1..SG_JPEG_MAX_FRAMES,
 * restart_interval outside 1..65535, header_bytes < 1, a frame whose largest possible file reaches 2^31 bytes. */
int sg_jpeg_layout(int width, int height, int K, int restart_interval, int header_bytes, size_t out[SG_JPEG_LAYOUT_WORDS]);

/* frames: uint8 [K, height, width, 3], R G B per pixel (B G R with bgr).  ws: ws_bytes >= out[SG_JPEG_L_WS_BYTES] of the same
 * arguments, 16-byte aligned.  Also refused: a NULL pointer, capacity < 1 or >= 2^31, a workspace too small or misaligned. */
int sg_jpeg_encode_frames(int K, int width, int height, int restart_interval, int bgr, const uint8_t *frames, const void *tables,
                          const uint8_t *header, int header_bytes, void *ws, size_t ws_bytes, uint8_t *out, size_t capacity,
                          int32_t *sizes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
