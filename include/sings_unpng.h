/*
 * sings_unpng.h -- the zlib streams of n PNG files to the frame store on the device, in two launches.
 *
 * A training kit holds its pictures as PNG files (images/: 8-bit RGB or RGBA; masks/: 8-bit grey); the reference reads them with
 * cv2.imread, one file after the other (Customdataset.py:235-236).  Here the host walks the chunks and joins every file's IDAT
 * payloads (sings_amd/unpng.py parse_png); the inflate, the unfilter and the scatter into the uint8 [F,H,W,4] store of
 * include/sings_feed.h happen on the device.  sings_amd/unpng.py also holds the Python restatement (inflate_host, unfilter_host) the
 * statuses and the bytes are tested against.  Everything is integer arithmetic.
 *
 * The stream table.  int64 [n, SG_UNPNG_TABLE_COLS] on the device, one row per stream:
 *     SG_UNPNG_T_OFFSET, SG_UNPNG_T_LENGTH   where the zlib stream lies in `streams`, in bytes.  offset + length lies inside `streams`:
 *                                            the caller's promise, as the extent of every pointer is
 *     SG_UNPNG_T_WIDTH, SG_UNPNG_T_HEIGHT    of the picture, from its IHDR
 *     SG_UNPNG_T_CHANNELS                    1 (colour type 0), 3 (colour type 2) or 4 (colour type 6); bit depth 8, no interlace
 *     SG_UNPNG_T_DEST                        frame * 4 + first_channel
 * A 3- or 4-channel stream writes channels 0..2 of its frame (first_channel 0; the alpha of a 4-channel stream is dropped, as
 * cv2.imread followed by [..., :3] drops it); a 1-channel stream writes channel 3, the mask (first_channel 3).
 *
 * Inflate (launch 1): one wave per stream, the whole of RFC 1950 / RFC 1951 -- stored blocks, the fixed code, dynamic codes, lengths
 * 3..258, distances 1..32 768, copies longer than their distance.  The h * (1 + w * channels) filtered scanline bytes go to the
 * stream's slot of the workspace: the workspace is divided evenly, slot pitch = (ws_bytes / n) rounded down to 16 bytes.  The
 * Adler-32 behind the last block is checked; bytes behind it are ignored, as zlib ignores them.  A code-length set is refused when it
 * is over-subscribed, or incomplete unless its longest code is one bit (zlib's rule), or has no end-of-block code.  A distance may
 * reach further back than the window size the zlib header declares, up to 32 768: zlib reads such a stream, so it is read here.
 *
 * Unfilter and scatter (launch 2): a wave per scanline.  A row of type None or Sub depends on no other row: Sub is a prefix sum
 * modulo 256 per channel.  Rows of type Up, Average and Paeth are walked downwards, in order, by the wave of the None / Sub row (or
 * the first row) above them.  The row above the first is zeros; Average is floor((a + b) / 2); Paeth breaks ties in the order a, b, c.
 *
 * status: int32 [n], 0 or the first error of the stream (SG_UNPNG_E_*).  A failed stream writes nothing to `dst` and does not disturb
 * any other stream of the call.  No input can make a launch fault or hang: every loop is bounded by the stream's length or by its
 * raw length, every table index and every distance is checked, and decoding stops at the first error.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error() before any HIP call, nothing synchronises or allocates.  Bitwise deterministic.  These functions
 * are not part of SG_ABI_VERSION's table: a library either exports them or predates this header.
 */
#ifndef SINGS_UNPNG_H
#define SINGS_UNPNG_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_UNPNG_MAX_STREAMS 65535      /* n per call */
#define SG_UNPNG_MAX_ROW_BYTES 16384    /* width * channels: two rows are kept in LDS while a chain of rows is walked */
#define SG_UNPNG_MAX_HEIGHT 65535
#define SG_UNPNG_TABLE_COLS 6
#define SG_UNPNG_T_OFFSET 0
#define SG_UNPNG_T_LENGTH 1
#define SG_UNPNG_T_WIDTH 2
#define SG_UNPNG_T_HEIGHT 3
#define SG_UNPNG_T_CHANNELS 4
#define SG_UNPNG_T_DEST 5
#define SG_UNPNG_LAYOUT_WORDS 2
/* words of sg_unpng_layout's result */
#define SG_UNPNG_L_WS_BYTES 0           /* bytes of the workspace of n_streams streams */
#define SG_UNPNG_L_SLOT_PITCH 1         /* bytes of a stream's slot: max_raw_bytes rounded up to 16 */

/* per-stream status.  1..15: the stream (csrc/sg_inflate.h gives the same code on the host); 16..: its table row and its scanlines */
#define SG_UNPNG_OK 0
#define SG_UNPNG_E_INPUT 1              /* the stream ends inside a header, a block or the Adler-32 */
#define SG_UNPNG_E_HEADER 2             /* not a zlib header: method, window size, check bits or a preset dictionary */
#define SG_UNPNG_E_BLOCK_TYPE 3         /* block type 3 */
#define SG_UNPNG_E_STORED 4             /* a stored block whose NLEN is not the complement of LEN */
#define SG_UNPNG_E_COUNTS 5             /* HLIT > 286 or HDIST > 30 symbols */
#define SG_UNPNG_E_CODE_LENGTHS 6       /* the code-length code is over-subscribed or incomplete */
#define SG_UNPNG_E_REPEAT 7             /* a repeat with no previous length, or one that runs past HLIT + HDIST */
#define SG_UNPNG_E_NO_END 8             /* no code for the end-of-block symbol */
#define SG_UNPNG_E_LITLEN_SET 9         /* the literal/length code is over-subscribed or incomplete */
#define SG_UNPNG_E_DIST_SET 10          /* the distance code is over-subscribed or incomplete */
#define SG_UNPNG_E_LITLEN_SYMBOL 11     /* a bit pattern that is no literal/length code, or symbol 286 / 287 */
#define SG_UNPNG_E_DIST_SYMBOL 12       /* a bit pattern that is no distance code, or symbol 30 / 31 */
#define SG_UNPNG_E_DISTANCE 13          /* a distance before the start of the output */
#define SG_UNPNG_E_OUTPUT_LONG 14       /* more raw bytes than h * (1 + w * channels) */
#define SG_UNPNG_E_OUTPUT_SHORT 15      /* the last block ends with fewer */
#define SG_UNPNG_E_ADLER 16             /* the Adler-32 of the raw bytes is not the stream's */
#define SG_UNPNG_E_TABLE 17             /* a table row: negative offset or length, channels not 1 / 3 / 4, width * channels or height
                                           out of range, a frame outside 0..F-1, a first channel that is not the stream's */
#define SG_UNPNG_E_SIZE 18              /* width or height is not the store's */
#define SG_UNPNG_E_WORKSPACE 19         /* the raw bytes do not fit the stream's slot */
#define SG_UNPNG_E_FILTER 20            /* a scanline's filter byte is not 0..4 */

/* Refused (status 1, before any HIP call): a NULL pointer, n_streams outside 1..SG_UNPNG_MAX_STREAMS, max_raw_bytes < 1, a workspace
 * of 2^40 bytes or more. */
int sg_unpng_layout(int n_streams, size_t max_raw_bytes, size_t out[SG_UNPNG_LAYOUT_WORDS]);

/* streams: uint8, the concatenated zlib streams.  table: int64 [n, SG_UNPNG_TABLE_COLS].  ws: ws_bytes >= 16 n, 16-byte aligned.
 * dst: uint8 [F, H, W, 4].  status: int32 [n].  Also refused: n outside 1..SG_UNPNG_MAX_STREAMS, F < 1, H outside
 * 1..SG_UNPNG_MAX_HEIGHT, W < 1 or 4 W > SG_UNPNG_MAX_ROW_BYTES, F H W >= 2^40, a workspace too small or misaligned. */
int sg_unpng_decode(int n, const uint8_t *streams, const int64_t *table, void *ws, size_t ws_bytes, uint8_t *dst, int F, int H, int W,
                    int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
