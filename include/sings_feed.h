/*
 * sings_feed.h -- the training frames on the device: stored as the bytes they came from, drawn and expanded inside the step.
 *
 * Replaces three things the reference decides per step on the host: the frame (RandomIndexIterator, general.py:16-32: a shuffled
 * pass over the F frames, shuffled again when it is used up), the background colour (bg_color = torch.rand(3), gs_trainer.py:238)
 * and the frame's ground truth out of Customdataset.load_data_to_cuda's cache -- four fp32 planes per frame, 16 B per pixel, for
 * data that was born as 8-bit PNGs.  Here the cache is [F][H][W][4] bytes (R, G, B, mask: 4 B per pixel), sg_frame_draw picks the
 * step's frames and colour from a counter in device memory, and sg_frame_expand turns the picked frames into the fp32 planes the
 * loss reads.  Nothing synchronises, and a captured graph draws the next frames at every replay.
 *
 * The rule:
 *     word_s(c, t): word t % 4 of Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (c & 0xffffffff, c >> 32, s, t / 4);
 *                   s = 0 is the order stream, s = 1 the background stream
 *     bounded(w, R) = (w * R) >> 32 in 64 bits, a value in [0, R)
 *     order of epoch e over F frames:  a[i] = i;  for i = F-1 down to 1:  j = bounded(word_0(e, F-1-i), i+1), swap a[i] and a[j]
 *                   -- a pure function of (F, seed, e): it starts from the identity, not from the previous epoch's order, so a
 *                   resumed run can rebuild it
 *     draw number t (t = frames drawn so far) is order(t / F)[t % F];  a step of K frames takes draws c .. c+K-1 and leaves c + K
 *                   (a chunk may straddle an epoch)
 *     background of a step that starts at counter c: channel i = (word_1(c, i) >> 8) * 2^-24, in [0, 1); one colour per step
 *     a stored byte v becomes (float) v / 255.0f, correctly rounded (the library is built with
 *                   -fhip-fp32-correctly-rounded-divide-sqrt): (img / 255).astype(np.float32) for all 256 values.  v * (1 / 255.0f)
 *                   is NOT that: it differs at 126 of the 256 values.
 * One deviation from the reference: the random streams are counter based, not Python's / torch's global ones.
 * Integer arithmetic and one exact conversion: two calls with the same state give the same bits.  Counters stay below 2^63.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises.  These functions are not part of SG_ABI_VERSION's table: a library either
 * exports them all or predates this header.
 */
#ifndef SINGS_FEED_H
#define SINGS_FEED_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_FEED_MAX_FRAMES 16384        /* most frames of a store (the order of an epoch is built in LDS) */
#define SG_FEED_MAX_K 16                /* most frames per step (SG_MAX_FRAMES) */
#define SG_FEED_STATE_WORDS 4           /* int64 words of `state` */

/* The next K frame indices (and the step's background colour), one workgroup.
 * state (device, int64 [SG_FEED_STATE_WORDS]): { next counter, seed, epoch that `order` currently holds (-1: none), counter of the
 * last call }.  order (device, int32 [F]).  The call draws with counter c = state[0], writes idx_out [K] and, with draw_bg != 0,
 * bg_out [3]; it rebuilds `order` whenever the epoch it needs is not the one held, also in the middle of a chunk, and leaves
 * { c + K, seed, the epoch held now, c }.
 * Refused (status 1, before any HIP call): F outside 1..SG_FEED_MAX_FRAMES, K outside 1..SG_FEED_MAX_K, a NULL state / order /
 * idx_out, draw_bg without bg_out. */
int sg_frame_draw(int F, int K, int draw_bg, int64_t *state, int32_t *order, int32_t *idx_out, float *bg_out, void *stream);

/* K frames of the store as fp32 planes.  store [F][H][W][4] bytes (R, G, B, mask); idx (device, int32 [K]); gt [K][3][H][W],
 * mask [K][H][W].  An index outside [0, F) is clamped into it: the kernel cannot fault on a bad index.
 * Refused (status 1, before any HIP call): K outside 1..SG_FEED_MAX_K, H or W < 1 or H*W >= 2^31, F < 1, a NULL pointer. */
int sg_frame_expand(int K, int H, int W, int F, const uint8_t *store, const int32_t *idx, float *gt, float *mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif
