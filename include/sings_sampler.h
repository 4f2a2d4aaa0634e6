/*
 * sings_sampler.h -- the corners of the LPIPS patches (sg_lpips_patch_gather of sings_hip.h), drawn on the device.
 *
 * Replaces PatchSampler of utils/image/sampler.py:16-33 (dilate = 0) in front of the LPIPS patch term: with probability
 * ratio_mask the n patches are centred on n distinct pixels of the mask, otherwise their corners are uniform over the image.
 * The reference decides that on the host from a copy of the mask (np.where over every pixel); here two launches read the mask
 * where it lies, and the counter of the random stream advances in device memory: nothing synchronises, and a captured graph
 * draws fresh patches at every replay.
 *
 * The rule -- corners of frame k are a pure function of (mask_k, H, W, P, n, ratio_mask, seed, counter, k):
 *     o = P / 2;  crop = mask[o : H - o, o : W - o], Hc = H - P rows by Wc = W - P columns;  position q = row q / Wc, column q % Wc
 *     valid: mask > 0 (a NaN or a negative value is not);  M = number of valid positions, ranked in row-major order
 *     word(t): word t % 4 of Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (counter & 0xffffffff, counter >> 32, k, t / 4)
 *     bounded(w, R) = (w * R) >> 32 in 64 bits, a value in [0, R) whose bias is at most R / 2^32
 *     masked branch, taken when word(0) < thr and M >= n, thr = (uint64) ((double) ratio_mask * 2^32)  (ratio_mask clamped to [0, 1]):
 *         Floyd's subset sampling: for i = 0 .. n-1:  j = M - n + i;  t = bounded(word(1 + i), j + 1);  t chosen before: t = j
 *         corner i = crop coordinates of the t-th valid position (as in the reference: an index into the CROP used as the
 *         top-left corner in the full image, so the patch is centred on the valid pixel)
 *     uniform branch:  corner i = (bounded(word(1 + 2 i), H - P), bounded(word(2 + 2 i), W - P))
 * Two deviations from the reference: the random stream (counter based, not numpy's global one), and word(0) < thr with M < n --
 * np.random.choice raises there, the device takes the uniform branch and counts the frame (info, state[3]).
 * Integer arithmetic only: two calls with the same state give the same bits.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises.  These functions are not part of SG_ABI_VERSION's table: a library either
 * exports them all or predates this header.
 */
#ifndef SINGS_SAMPLER_H
#define SINGS_SAMPLER_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_PATCH_MAX_N 16               /* most patches per frame */
#define SG_PATCH_CHUNK 4096             /* crop positions counted by one workgroup */
#define SG_PATCH_STATE_WORDS 4          /* int64 words of `state` */
#define SG_PATCH_BRANCH_MASKED 0        /* info[k][1]: n distinct valid pixels */
#define SG_PATCH_BRANCH_UNIFORM 1       /*             uniform corners, by the draw */
#define SG_PATCH_BRANCH_FORCED 2        /*             uniform corners, because M < n */

/* Bytes of the workspace of a K-frame call (0 for sizes the call refuses). */
size_t sg_patch_sampler_ws_bytes(int K, int H, int W, int P);

/* Patch corners of K frames, two launches.  mask [H,W] fp32 at + mask_stride floats per frame (H*W, or 0 = one mask for all
 * frames); origins [K][n][2] (row, col); info [K][2] = (M, branch: SG_PATCH_BRANCH_*); ws: sg_patch_sampler_ws_bytes bytes.
 * state (device, int64 [SG_PATCH_STATE_WORDS]): { next counter, counter of the last call, seed, SG_PATCH_BRANCH_FORCED frames so
 * far }.  The call draws with counter state[0] and leaves state[0] + 1 there, on the device.
 * Refused (status 1, before any HIP call): K outside 1..65535, n outside 1..SG_PATCH_MAX_N, P odd or < 2, H <= P or W <= P (or
 * 2^31 pixels and more), mask_stride neither 0 nor H*W, a NULL mask / state / ws / origins / info. */
int sg_patch_origins(int K, int H, int W, int P, int n, int mask_stride, float ratio_mask, const float *mask, int64_t *state,
                     void *ws, int32_t *origins, int32_t *info, void *stream);

#ifdef __cplusplus
}
#endif
#endif
