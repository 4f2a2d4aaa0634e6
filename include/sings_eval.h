/*
 * sings_eval.h -- the evaluation entry points of libsings_hip.so: what a validation pass computes from rendered frames.
 *
 * Replaces, for the PSNR and SSIM figures of SinGaussianTrainer.validate (sings/rec/trainer/gs_trainer.py:577-585), the chain
 *     image = render_pkg["render"]                       (clamped to [0,1]: gs_renderer_single.py:96)
 *     image, gt = image * mask, gt * mask                (dataset `zju` only: :580-582)
 *     psnr(image, gt).mean()                             (utils/image/image.py:15-17: PER-CHANNEL mse, mean of three PSNRs)
 *     ssim(image, gt).mean()                             (losses/utils.py:39-70: 11 x 11, sigma 1.5, zero padding, unmasked)
 * for K frames in one launch.  (LPIPS: sg_lpips_forward of sings_hip.h.)
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises.  These functions are not part of SG_ABI_VERSION's table: a library either
 * exports them all or predates this header.
 */
#ifndef SINGS_EVAL_H
#define SINGS_EVAL_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_METRICS_CLAMP 1          /* flags bit 0: clamp pred to [0,1] first (pred is the UNCLAMPED render, 'render_raw') */
#define SG_METRICS_FLOATS 8         /* floats per frame of `metrics` */
/* metrics[f]: [0..2] per-channel MSE, [3..5] per-channel PSNR = 20 log10(1 / sqrt(mse)) dB (+inf where the MSE is 0),
 * [6] mean of the three PSNRs (+inf if one of them is), [7] mean of the SSIM map over its 3 H W elements.
 * The sums are fp64 in a fixed order (no atomics): two calls give the same bits, and a frame's bits depend neither on K nor on the
 * frame's position in the batch.  PSNR is formed in fp64 from the fp64 MSE and rounded once. */

/* Geometry of the kernel, for tests at its edges: a wave marches down a strip of SG_METRICS_STRIP_COLS columns; an image is cut
 * into chunks of at least SG_METRICS_CHUNK_ROWS rows (an image of up to that many rows is one chunk). */
#define SG_METRICS_STRIP_COLS 64
#define SG_METRICS_CHUNK_ROWS 32

/* Bytes of the workspace of a K-frame call (0 for sizes the call refuses). */
size_t sg_image_metrics_ws_bytes(int K, int width, int height);

/* PSNR and SSIM of K frames, two launches.  pred [K,3,H,W]; gt at + gt_stride floats per frame, mask [H,W] at + mask_stride floats
 * per frame (0 = one target / one mask for all frames); mask NULL = no mask, otherwise pred (after the clamp) and gt are both
 * multiplied by it.  ws: sg_image_metrics_ws_bytes(K, width, height) bytes; metrics [K][SG_METRICS_FLOATS].
 * Refused (status 1, before any HIP call): K outside 1..65535, width or height < 1 (or 2^30 pixels and more), unknown flag bits,
 * NULL pred / gt / ws / metrics, a non-zero mask_stride with a NULL mask.  Images smaller than the window are legal. */
int sg_image_metrics_frames(int K, int width, int height, int flags, const float *pred, const float *gt, size_t gt_stride,
                            const float *mask, size_t mask_stride, void *ws, float *metrics, void *stream);

#ifdef __cplusplus
}
#endif
#endif
