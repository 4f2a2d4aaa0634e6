/*
 * sings_density.h -- the densification statistics of a training step in ONE launch, behind a gate in device memory.
 *
 * The reference accumulates xyz_gradient_accum, denom and max_radii2D only inside densify_or_prune_hybrid (gs_trainer.py:486-492,
 * sings_hybrid.py:1013-1015): on the iteration that takes a density decision, from that iteration's frame.  A captured step cannot
 * contain "sometimes": it contains this launch always, and the launch reads one word of device memory first.  The host sets that
 * word, stream-ordered, before a replay (sings_amd.train_loop.AvatarTrainer under a HybridDensitySchedule); with the word at 0 every
 * thread returns before it has touched any of the three arrays.
 *
 * The rule, per Gaussian i, over the K frames of the step in ascending frame order:
 *     a frame k with radii[k][i] > 0 (the Gaussian was visible in it):
 *         norm_k = sqrtf(fmaf(gx, gx, gy * gy))      gx, gy = grad[k][i][0], grad[k][i][1]; grad[k][i][2] is never read
 *         denom[i] += 1;   max_radii[i] = max(max_radii[i], (float) radii[k][i])
 *     a frame with radii <= 0 is SKIPPED, not multiplied by zero: its gradient is not read, so a non-finite gradient of an invisible
 *         Gaussian leaves the row as it was (the reference's boolean indexing behaves this way)
 *     accum[i] += norm of the first visible frame + the next + ...   (the frames' sum first, one addition into accum)
 *     a Gaussian that no frame saw is not written at all
 * One thread per Gaussian and a fixed order of the additions: two calls on the same inputs give the same bits.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises.  This function is not part of SG_ABI_VERSION's table: a library either
 * exports it or predates this header.
 */
#ifndef SINGS_DENSITY_H
#define SINGS_DENSITY_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_DENSITY_MAX_K 16             /* most frames per step (SG_MAX_FRAMES) */
#define SG_DENSITY_BLOCK 256            /* threads (Gaussians) per workgroup */

/* grad [K][N][3] fp32 (the screen-space gradient of the step: viewspace_points.grad), radii [K][N] int32; accum, denom,
 * max_radii [N] fp32, updated in place.  gate: one int32 in device memory, or NULL ("always accumulate"); *gate == 0 makes the
 * launch a no-op.  N == 0 returns 0 without a launch.
 * Refused (status 1, before any HIP call): N < 0, K outside 1..SG_DENSITY_MAX_K, with N > 0 a NULL grad / radii / accum / denom /
 * max_radii. */
int sg_density_stats(int K, int N, const float *grad, const int32_t *radii, const int32_t *gate, float *accum, float *denom,
                     float *max_radii, void *stream);

#ifdef __cplusplus
}
#endif
#endif
