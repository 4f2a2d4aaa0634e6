/*
 * sings_order.h -- the work order of a K-camera launch of the plain raster path.
 *
 * A work order is a permutation `order` of [0, P): the (tile, Gaussian) pairs of a frame are expanded and counted by a kernel whose
 * lane i works on Gaussian order[i], behind a per-Gaussian kernel that stays in id order.  Everything a caller or another kernel
 * sees is what the unordered call leaves, bit for bit -- the geometry records, radii, the record slots, the sorted lists, the
 * image, the gradients: a pair's rank in its tile's row is an arbitrary slot (the composite sorts the row by depth and id).  ANY
 * permutation is correct; a stale one only costs speed.
 *
 * What a spatially coherent order buys (Gaussians that are neighbours in space next to each other): the 256 Gaussians of a
 * workgroup cover a small window of tiles, so the workgroup counts its pairs per tile in LDS and issues one global returning atomic
 * per (workgroup, tile) instead of one per pair.  A workgroup whose window has more than SG_ORDER_WINDOW_TILES tiles counts per
 * pair, as the unordered kernel does.
 *
 * The order takes effect on frames of many tiles that are binned directly (SG_FLAG_SHORT_LISTS on an image of more than 4096
 * tile counters); on every other frame the ordered call is the unordered one.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises.  These functions are not part of SG_ABI_VERSION's table: a library either
 * exports them all or predates this header.
 */
#ifndef SINGS_ORDER_H
#define SINGS_ORDER_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ORDER_WINDOW_TILES 1536      /* largest tile window (bounding box of a workgroup's tile rectangles) counted in LDS */
#define SG_ORDER_BLOCK 256              /* Gaussians per workgroup: positions [256 b, 256 b + 256) of the order */
#define SG_ORDER_CODE_BITS 10           /* bits per axis of sg_work_order_codes */
#define SG_ORDER_WS_BYTES 32            /* workspace of sg_work_order_codes */

/* sg_rasterize_forward_frames with a work order.  order: P entries (device), or NULL with order_len 0 = the unordered call.
 * Refused: order_len != P.  An entry >= P is never dereferenced (its lane idles; the frame is then wrong, not the process). */
int sg_rasterize_forward_frames_ordered(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const float *means3D,
                                        const float *shs, const float *colors_precomp, const float *opacities,
                                        const float *scales, const float *rotations, const float *cov3D_precomp, void *geom_ws,
                                        void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                                        int64_t *num_rendered_host, const uint32_t *order, int order_len, void *stream);

/* 30-bit 3-D Morton codes of means3D [P,3] over their bounding box, SG_ORDER_CODE_BITS per axis (x in bit 0, y in bit 1, z in
 * bit 2 of every triple), into codes [P].  A pure function of the positions, in fp32:
 *     lo, hi = min, max per axis (NaNs ignored);  q = (x - lo) * (1023 / max(hi - lo, 1e-12)),  cell = min((uint32) q, 1023)
 * (a NaN coordinate: cell 0).  A stable sort of (code, index) is the order; two launches, ws: SG_ORDER_WS_BYTES bytes. */
int sg_work_order_codes(int P, const float *means3D, void *ws, uint32_t *codes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
