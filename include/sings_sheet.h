/*
 * sings_sheet.h -- planar fp32 frames tiled, quantised and interleaved into finished 8-bit HWC sheets, in ONE launch.
 *
 * Every picture a training run leaves behind is the same operation: K frames [3,H,W] fp32 -> a grid of tiles with a border
 * (torchvision's published make_grid layout) -> bytes.  The reference does it with make_grid / save_image / numpy on the host
 * (gs_trainer.py:443-449 the training picture, :588-591 the validation grids, :838 the turntable frames, :842 the progress sheet).
 *
 * Sheets and tiles.  S sheets of T tiles; a tile is one [3,H,W] planar fp32 frame.
 *     b == NULL   tile t of sheet s is frame s*T + t of `a`
 *     b != NULL   T is even; tile t is frame s*T/2 + t/2 of `a` for even t, of `b` for odd t (the `gt | pred` pair, repeated)
 * Geometry.
 *     xmaps = min(nrow, T), ymaps = ceil(T / xmaps); Hs = ymaps*(H+padding) + padding, Ws = xmaps*(W+padding) + padding
 *     tile t starts at row (t / xmaps)*(H+padding) + padding and column (t % xmaps)*(W+padding) + padding
 *     every other pixel is pad_value, the cells of an incomplete last row included; padding 0 is plain concatenation
 * Quantisation, of the tiles' values and of pad_value alike (fp32, every operation rounded on its own); NaN gives 0.
 *     SG_SHEET_TRUNC   (uint8)(clamp(x, 0, 1) * 255)               sg_frames_to_u8, gs_trainer.py:446-447 / :717
 *     SG_SHEET_ROUND   (uint8)clamp(x * 255 + 0.5, 0, 255)         torchvision's save_image
 * mask (optional, [frames of a, H, W] fp32): a tile is multiplied by the mask row of its frame index within its source tensor
 * before it is quantised (gs_trainer.py:580-582).  bgr swaps the first and the third byte.  out: [S, Hs, Ws, 3] uint8.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises.  This function is not part of SG_ABI_VERSION's table: a library either
 * exports it or predates this header.
 */
#ifndef SINGS_SHEET_H
#define SINGS_SHEET_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_SHEET_TRUNC 0
#define SG_SHEET_ROUND 1
#define SG_SHEET_MAX_SHEETS 65535       /* most sheets per launch (the grid's second dimension) */
#define SG_SHEET_BLOCK 256              /* threads per workgroup; a thread writes 4 consecutive pixels of a sheet */

/* Refused (status 1, before any HIP call): a NULL a or out; S, T, width, height or nrow below 1; padding < 0; a quant that is
 * neither SG_SHEET_TRUNC nor SG_SHEET_ROUND; an odd T with b; S > SG_SHEET_MAX_SHEETS; a sheet of 2^31 pixels or more. */
int sg_image_sheets(int S, int T, int width, int height, int nrow, int padding, float pad_value, int quant, int bgr,
                    const float *a, const float *b, const float *mask, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
