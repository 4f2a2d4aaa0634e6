/*
 * sings_silhouette.h -- the soft silhouette of a posed triangle mesh in libsings_hip.so, with its backward, and the update launch of
 * the pose refinement around it (the reference's `--opt` step: preprocess/utils/ooptimize_smpl.py:260-364, which goes through
 * pytorch3d's MeshRasterizer + SoftSilhouetteShader).  The definition is `silhouette_host` of sings_amd/pose_refine.py.
 *
 *     sg_sil_layout        the pieces of the workspace, in bytes (host only)
 *     sg_sil_forward       project, file the faces into 16 x 16 tiles in ascending face index, blend: alpha [K,H,W]
 *     sg_sil_backward      dL/dalpha -> dL/dverts_cam, one partial per (tile, face) pair, every sum in a fixed order
 *     sg_sil_pose_update   gate + Adam on [K,72] pose rows, the step counter in device memory
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises, nothing allocates.  These functions are not part of SG_ABI_VERSION's table: a
 * library either exports them all or predates this header.
 *
 * No floating-point atomics, no waiting between workgroups: two calls on the same inputs give the same bits.  With
 * x_f = signed_f / sigma and q_f = 1 - prob_f, alpha = 1 - Q, Q = prod_f q_f, so d alpha / d x_f = -Q prob_f: the backward needs a
 * pixel's Q (saved by the forward) and the pair's own prob_f, no product over the other faces and no division.
 */
#ifndef SINGS_SILHOUETTE_H
#define SINGS_SILHOUETTE_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_SIL_TILE 16              /* a tile is 16 x 16 pixels: one workgroup of 256, one pixel per lane */
#define SG_SIL_CHUNK 256            /* faces of a tile list staged through LDS at a time; a list may have any length */
#define SG_SIL_SORT_LDS 1024        /* a list up to here is brought into ascending order in LDS, a longer one in place */
#define SG_SIL_MAX_FRAMES 64        /* K */
#define SG_SIL_GUARD_WORDS 64       /* 4-byte words behind the pair list and behind the partials that no kernel writes */
#define SG_SIL_INFO_WORDS 4         /* info[0]: overflow (pairs > capacity) and info[1]: pairs of all frames, of the last launch; info[2]:
                                     * overflow and info[3]: most pairs of any launch since the caller zeroed them; then pairs per frame [K] */
#define SG_SIL_POSE 72              /* entries of a pose row */
/* sg_sil_layout: byte OFFSETS of the pieces, then the total */
#define SG_SIL_L_INFO 0
#define SG_SIL_L_REC 1              /* float [K,F,8]: u0 v0 u1 v1 u2 v2 - - in pixels */
#define SG_SIL_L_RECT 2             /* int32 [K,F,4]: the tiles x0 y0 x1 y1 a face's grown bounding box meets (x1 < x0: none) */
#define SG_SIL_L_TILE_COUNT 3       /* uint32 [K,T]: list lengths */
#define SG_SIL_L_TILE_START 4       /* uint32 [K,T] + block sums: the exclusive scan of the lengths */
#define SG_SIL_L_CURSOR 5           /* uint32 [K,T] */
#define SG_SIL_L_Q 6                /* float [K,H,W]: 1 - alpha before rounding, what the backward multiplies by */
#define SG_SIL_L_FACE_GRAD 7        /* float [K,F,6] */
#define SG_SIL_L_LIST 8             /* uint32 [capacity]: face indices, tile after tile; then SG_SIL_GUARD_WORDS */
#define SG_SIL_L_PARTIAL 9          /* float [capacity,6]; then SG_SIL_GUARD_WORDS */
#define SG_SIL_L_BYTES 10
#define SG_SIL_LAYOUT_WORDS 11

/* Host only, no HIP call.  Refused (status 1): K outside 1..SG_SIL_MAX_FRAMES, V, F, H, W < 1, capacity < 1, or any piece whose
 * element offsets (K H W, 8 K F, 6 capacity + guard, K tiles + 1024) do not fit int32. */
int sg_sil_layout(int K, int V, int F, int H, int W, size_t capacity, size_t *layout);

/* verts [K,V,3] camera space, faces [F,3] int32 (a face with a corner outside [0, V) is skipped, never dereferenced) -> alpha [K,H,W].
 * counts [K] int32 or NULL: the largest number of blended faces of a pixel (the counting variant of the composite, asked for only
 * when wanted).  ws: sg_sil_layout's bytes, 16-byte aligned; a backward on the same ws reads what this call left there.  A (tile,
 * face) pair beyond `capacity` is dropped and info[0] set: never a write out of bounds; alpha is then not the silhouette. */
int sg_sil_forward(int K, int V, int F, int H, int W, float fx, float fy, float cx, float cy, float sigma, size_t capacity,
                   const float *verts, const int32_t *faces, void *ws, float *alpha, int32_t *counts, void *stream);

/* After sg_sil_forward with the same arguments on the same ws.  dalpha [K,H,W]; row_ptr [V+1] / corner: the CSR vertex -> 3 f + c of
 * the face corners (built once per topology, rows in ascending 3 f + c) -> dverts [K,V,3], every entry written; a vertex that is not
 * finite or not in front, and the corners of skipped faces, get exact zeros. */
int sg_sil_backward(int K, int V, int F, int H, int W, float fx, float fy, float cx, float cy, float sigma, size_t capacity,
                    const float *verts, const int32_t *faces, void *ws, const float *dalpha, const int32_t *row_ptr,
                    const int32_t *corner, float *dverts, void *stream);

/* ONE launch, one workgroup: it = step[0] + 1; for the K rows of pose / grad / m / v [K,72]:
 *     g = grad * grad_mask * ((pose < hi) & (pose > lo));  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g
 *     pose -= (lr / (1 - b1^it)) m / (sqrt(v) / sqrt(1 - b2^it) + 1e-8)          (b1 = 0.9, b2 = 0.999, as torch.optim.Adam)
 * then step[0] = it.  terms [K,2] with table [max_iterations,K,2], or both NULL: table[it - 1] = terms when it <= max_iterations.
 * Refused: K outside 1..SG_SIL_MAX_FRAMES, NULL pointers, one of terms / table without the other. */
int sg_sil_pose_update(int K, float lr, float *pose, const float *grad, float *m, float *v, const float *grad_mask, const float *lo,
                       const float *hi, int32_t *step, const float *terms, float *table, int max_iterations, void *stream);

#ifdef __cplusplus
}
#endif
#endif
