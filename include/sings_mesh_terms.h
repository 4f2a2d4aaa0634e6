/*
 * sings_mesh_terms.h -- the mesh terms of the training step of libsings_hip.so: the three Laplacian regularisers that every shipped
 * configuration optimises (sings/rec/trainer/gs_trainer.py:366-399 with losses/loss_items.py:93-192), fused, and their graph built on
 * the device.
 *
 *     L = D^-1 A - I  over the unique edges whose two endpoints share a label (a vertex without such an edge: y_i = -x_i)
 *     term(x, w) = sum_i  w[label_i] / (count[label_i] * 3)  |(L x)_i|^2
 *     terms[0] = term_w[0] term(xyz_canon + mean(scales, -1) n / 2, w_pos)      region_mesh_lap
 *     terms[1] = term_w[1] term(colour, w_col)                                  region_mesh_lap_color
 *     terms[2] = term_w[2] term(xyz_canon, w_hand)                              the hand term
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises, nothing allocates.  These functions are not part of SG_ABI_VERSION's table: a
 * library either exports them all or predates this header.
 */
#ifndef SINGS_MESH_TERMS_H
#define SINGS_MESH_TERMS_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_MESH_TERMS_INFO_INTS 2   /* info[0]: flag bits below; info[1]: row_ptr[V], the number of CSR entries */
#define SG_MESH_TERMS_BAD_LABEL 1   /* a vertex label outside [0, L) */
#define SG_MESH_TERMS_BAD_EDGE 2    /* an edge row that is not 0 <= a < b < V */

/* The CSR of the same-label edges and what hangs on it, five launches, no host read.  edges [E,2]: unique rows a < b in lexicographic
 * order; vertex_label [V]; w_pos / w_col / w_hand [L]: per-label weights of the three terms.
 *   row_ptr [V+1], col [2E] (the upper bound; row_ptr[V] entries are written): both directions, columns ascending within a row
 *   deg_inv [V]: 1 / degree (0 for an isolated vertex);  count [L]: vertices per label
 *   vscale [V,3]: w[label] / (count[label] * 3) for position, colour, hand (fp32: the product, then the division)
 *   deg_ws [V]: scratch;  info [SG_MESH_TERMS_INFO_INTS]
 * Every output is a pure function of the inputs (integer atomics for counts and slots only; the rows are sorted): two builds give the
 * same bits.  A bad label or a bad edge row sets its flag in info[0] and is skipped, never dereferenced; an edge with a bad label at
 * either end does not count.  vertex_label NULL: every edge counts (the CSR of the whole mesh, as sg_mesh_edge_loss reads it); the
 * weights, count and vscale are then not read or written and L is ignored.
 * Refused (status 1, before any HIP call): V outside 1..2^30, E outside 0..2^30 - 1, L < 1 (with labels), NULL pointers (edges / col
 * may be NULL when E is 0). */
int sg_mesh_terms_build(int V, int E, int L, const int32_t *edges, const int32_t *vertex_label, const float *w_pos, const float *w_col,
                        const float *w_hand, int32_t *row_ptr, int32_t *col, float *deg_inv, int32_t *count, float *vscale,
                        int32_t *deg_ws, int32_t *info, void *stream);

/* The three terms and their gradients: forward, reduction, backward -- three launches (two without a gradient output).
 * xyz_canon, scales, normals [V,3]; colour: V rows of 3 floats, colour_stride floats apart (48 for the DC row of shs [V,16,3]);
 * term_w [3] in DEVICE memory (the step weights: a captured graph replays with the values of the moment);
 * ws: sg_reg_ws_bytes(V) bytes; g_ws [3,V,3] floats; terms [3]: the weighted values (fp64 sums in a fixed order, no atomics).
 * upstream [1] or NULL (= 1) scales the gradients:  d_xyz_canon [V,3] (position + hand), d_scales [V,3] (each column
 * (n_i . g_i) / 6 with g the position term's gradient of the anchor), d_colour [V,3] dense.  Each may be NULL.
 * Refused (status 1, before any HIP call): V outside 1..2^30, colour_stride < 3, NULL inputs / ws / g_ws / terms. */
int sg_mesh_terms(int V, const float *xyz_canon, const float *scales, const float *normals, const float *colour, int colour_stride,
                  const int32_t *row_ptr, const int32_t *col, const float *deg_inv, const float *vscale, const float *term_w, void *ws,
                  float *g_ws, float *terms, const float *upstream, float *d_xyz_canon, float *d_scales, float *d_colour, void *stream);

#ifdef __cplusplus
}
#endif
#endif
