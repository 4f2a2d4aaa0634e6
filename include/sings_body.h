/*
 * sings_body.h -- the body model of libsings_hip.so: what turns SMPL-shaped arrays and a betas vector into the mesh a run starts from
 * (the reference's SMPL / SMPLH layer: smpl_layer.py:296-353 `subdivide_meshes`, sings_hybrid.py:578-596 `get_canonical_verts`).
 *
 *     sg_body_renorm        J_regressor of a subdivided template: rows of the averaged J^T, each divided by its sum
 *     sg_body_joint_basis   the regressor folded through [v_template | shapedirs]: joints_rest(betas) = J0 + JS . betas
 *     sg_body_shaped        blend shapes and pose correctives of K rows in one march over the vertices
 *     sg_body_smooth        the mutable diffusion Laplacian filter with volume constraint, every iteration on the device
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises, nothing allocates.  These functions are not part of SG_ABI_VERSION's table: a
 * library either exports them all or predates this header.
 *
 * Every sum here is taken in a fixed order in fp64 (or, for the vertex normals, in 64-bit fixed point with integer atomics): two calls
 * on the same inputs give the same bits.
 */
#ifndef SINGS_BODY_H
#define SINGS_BODY_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_BODY_MAX_JOINTS 64       /* J: the joint transforms run one wave per frame, lane = joint */
#define SG_BODY_MAX_BETAS 32        /* B: a thread of the joint basis keeps B + 1 fp64 sums in registers */
#define SG_BODY_MAX_VERTS 4194304   /* V: 2^22 */
#define SG_BODY_MAX_ROWS 1024       /* K: rows of betas / pose features in one sg_body_shaped call */
#define SG_BODY_MAX_ITERATIONS 64   /* iterations of one sg_body_smooth call */
#define SG_BODY_INFO_INTS 4         /* info[0]: flag bits below; the rest reserved (zero) */
#define SG_BODY_ISOLATED 1          /* a vertex without a neighbour in the CSR */
#define SG_BODY_NOT_FINITE 2        /* a non-finite input vertex */
#define SG_BODY_BAD_SLOPE 4         /* vol(x + eps n) - vol(x) is zero or not finite */
#define SG_BODY_BAD_FACE 8          /* a face corner outside [0, V): the face is skipped, never dereferenced */

/* J_regressor [J,V] from Jt [V,J] (the endpoint means of J_regressor^T after a subdivision): row j divided by its sum,
 * smpl_layer.py:349-350.  The sum of a row is fp64 in a fixed order, rounded to fp32 once; the division is fp32.
 * Refused (status 1, before any HIP call): J outside 1..SG_BODY_MAX_JOINTS, V outside 1..SG_BODY_MAX_VERTS, NULL pointers. */
int sg_body_renorm(int J, int V, const float *Jt, float *J_regressor, void *stream);

/* J0 [J,3] = J_regressor . v_template and JS [J,3,B] = J_regressor . shapedirs (shapedirs [V,3,B]) in ONE launch: a workgroup per
 * (joint, axis), fp64 sums over V in a fixed order, rounded to fp32 once.
 * Refused: J, V as above, B outside 1..SG_BODY_MAX_BETAS, NULL pointers. */
int sg_body_joint_basis(int V, int J, int B, const float *v_template, const float *shapedirs, const float *J_regressor, float *J0,
                        float *JS, void *stream);

/* K rows in ONE launch over the vertices: betas [K,B]; pose_feature [K,P] with posedirs [P, 3V], or both NULL (P = 0: zero pose
 * offsets).  Outputs [K,V,3] each, any may be NULL:
 *     shape_offsets = shapedirs . betas        v_shaped = v_template + shape_offsets
 *     pose_offsets  = pose_feature . posedirs  v_posed  = v_shaped + pose_offsets
 * Sums in fp64 in index order; every output is rounded to fp32 once from the fp64 value.
 * Refused: V as above, B outside 1..SG_BODY_MAX_BETAS, K outside 1..SG_BODY_MAX_ROWS, P < 0, P > 0 without posedirs / pose_feature,
 * NULL inputs. */
int sg_body_shaped(int V, int B, int K, int P, const float *v_template, const float *shapedirs, const float *betas,
                   const float *posedirs, const float *pose_feature, float *v_shaped, float *shape_offsets, float *pose_offsets,
                   float *v_posed, void *stream);

/* Bytes of sg_body_smooth's workspace (0: V or F outside what it covers). */
size_t sg_body_smooth_ws_bytes(int V, int F);

/* The filter, `iterations` times, without a host read in between.  x0 [V,3]; faces [F,3]; row_ptr [V+1] / col: the CSR of the unique
 * edges, both directions (sg_mesh_terms_build without labels).  With L the uniform umbrella ((L x)_v: the mean of v's neighbours),
 * n_v the unit vector of the sum of the unit normals of v's faces (of x0, not updated), eps = 0.01 sqrt(max face area of x0),
 * vol(x) = sum_f x_a . (x_b x x_c) / 6 and vol0 = vol(x0), iteration i is
 *     d = |n . (x - L x)|;  a = 1 / max(1e-12, d);  lambda_v = max(0.2 lamb, min(1, lamb a_v / mean(a)))
 *     x += lambda (L x - x)
 *     i == 0:  slope = eps / (vol(x + eps n) - vol(x))
 *     x += n slope (vol0 - vol(x))
 * x is held in fp64 in the workspace across the iterations and all arithmetic is fp64; x_out [V,3] is its fp32 rounding, written by
 * the last launch and ONLY when info[0] is zero.  x_out may not alias x0.  info [SG_BODY_INFO_INTS]: the caller reads it once.
 * Refused: V outside 1..SG_BODY_MAX_VERTS, F outside 1..715827882, iterations outside 0..SG_BODY_MAX_ITERATIONS, a lamb that is not
 * finite, NULL pointers. */
int sg_body_smooth(int V, int F, int iterations, float lamb, const float *x0, const int32_t *faces, const int32_t *row_ptr,
                   const int32_t *col, void *ws, float *x_out, int32_t *info, void *stream);

#ifdef __cplusplus
}
#endif
#endif
