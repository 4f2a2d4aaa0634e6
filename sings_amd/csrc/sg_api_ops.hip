// extern "C" wrappers of the modules whose kernel files carry no entry points (see include/sings_hip.h), in the header's order:
// LBS, joint and pose transforms, rotation conversions, photometric loss, regularisers, tri-plane decode, linear layers.
// Each checks its arguments, calls one sg_launch_* and reports the launch.
#include "sg_host.h"
#include "sg_reduce.h"                 // sg_launch_rows_laplacian

// ---- stand-alone lbs_extra (a9)
extern "C" int sg_lbs_forward(int P, int J, const float *lbs_weights, const float *A, const float *v, float *T_out,
                              float *verts_out, void *stream)
{
    if (P <= 0 || J < 1 || J > 64 || !lbs_weights || !A || !v || !verts_out)
        return sg_set_error("sg_lbs_forward: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_lbs_fwd(P, J, lbs_weights, A, v, T_out, verts_out, (hipStream_t)stream);
    return sg_launched("sg_lbs_forward");
}
extern "C" int sg_lbs_backward(int P, int J, const float *lbs_weights, const float *A, const float *v, const float *dT,
                               const float *dverts, float *ws, float *dv, float *dA, void *stream)
{
    if (P <= 0 || J < 1 || J > 64 || !lbs_weights || !A || !v || !ws || !dA || (!dT && !dverts))
        return sg_set_error("sg_lbs_backward: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_lbs_bwd(P, J, lbs_weights, A, v, dT, dverts, ws, dv, dA, (hipStream_t)stream);
    return sg_launched("sg_lbs_backward");
}

// ---- SMPL kinematic chain (a10)
extern "C" int sg_joint_transforms(int B, int J, const float *pose, const float *joints_rest, const int32_t *parents,
                                   const float *post, float *A_out, void *stream)
{
    if (B <= 0 || J < 1 || J > 64 || !pose || !joints_rest || !parents || !A_out)
        return sg_set_error("sg_joint_transforms: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_joint_transforms(B, J, pose, joints_rest, (const int *)parents, post, nullptr, A_out, nullptr, (hipStream_t)stream);
    return sg_launched("sg_joint_transforms");
}
extern "C" int sg_joint_transforms_backward(int B, int J, const float *pose, const float *joints_rest, const int32_t *parents,
                                            const float *post, const float *dA, float *dpose, float *djoints, void *stream)
{
    if (B <= 0 || J < 1 || J > 64 || !pose || !joints_rest || !parents || !dA || !dpose)
        return sg_set_error("sg_joint_transforms_backward: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_joint_transforms(B, J, pose, joints_rest, (const int *)parents, post, dA, dpose, djoints, (hipStream_t)stream);
    return sg_launched("sg_joint_transforms_backward");
}

// ---- learned per-frame pose tables -> A
static bool sg_pose_shape_ok(int K, int F, int J, int NBu)
{
    return K >= 1 && F >= 1 && J >= 1 && J <= 64 && NBu >= 0 && NBu <= SG_POSE_NB && NBu < J;
}
extern "C" int sg_pose_transforms(int K, int F, int J, int NBu, const int32_t *frame_idx, const float *global_orient,
                                  const float *body_pose, const float *tail_pose, const float *transl, const float *joints_rest,
                                  const int32_t *parents, const float *post, float *A_out, float *aa_out, float *transl_out,
                                  void *stream)
{
    if (!sg_pose_shape_ok(K, F, J, NBu) || !frame_idx || !global_orient || !body_pose || (J - 1 - NBu > 0 && !tail_pose) ||
        !joints_rest || !parents || !A_out || !aa_out || (transl == nullptr) != (transl_out == nullptr))
        return sg_set_error("sg_pose_transforms: bad argument (1 <= J <= 64, 0 <= NBu <= 23, NBu < J; tail_pose for J - 1 - NBu joints; "
                       "transl and transl_out together)", hipSuccess);
    sg_launch_pose_transforms(K, F, J, NBu, (const int *)frame_idx, global_orient, body_pose, tail_pose, transl, joints_rest,
                              (const int *)parents, post, A_out, aa_out, transl_out, (hipStream_t)stream);
    return sg_launched("sg_pose_transforms");
}
extern "C" int sg_pose_transforms_backward(int K, int F, int J, int NBu, const int32_t *frame_idx, const float *global_orient,
                                           const float *body_pose, const float *aa, const float *joints_rest, const int32_t *parents,
                                           const float *post, const float *dA, const float *d_transl_rows, float *d_global_orient,
                                           float *d_body_pose, float *d_transl, void *stream)
{
    if (!sg_pose_shape_ok(K, F, J, NBu) || !frame_idx || !global_orient || !body_pose || !aa || !joints_rest || !parents || !dA ||
        !d_global_orient || !d_body_pose || (d_transl_rows == nullptr) != (d_transl == nullptr))
        return sg_set_error("sg_pose_transforms_backward: bad argument (1 <= J <= 64, 0 <= NBu <= 23, NBu < J; d_transl_rows and d_transl "
                       "together)", hipSuccess);
    sg_launch_pose_transforms_bwd(K, F, J, NBu, (const int *)frame_idx, global_orient, body_pose, aa, joints_rest, (const int *)parents,
                                  post, dA, d_transl_rows, d_global_orient, d_body_pose, d_transl, (hipStream_t)stream);
    return sg_launched("sg_pose_transforms_backward");
}

// ---- stand-alone matrix_to_quaternion (a11)
extern "C" int sg_matrix_to_quaternion(int N, const float *matrices, float *quaternions, void *stream)
{
    if (N <= 0 || !matrices || !quaternions) return sg_set_error("sg_matrix_to_quaternion: bad argument", hipSuccess);
    sg_launch_m2q(N, matrices, nullptr, quaternions, (hipStream_t)stream);
    return sg_launched("sg_matrix_to_quaternion");
}
extern "C" int sg_matrix_to_quaternion_backward(int N, const float *matrices, const float *dq, float *dmatrices, void *stream)
{
    if (N <= 0 || !matrices || !dq || !dmatrices) return sg_set_error("sg_matrix_to_quaternion_backward: bad argument", hipSuccess);
    sg_launch_m2q(N, matrices, dq, dmatrices, (hipStream_t)stream);
    return sg_launched("sg_matrix_to_quaternion_backward");
}

// ---- the other rotation conversions (a11)
extern "C" int sg_rotation_convert(int op, int N, const float *in, float *out, void *stream)
{
    if (N <= 0 || !in || !out) return sg_set_error("sg_rotation_convert: bad argument", hipSuccess);
    if (sg_launch_rot_map(op, N, in, nullptr, out, (hipStream_t)stream)) return sg_set_error("sg_rotation_convert: unknown op", hipSuccess);
    return sg_launched("sg_rotation_convert");
}
extern "C" int sg_rotation_convert_backward(int op, int N, const float *in, const float *d_out, float *d_in, void *stream)
{
    if (N <= 0 || !in || !d_out || !d_in) return sg_set_error("sg_rotation_convert_backward: bad argument", hipSuccess);
    if (sg_launch_rot_map(op, N, in, d_out, d_in, (hipStream_t)stream)) return sg_set_error("sg_rotation_convert_backward: unknown op", hipSuccess);
    return sg_launched("sg_rotation_convert_backward");
}
extern "C" int sg_quaternion_multiply(int N, const float *a, const float *b, float *out, void *stream)
{
    if (N <= 0 || !a || !b || !out) return sg_set_error("sg_quaternion_multiply: bad argument", hipSuccess);
    sg_launch_qmul(N, a, b, nullptr, out, nullptr, (hipStream_t)stream);
    return sg_launched("sg_quaternion_multiply");
}
extern "C" int sg_quaternion_multiply_backward(int N, const float *a, const float *b, const float *d_out, float *da, float *db,
                                               void *stream)
{
    if (N <= 0 || !a || !b || !d_out || !da || !db) return sg_set_error("sg_quaternion_multiply_backward: bad argument", hipSuccess);
    sg_launch_qmul(N, a, b, d_out, da, db, (hipStream_t)stream);
    return sg_launched("sg_quaternion_multiply_backward");
}

// ---- photometric loss
extern "C" int sg_photo_loss_frames(int K, int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                                    size_t gt_stride, const float *mask, size_t mask_stride, const float *bg, void *ws,
                                    float *pred_out, float *gt_out, float *losses, const float *upstream, float *dL_draw, void *stream)
{
    if (width <= 0 || height <= 0 || K < 1 || K > SG_MAX_FRAMES) return sg_set_error("sg_photo_loss: bad image size / K not in 1..16", hipSuccess);
    if (!raw || !gt_rgb || !mask || !bg || !ws || (!losses && !dL_draw))
        return sg_set_error("sg_photo_loss: null pointer", hipSuccess);
    sg_launch_photo_loss(K, width, height, l1_w, ssim_w, raw, gt_rgb, mask, bg, ws, pred_out, gt_out, losses, upstream,
                         dL_draw, gt_stride, mask_stride, (hipStream_t)stream);
    return sg_launched("sg_photo_loss");
}
extern "C" int sg_photo_loss_backward_frames(int K, int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                                             size_t gt_stride, const float *mask, size_t mask_stride, const float *bg, const void *ws,
                                             const float *upstream, int upstream_stride, float *dL_draw, void *stream)
{
    if (K < 1 || K > SG_MAX_FRAMES || width <= 0 || height <= 0 || !raw || !gt_rgb || !mask || !bg || !ws || !dL_draw)
        return sg_set_error("sg_photo_loss_backward_frames: bad arguments (K in 1..16, no null pointers)", hipSuccess);
    if (upstream_stride != 0 && upstream_stride != 2) return sg_set_error("sg_photo_loss_backward_frames: upstream_stride must be 0 or 2", hipSuccess);
    sg_launch_photo_loss_bwd(K, width, height, l1_w, ssim_w, raw, gt_rgb, mask, bg, ws, upstream, dL_draw, gt_stride, mask_stride,
                             (hipStream_t)stream, upstream ? upstream_stride : 0);
    return sg_launched("sg_photo_loss_backward_frames");
}

extern "C" size_t sg_photo_loss_ws_bytes(int width, int height)
{
    return width > 0 && height > 0 ? sg_photo_loss_ws_bytes_impl(width, height) : 0;
}

extern "C" int sg_photo_loss(int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                             const float *mask, const float *bg, void *ws, float *pred_out, float *gt_out,
                             float *losses, const float *upstream, float *dL_draw, void *stream)
{
    return sg_photo_loss_frames(1, width, height, l1_w, ssim_w, raw, gt_rgb, 0, mask, 0, bg, ws, pred_out, gt_out, losses, upstream,
                                dL_draw, stream);
}

extern "C" int sg_photo_loss_backward(int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                                      const float *mask, const float *bg, const void *ws, const float *upstream,
                                      float *dL_draw, void *stream)
{
    if (width <= 0 || height <= 0) return sg_set_error("sg_photo_loss_backward: bad image size", hipSuccess);
    if (!raw || !gt_rgb || !mask || !bg || !ws || !dL_draw) return sg_set_error("sg_photo_loss_backward: null pointer", hipSuccess);
    sg_launch_photo_loss_bwd(1, width, height, l1_w, ssim_w, raw, gt_rgb, mask, bg, ws, upstream, dL_draw, 0, 0, (hipStream_t)stream);
    return sg_launched("sg_photo_loss_backward");
}

// ---- regularisers (f1)
extern "C" size_t sg_reg_ws_bytes(int rows) { return sg_reg_ws_bytes_impl(rows > 0 ? rows : 1); }
extern "C" size_t sg_knn_ws_bytes(int N) { return sg_knn_ws_bytes_impl(N > 0 ? N : 1); }

extern "C" int sg_region_laplacian(int V, int C, const float *x, const int *row_ptr, const int *col,
                                   const float *deg_inv, const float *vscale, void *ws, float *g_ws, float *loss,
                                   const float *upstream, float *dL_dx, void *stream)
{
    if (V <= 0 || C <= 0 || !x || !row_ptr || !col || !deg_inv || !vscale || !ws || !g_ws || (!loss && !dL_dx))
        return sg_set_error("sg_region_laplacian: bad argument", hipSuccess);
    sg_launch_region_laplacian(V, C, x, row_ptr, col, deg_inv, vscale, ws, g_ws, loss, upstream, dL_dx, (hipStream_t)stream);
    return sg_launched("sg_region_laplacian");
}

extern "C" int sg_rows_laplacian(int R, int V, int C, const float *x, const int *row_ptr, const int *col, const float *val,
                                 const float *rscale, const int *t_row_ptr, const int *t_row, const float *t_val, void *ws,
                                 float *g_ws, float *loss, const float *upstream, float *dL_dx, void *stream)
{
    if (R <= 0 || V <= 0 || C <= 0 || !x || !row_ptr || !col || !val || !rscale || !ws || !g_ws || (!loss && !dL_dx) ||
        (dL_dx && (!t_row_ptr || !t_row || !t_val)))
        return sg_set_error("sg_rows_laplacian: bad argument", hipSuccess);
    sg_launch_rows_laplacian(R, V, C, x, row_ptr, col, val, rscale, t_row_ptr, t_row, t_val, ws, g_ws, loss, upstream, dL_dx,
                             (hipStream_t)stream);
    return sg_launched("sg_rows_laplacian");
}

extern "C" int sg_mesh_edge_loss(int V, int E, const float *x, const int *row_ptr, const int *col, void *ws,
                                 float *loss, const float *upstream, float *dL_dx, void *stream)
{
    if (V <= 0 || E <= 0 || !x || !row_ptr || !col || !ws || (!loss && !dL_dx))
        return sg_set_error("sg_mesh_edge_loss: bad argument", hipSuccess);
    sg_launch_mesh_edge(V, E, x, row_ptr, col, ws, loss, upstream, dL_dx, (hipStream_t)stream);
    return sg_launched("sg_mesh_edge_loss");
}

extern "C" int sg_l2norm_reg(int N, const float *xyz_offsets, const float *scales, const float *opacity,
                             const float *lambdas6, void *ws, float *loss, const float *upstream, float *d_offsets,
                             float *d_scales, float *d_opacity, void *stream)
{
    if (N <= 0 || !lambdas6 || !ws || (!xyz_offsets && !scales && !opacity))
        return sg_set_error("sg_l2norm_reg: bad argument", hipSuccess);
    sg_launch_l2norm(N, xyz_offsets, scales, opacity, lambdas6, ws, loss, upstream, d_offsets, d_scales, d_opacity,
                     (hipStream_t)stream);
    return sg_launched("sg_l2norm_reg");
}

extern "C" int sg_gaussian_edge_loss(int N, int K, const float *xyz, const float *scales, void *ws,
                                     float *mean_edge_out, float *loss, const float *upstream, float *d_scales,
                                     void *stream)
{
    if (N < K || !xyz || !ws) return sg_set_error("sg_gaussian_edge_loss: bad argument (need N >= K)", hipSuccess);
    if (sg_launch_knn_edge(N, K, xyz, scales, ws, mean_edge_out, loss, upstream, d_scales, (hipStream_t)stream))
        return sg_set_error("sg_gaussian_edge_loss: K must be 5, 9 or 17", hipSuccess);
    return sg_launched("sg_gaussian_edge_loss");
}

extern "C" int sg_gaussian_edge_prepare(int N, const float *xyz, void *ws, void *stream)
{
    if (N < 1 || !xyz || !ws) return sg_set_error("sg_gaussian_edge_prepare: bad argument", hipSuccess);
    sg_launch_knn_prepare(N, xyz, ws, (hipStream_t)stream);
    return sg_launched("sg_gaussian_edge_prepare");
}

extern "C" int sg_gaussian_edge_finish(int N, int K, const float *scales, void *ws, float *mean_edge_out, float *loss,
                                       const float *upstream, float *d_scales, void *stream)
{
    if (N < K || !ws) return sg_set_error("sg_gaussian_edge_finish: bad argument (need N >= K)", hipSuccess);
    if (sg_launch_knn_finish(N, K, scales, ws, mean_edge_out, loss, upstream, d_scales, (hipStream_t)stream))
        return sg_set_error("sg_gaussian_edge_finish: K must be 5, 9 or 17", hipSuccess);
    return sg_launched("sg_gaussian_edge_finish");
}

// ---- attribute decode (f3)
extern "C" size_t sg_triplane_ws_bytes(const SgTriplane *tp) { return sg_tp_check(tp) ? 0 : sg_triplane_ws_bytes_impl(tp); }
extern "C" size_t sg_triplane_bwd_ws_bytes(const SgTriplane *tp, int N)
{
    return sg_tp_check(tp) || N <= 0 ? 0 : sg_triplane_bwd_ws_bytes_impl(tp, N);
}
extern "C" int sg_triplane_forward(const SgTriplane *tp, int N, const float *xyz, void *ws, float *feats, void *stream)
{
    if (sg_tp_check(tp)) return sg_set_error("sg_triplane_forward: bad plane description (feat must be 32, 1..4 scales)", hipSuccess);
    if (N <= 0 || !xyz || !ws || !feats) return sg_set_error("sg_triplane_forward: bad argument", hipSuccess);
    sg_launch_triplane_fwd(tp, N, xyz, ws, feats, (hipStream_t)stream);
    return sg_launched("sg_triplane_forward");
}
extern "C" int sg_triplane_backward(const SgTriplane *tp, int N, const float *xyz, void *ws, const float *dfeats,
                                    float *const dplanes[4][3], float *dxyz, void *stream)
{
    if (sg_tp_check(tp)) return sg_set_error("sg_triplane_backward: bad plane description", hipSuccess);
    if (N <= 0 || !xyz || !ws || !dfeats || !dplanes) return sg_set_error("sg_triplane_backward: bad argument", hipSuccess);
    if (sg_launch_triplane_bwd(tp, N, xyz, ws, dfeats, dplanes, dxyz, (hipStream_t)stream))
        return sg_set_error("sg_triplane_backward: memset", hipGetLastError());
    return sg_launched("sg_triplane_backward");
}
extern "C" int sg_triplane_backward_prepare(const SgTriplane *tp, int N, const float *xyz, void *ws, void *stream)
{
    if (sg_tp_check(tp)) return sg_set_error("sg_triplane_backward_prepare: bad plane description", hipSuccess);
    if (N <= 0 || !xyz || !ws) return sg_set_error("sg_triplane_backward_prepare: bad argument", hipSuccess);
    sg_launch_triplane_bwd_prepare(tp, N, xyz, ws, (hipStream_t)stream);
    return sg_launched("sg_triplane_backward_prepare");
}
extern "C" int sg_triplane_backward_prepared(const SgTriplane *tp, int N, const float *xyz, void *ws, const float *dfeats,
                                             float *const dplanes[4][3], float *dxyz, void *stream)
{
    if (sg_tp_check(tp)) return sg_set_error("sg_triplane_backward_prepared: bad plane description", hipSuccess);
    if (N <= 0 || !xyz || !ws || !dfeats || !dplanes) return sg_set_error("sg_triplane_backward_prepared: bad argument", hipSuccess);
    sg_launch_triplane_bwd_run(tp, N, xyz, ws, dfeats, dplanes, dxyz, (hipStream_t)stream);
    return sg_launched("sg_triplane_backward_prepared");
}
extern "C" size_t sg_bias_act_ws_bytes(int N, int C) { return sg_bias_act_ws_bytes_impl(N > 0 ? N : 1, C > 0 ? C : 1); }
extern "C" int sg_bias_act_forward(int N, int C, int act, const float *y, const float *bias, const float *row_offset,
                                   float *z_out, float *h_out, void *stream)
{
    if (N <= 0 || C <= 0 || act < 0 || act > 3 || !y || !h_out) return sg_set_error("sg_bias_act_forward: bad argument", hipSuccess);
    sg_launch_bias_act_fwd(N, C, act, y, bias, row_offset, z_out, h_out, (hipStream_t)stream);
    return sg_launched("sg_bias_act_forward");
}
extern "C" int sg_bias_act_backward(int N, int C, int act, const float *z, const float *row_offset, const float *dh,
                                    void *ws, float *dz, float *dbias, void *stream)
{
    if (N <= 0 || C <= 0 || C > 128 || act < 0 || act > 3 || !z || !dh || !ws || !dz)
        return sg_set_error("sg_bias_act_backward: bad argument (C <= 128)", hipSuccess);
    sg_launch_bias_act_bwd(N, C, act, z, row_offset, dh, ws, dz, dbias, (hipStream_t)stream);
    return sg_launched("sg_bias_act_backward");
}

extern "C" int sg_scales_head_forward(int N, const float *z, float *scales_out, float *aux_out, void *stream)
{
    if (N <= 0 || !z || !scales_out || !aux_out) return sg_set_error("sg_scales_head_forward: bad argument", hipSuccess);
    sg_launch_scales_head(N, z, scales_out, aux_out, nullptr, nullptr, nullptr, (hipStream_t)stream);
    return sg_launched("sg_scales_head_forward");
}
extern "C" int sg_scales_head_backward(int N, const float *z, const float *dscales, const float *daux, float *dz, void *stream)
{
    if (N <= 0 || !z || !dz || (!dscales && !daux)) return sg_set_error("sg_scales_head_backward: bad argument", hipSuccess);
    sg_launch_scales_head(N, z, nullptr, nullptr, dscales, daux, dz, (hipStream_t)stream);
    return sg_launched("sg_scales_head_backward");
}

// ---- decoder layers as fused MFMA kernels (f3)
extern "C" int sg_linear_forward(int N, int Cin, int Cout, int act, const float *x, const float *W, const float *bias,
                                 const float *row_offset, float *z_out, float *h_out, void *stream)
{
    if (N <= 0 || !x || !W || !h_out || act < 0 || act > 3) return sg_set_error("sg_linear_forward: bad argument", hipSuccess);
    if (sg_launch_linear_fwd(N, Cin, Cout, act, x, W, bias, row_offset, z_out, h_out, (hipStream_t)stream))
        return sg_set_error("sg_linear_forward: 1 <= Cin, Cout <= 128", hipSuccess);
    return sg_launched("sg_linear_forward");
}
static int sg_linear_backward_impl(const char *who, int N, int Cin, int Cout, int act, const float *z, const float *row_offset,
                                   const float *dh, const float *W, float *dz_out, float *dx_out, void *stream, int accumulate)
{
    if (N <= 0 || !dh || !W || !dx_out || act < 0 || act > 3 || (act != 0 && !z)) return sg_set_error(who, hipSuccess);
    if (accumulate && (Cin & 31)) return sg_set_error("sg_linear_backward_accumulate: Cin must be a multiple of 32", hipSuccess);
    if (sg_launch_linear_bwd(N, Cin, Cout, act, z, row_offset, dh, W, dz_out, dx_out, (hipStream_t)stream, accumulate))
        return sg_set_error("sg_linear_backward: 1 <= Cin, Cout <= 128 (accumulate: N Cin < 2^29)", hipSuccess);
    return sg_launched(who);
}
extern "C" int sg_linear_backward(int N, int Cin, int Cout, int act, const float *z, const float *row_offset, const float *dh,
                                  const float *W, float *dz_out, float *dx_out, void *stream)
{
    return sg_linear_backward_impl("sg_linear_backward: bad argument", N, Cin, Cout, act, z, row_offset, dh, W, dz_out, dx_out, stream, 0);
}
extern "C" int sg_linear_backward_accumulate(int N, int Cin, int Cout, int act, const float *z, const float *row_offset,
                                             const float *dh, const float *W, float *dz_out, float *dx_out, void *stream)
{
    return sg_linear_backward_impl("sg_linear_backward_accumulate: bad argument", N, Cin, Cout, act, z, row_offset, dh, W, dz_out, dx_out,
                                   stream, 1);
}
extern "C" int sg_linear_backward_fan(int N, int Cin, int Cout, int act, const float *z, const float *dh, const float *W,
                                      float *dz_out, float *dx_out, const SgLinearSide side[2], void *stream)
{
    if (N <= 0 || !dh || !W || !dx_out || !side || act < 0 || act > 3 || (act != 0 && !z))
        return sg_set_error("sg_linear_backward_fan: bad argument", hipSuccess);
    for (int i = 0; i < 2; i++) {
        const SgLinearSide &s = side[i];
        if (s.cout < 0 || s.cout > 16 || (s.cout && (!s.dh || !s.W || (s.act != 0 && s.act != 2) || (s.act == 2 && !s.aux))))
            return sg_set_error("sg_linear_backward_fan: a head needs dh, W, act 0 | 2 (with aux)", hipSuccess);
    }
    if (side[0].cout + side[1].cout == 0) return sg_set_error("sg_linear_backward_fan: no head (use sg_linear_backward)", hipSuccess);
    if (sg_launch_linear_bwd_fan(N, Cin, Cout, act, z, dh, W, dz_out, dx_out, side, (hipStream_t)stream))
        return sg_set_error("sg_linear_backward_fan: Cin a multiple of 32 <= 128, Cout a multiple of 4 <= 128, heads <= 16 columns", hipSuccess);
    return sg_launched("sg_linear_backward_fan");
}

extern "C" size_t sg_weight_grad_ws_bytes(int N, int Cout, int Cin)
{
    return N > 0 && Cout > 0 && Cin > 0 ? sg_weight_grad_ws_bytes_impl(N, Cout, Cin) : 0;
}
extern "C" int sg_weight_grad(int N, int Cout, int Cin, const float *dz, const float *x, void *ws, float *dW, float *db,
                              void *stream)
{
    if (N <= 0 || !dz || !x || !ws || !dW) return sg_set_error("sg_weight_grad: bad argument", hipSuccess);
    if (sg_launch_weight_grad(N, Cout, Cin, dz, x, ws, dW, db, (hipStream_t)stream))
        return sg_set_error("sg_weight_grad: Cin must be 32/64/96/128 and Cout <= 128", hipSuccess);
    return sg_launched("sg_weight_grad");
}
