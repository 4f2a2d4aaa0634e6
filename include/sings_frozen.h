/*
 * sings_frozen.h -- the two decoders without a gradient, one launch each.
 *
 * The reference trains its first `opt_geo_from` / `opt_app_from` iterations with the decoders frozen (gs_trainer.py:225-226,
 * sings_hybrid.py:265-277: a decoder whose flag is False runs under torch.no_grad()).  A decoder that is never differentiated needs
 * no saved activation: these entry points read the tri-plane features [N, Cin] and write the decoder's outputs, nothing else.
 * The hidden layers stay in LDS.
 *
 *   geometry   (modules/decoders.py:57-110)   t = gelu(net.2(gelu(net.0(x))))
 *                                             xyz_offsets = xyz_offsets(t);  rotations = rotations.0(t)  (anisotropic)
 *                                             z = scales.2(gelu(scales.0(t)));  scales_aux = z;  scales = log(exp(z) + 1)
 *                                             isotropic: z is one column, both outputs repeat it three times
 *   appearance (modules/decoders.py:16-54)    t = gelu(net.2(gelu(net.0(x))))
 *                                             shs = shs(t) [N,48];  opacity = sigmoid(opacity(t) + opacity_offset[n])
 *
 * fp32 in and out, exact fp32 products (v_mfma_f32_32x32x2_f32), the GELU of sg_linear_forward's epilogue: the results differ from
 * the per-layer kernels' by summation order only.
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises.  These functions are not part of SG_ABI_VERSION's table: a library either
 * exports them all or predates this header.
 */
#ifndef SINGS_FROZEN_H
#define SINGS_FROZEN_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_FROZEN_BLOCK 128             /* points per workgroup */
#define SG_FROZEN_SHS 48                /* columns of the shs head */

/* Every weight is row-major [out, in] with its bias [out], as nn.Linear keeps them; every pointer 16-byte aligned.
 * Refused (status 1, before any HIP call): N < 1, Cin not a multiple of 4 in 4..128, hidden not 64 or 128, a NULL required
 * pointer, a pointer that is not 16-byte aligned. */

/* feats [N,Cin] -> xyz_offsets [N,3], scales [N,3], scales_aux [N,3], rotations [N,6] (anisotropic only).
 * anisotropic = 0: W_scales2 [1,hidden], W_rot / b_rot / rotations ignored (may be NULL);  1: W_scales2 [3,hidden], W_rot [6,hidden]. */
int sg_frozen_geometry(int N, int Cin, int hidden, int anisotropic, const float *feats, const float *W_net0, const float *b_net0,
                       const float *W_net2, const float *b_net2, const float *W_scales0, const float *b_scales0,
                       const float *W_scales2, const float *b_scales2, const float *W_xyz, const float *b_xyz, const float *W_rot,
                       const float *b_rot, float *xyz_offsets, float *scales, float *scales_aux, float *rotations, void *stream);

/* feats [N,Cin] -> shs [N,48], opacity [N,1].  W_opacity NULL: no opacity head (fixed_opacity), b_opacity / opacity_offset /
 * opacity ignored.  opacity_offset [N] or NULL. */
int sg_frozen_appearance(int N, int Cin, int hidden, const float *feats, const float *W_net0, const float *b_net0,
                         const float *W_net2, const float *b_net2, const float *W_shs, const float *b_shs, const float *W_opacity,
                         const float *b_opacity, const float *opacity_offset, float *shs, float *opacity, void *stream);

#ifdef __cplusplus
}
#endif
#endif
