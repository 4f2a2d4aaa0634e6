/*
 * sings_scene.h -- several avatars in one frame through the fused K-frame forward.
 *
 * The reference renders a scene of avatars by posing each of them, concatenating the posed Gaussians (SH block included) and
 * rasterizing once (sings/rec/renderer/gs_renderer_multiple.py:12-68 behind SinGaussianTrainer.animate_more_without_render,
 * gs_trainer.py:732-754).  Here the LBS-fused preprocess looks up which avatar a workgroup's 256 Gaussians belong to, skins them
 * with that avatar's joints, weights and placement, and writes into ONE set of geometry records; binning and the composites see
 * nothing but Ptot records.  Nothing is concatenated and no posed value touches HBM unless the caller asks for it.
 *
 * Gaussian ids: Ptot = sum P_s; avatar s owns [start_s, start_s + P_s), start_s = sum of P_t over t < s, with no padding in
 * anything a caller sees (radii, posed outputs, the workspaces' records).  Every value is what sg_skinned_forward_frames gives
 * for that avatar alone, bit for bit; the image is what sg_rasterize_forward gives for the concatenated posed sets.
 *
 * Forward only, as the reference uses it (no_grad) and as ext_tfs are in sings_hip.h.  One sh_coeffs and one sh_degree for the
 * scene, from the settings (the reference takes the first avatar's degree for all).
 *
 * Same contract as sings_hip.h (which this header includes): plain C, raw device pointers, a hipStream_t as void *, status 0 or
 * non-zero with sg_last_error(), nothing synchronises unless num_rendered_host is given.  These functions are not part of
 * SG_ABI_VERSION's table: a library either exports them all or predates this header.
 */
#ifndef SINGS_SCENE_H
#define SINGS_SCENE_H

#include "sings_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SG_SCENE_MAX_AVATARS 8

/* One avatar of the scene.  The array of S of them lives in HOST memory and is read during the call; its pointers are device
 * pointers.  Every per-frame array has K rows (a caller with one value for all frames repeats it). */
typedef struct SgSceneAvatar {
    int32_t P, J, rot_format, reserved;     /* P >= 1; 1 <= J <= 64; SG_ROT_CANON_*; reserved = 0 */
    const float *xyz_canon;                 /* [P,3] */
    const float *rot_canon;                 /* [P,9] or [P,6] (rot_format); NULL = isotropic */
    const float *lbs_weights;               /* [P,J] */
    const float *scales;                    /* [P,3] */
    const float *opacities;                 /* [P] */
    const float *shs;                       /* [P,M,3], M = SgRasterSettings.sh_coeffs */
    const float *A;                         /* [K,J,16] */
    const float *transl;                    /* [K,3] or NULL */
    const float *smpl_scale;                /* [K] or NULL */
    const float *ext_trans;                 /* [K,3] */
    const float *ext_rot;                   /* [K,9] */
    const float *ext_scale;                 /* [K]; the three ext pointers: all or none */
} SgSceneAvatar;

/* K frames of S avatars.  camera_stride 0: one camera for all frames, 1: one per frame (as SgFrameBatch.camera_stride).
 * Workspaces: those of sg_frames_layout(Ptot, W, H, cap, K, ...); counts: num_rendered_host [K] here, or later with
 * sg_read_num_rendered_frames(..., Ptot, ...).  radii [K,Ptot]; posed_xyz / posed_rotq / posed_scales [K,Ptot,3|4|3] or NULL.
 * Flags: what sg_skinned_forward_frames accepts.
 * Refused (status 1, before any HIP call): S outside 1..SG_SCENE_MAX_AVATARS, K outside 1..16, camera_stride not 0 or 1, a NULL
 * avatars array; per avatar P < 1, J outside 1..64, an unknown rot_format, reserved != 0, ext pointers neither all nor none, a
 * NULL required pointer; bad settings, a NULL workspace / out_color / radii, sh_coeffs < (sh_degree + 1)^2. */
int sg_scene_forward_frames(const SgRasterSettings *s, int K, int camera_stride, int S, const SgSceneAvatar *avatars,
                            void *geom_ws, void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                            float *posed_xyz, float *posed_rotq, float *posed_scales, int64_t *num_rendered_host, void *stream);

/* The same with the depth and alpha maps of every frame: aux_ws of sg_frames_aux_layout(Ptot, ...), out_depth / out_alpha
 * [K,1,H,W].  Flags: what sg_skinned_forward_frames_aux accepts. */
int sg_scene_forward_frames_aux(const SgRasterSettings *s, int K, int camera_stride, int S, const SgSceneAvatar *avatars,
                                void *geom_ws, void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                                float *posed_xyz, float *posed_rotq, float *posed_scales, int64_t *num_rendered_host,
                                void *aux_ws, float *out_depth, float *out_alpha, void *stream);

#ifdef __cplusplus
}
#endif
#endif
