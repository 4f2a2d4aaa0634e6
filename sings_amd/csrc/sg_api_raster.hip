// extern "C" boundary of the rasterizer (see include/sings_hip.h): settings -> camera, the frame batch, the early pair count,
// and the forward / backward entry points of the plain and the skinned paths, with and without the depth / alpha maps.
#include "sg_host.h"
#include "../../include/sings_order.h"
#include "../../include/sings_scene.h"

#include <chrono>
#include <stdlib.h>
#include <thread>

static int sg_make_cam(const SgRasterSettings *s, SgCam *c)
{
    if (!s || s->image_width <= 0 || s->image_height <= 0 || !s->viewmatrix || !s->projmatrix || !s->campos || !s->bg)
        return 1;
    if (s->sh_degree < 0 || s->sh_degree > 3) return 1;
    c->W = s->image_width; c->H = s->image_height;
    c->gx = (c->W + SG_TILE - 1) / SG_TILE; c->gy = (c->H + SG_TILE - 1) / SG_TILE;
    if ((size_t)c->gx * (size_t)c->gy >= SG_MAX_TILES) return 1;      // tile id | segment << 20 (backward work items)
    c->tanfovx = s->tanfovx; c->tanfovy = s->tanfovy;
    c->fx = (float)c->W / (2.0f * s->tanfovx); c->fy = (float)c->H / (2.0f * s->tanfovy);
    c->mod = s->scale_modifier; c->D = s->sh_degree; c->M = s->sh_coeffs; c->flags = s->flags;
    c->view = s->viewmatrix; c->proj = s->projmatrix; c->campos = s->campos; c->bg = s->bg;
    c->count_signal = nullptr;
    return 0;
}

// Early pair count (SgRasterSettings.count_signal): armed only for calls that want R back, cleared before the first launch.
static void sg_arm_count(const SgRasterSettings *s, SgCam *c, const int64_t *num_rendered_host)
{
    if (!num_rendered_host || !s->count_signal || !s->count_signal_host) return;
    __atomic_store_n(s->count_signal_host, 0ull, __ATOMIC_RELEASE);
    c->count_signal = s->count_signal;
}

// R for the caller: from the published word once it arrives (no stream synchronisation), otherwise -- no signal word, debug
// mode, or nothing after SG_SIGNAL_TIMEOUT_MS (a kernel that failed to launch never publishes) -- the synchronous read.
#define SG_SIGNAL_TIMEOUT_MS 50.0
// (SINGS_SIGNAL_TIMEOUT_MS in the environment overrides the 50 ms, read once: a caller that queues more than that in front of
// a forward -- large scenes, a shared GPU -- would otherwise spin 50 ms and then synchronise the stream on every call)
static double sg_signal_timeout_ms()
{
    static const double v = [] {
        const char *e = getenv("SINGS_SIGNAL_TIMEOUT_MS");
        const double x = e ? atof(e) : 0.0;
        return x > 0.0 ? x : SG_SIGNAL_TIMEOUT_MS;
    }();
    return v;
}
static int sg_finish_count(const SgRasterSettings *s, const SgCam &c, const void *binning_ws, int64_t *num_rendered_host, void *stream)
{
    if (!num_rendered_host) return 0;
    if (c.count_signal) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 0;; spin++) {
            const unsigned long long v = __atomic_load_n(s->count_signal_host, __ATOMIC_ACQUIRE);
            if (v >> 63) {
                const uint32_t flags = (uint32_t)(v >> 32) & 0x7fffffffu;
                *num_rendered_host = (flags & 2u) ? (int64_t)SG_NUM_RENDERED_LONG_LIST : (int64_t)(v & 0xffffffffull);
                return 0;
            }
            if ((spin & 63u) == 63u) {
                const double waited = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (waited > sg_signal_timeout_ms()) break;
                // a queue that is more than ~0.2 ms deep in front of the binning kernel: stop burning the core, yield between looks
                if (waited > 0.2) std::this_thread::yield();
            } else {
#if defined(__x86_64__) || defined(__i386__)
                __builtin_ia32_pause();
#endif
            }
        }
    }
    return sg_read_num_rendered(binning_ws, num_rendered_host, stream);
}

static int sg_check_skin(const SgSkinInputs *k, int P, bool fwd)
{
    if (!k || k->J <= 0 || k->J > 64) return 1;
    if (k->rot_format != SG_ROT_CANON_MATRIX && k->rot_format != SG_ROT_CANON_6D) return 1;
    if (P > 0 && (!k->xyz_canon || !k->lbs_weights || !k->A)) return 1;
    int e = (k->ext_trans != nullptr) + (k->ext_rot != nullptr) + (k->ext_scale != nullptr);
    if (e != 0 && e != 3) return 1;
    if (!fwd && e) return 1;
    return 0;
}

// ---- K frames per call ---------------------------------------------------------------------------------------------------
static const SgFrameBatch SG_ONE_FRAME = { 1, 0, 0, 0 };

// SgFrameBatch -> the kernels' SgBatch (strides of the K consecutive workspaces: sg_layout's sizes)
static int sg_make_batch(const SgFrameBatch *fb, int P, const SgCam &c, const SgLayout &L, size_t cap, SgBatch *bt)
{
    if (!fb || fb->K < 1 || fb->K > SG_MAX_FRAMES) return 1;
    if (fb->camera_stride != 0 && fb->camera_stride != 1) return 1;
    if (fb->transl_stride != 0 && fb->transl_stride != 3) return 1;
    bt->K = fb->K; bt->cam_stride = fb->camera_stride; bt->transl_stride = fb->transl_stride; bt->P = P;
    bt->placement = fb->placement;                                   // (checked by sg_check_placement)
    bt->geom = L.geom_bytes; bt->bin = L.bin_bytes; bt->img = L.img_bytes; bt->rec = sg_rec_bytes(cap);
    bt->image = (size_t)3 * (size_t)c.W * (size_t)c.H;
    return 0;
}

// SgFrameBatch.placement (SG_PLACEMENT_*), checked before anything else of the frame batch is used: `skin` is the call's skin inputs
// for the skinned K-frame forward, the only calls that take the bits; nullptr for every other entry point (any bit refused)
static int sg_check_placement(const char *who, const SgFrameBatch *fb, const SgSkinInputs *skin)
{
    if (!fb || !fb->placement) return 0;
    const int known = SG_PLACEMENT_EXT_TFS | SG_PLACEMENT_SMPL_SCALE;
    if (fb->placement & ~known) return sg_failf("%s: unknown SgFrameBatch.placement bits 0x%x", who, fb->placement & ~known);
    if (!skin) {
        const char *flag = (fb->placement & SG_PLACEMENT_EXT_TFS) ? "SG_PLACEMENT_EXT_TFS" : "SG_PLACEMENT_SMPL_SCALE";
        return sg_failf("%s: %s is not supported here (per-frame ext_tfs / smpl_scale are forward-only: the skinned K-frame forward)",
                        who, flag);
    }
    if ((fb->placement & SG_PLACEMENT_EXT_TFS) && !(skin->ext_trans && skin->ext_rot && skin->ext_scale))
        return sg_failf("%s: SG_PLACEMENT_EXT_TFS without ext_trans / ext_rot / ext_scale", who);
    if ((fb->placement & SG_PLACEMENT_SMPL_SCALE) && !skin->smpl_scale)
        return sg_failf("%s: SG_PLACEMENT_SMPL_SCALE without smpl_scale", who);
    return 0;
}

// the K pair counts for the caller: one strided copy of (R, flags) of every frame's header behind the forward, then a wait
static int sg_read_counts(const void *binning_ws, size_t bin_stride, int K, int64_t *num_rendered_host, void *stream)
{
    uint32_t r[2 * SG_MAX_FRAMES];
    hipError_t e = hipMemcpy2DAsync(r, 8, binning_ws, bin_stride ? bin_stride : 8, 8, (size_t)K, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return sg_set_error("sg_read_num_rendered", e);
    for (int f = 0; f < K; f++)
        num_rendered_host[f] = (r[2 * f + 1] & 2u) ? (int64_t)SG_NUM_RENDERED_LONG_LIST : (int64_t)r[2 * f];
    return 0;
}

// Which depth / alpha maps an entry point adds to its colour path: none, one view's (the single-frame *_aux calls) or K frames'
// (the *_frames_aux calls: frame f's aux workspace and maps at the SgAuxFwd / SgAuxBwd strides).
enum SgAux { SG_AUX_NONE, SG_AUX_ONE, SG_AUX_FRAMES };

// The flags the depth / alpha entry points accept: the learned list hints and the clean-workspace promise.  THROUGHPUT, the
// FORWARD_BINNING / FORWARD_COMPOSITE split and SH_PLANAR select kernels or layouts that have no AUX variant.
// The K-frame entry points (`frames`) also accept THROUGHPUT: their composites are the frames kernels, which have AUX variants.
static int sg_aux_flags(const char *who, int flags, bool frames)
{
    static const struct { int bit; const char *name; } refused[] = {
        { SG_FLAG_THROUGHPUT, "SG_FLAG_THROUGHPUT" }, { SG_FLAG_FORWARD_BINNING, "SG_FLAG_FORWARD_BINNING" },
        { SG_FLAG_FORWARD_COMPOSITE, "SG_FLAG_FORWARD_COMPOSITE" }, { SG_FLAG_SH_PLANAR, "SG_FLAG_SH_PLANAR" } };
    for (const auto &r : refused)
        if ((flags & r.bit) && !(frames && r.bit == SG_FLAG_THROUGHPUT))
            return sg_failf("%s: %s is not supported with depth / alpha maps", who, r.name);
    const int known = SG_FLAG_SHORT_LISTS | SG_FLAG_LONG_ROWS | SG_FLAG_WS_CLEAN | (frames ? SG_FLAG_THROUGHPUT : 0);
    if (flags & ~known) return sg_failf("%s: unknown flags 0x%x", who, flags & ~known);
    return 0;
}

// A work order (include/sings_order.h) is P entries or none; the kernels never dereference an entry >= P.
static int sg_check_order(const char *who, const uint32_t *order, int order_len, int P)
{
    if (!order) return order_len ? sg_failf("%s: order_len %d without an order", who, order_len) : 0;
    if (order_len != P) return sg_failf("%s: the order has %d entries, the call %d Gaussians", who, order_len, P);
    return 0;
}

static int sg_forward_impl(const char *who, const SgRasterSettings *s, const SgFrameBatch *fb, int P, const SgSkinInputs *skin,
                           const float *means3D, const float *shs, const float *colors_precomp, const float *opacities,
                           const float *scales, const float *rotations, const float *cov3D_precomp, void *geom_ws, void *binning_ws,
                           size_t cap, void *image_ws, float *out_color, int32_t *radii, float *posed_xyz, float *posed_rotq,
                           float *posed_scales, int write_point_keys, int64_t *num_rendered_host, void *stream,
                           SgAux aux = SG_AUX_NONE, void *aux_ws = nullptr, float *out_depth = nullptr, float *out_alpha = nullptr,
                           const uint32_t *order = nullptr, int order_len = 0, const SgSceneAvatar *scene = nullptr, int scene_S = 0)
{
    // (scene != null, include/sings_scene.h: scene_S checked avatars whose Gaussians sum to P; the preprocess launch is theirs)
    hipStream_t st = (hipStream_t)stream;
    SgCam c;
    if (sg_check_order(who, order, order_len, P)) return 1;
    if (aux && !aux_ws) return sg_failf("%s: null pointer (aux_ws)", who);
    if (sg_make_cam(s, &c)) return sg_failf("%s: bad settings", who);
    if (aux) {
        if (sg_aux_flags(who, c.flags, aux == SG_AUX_FRAMES)) return 1;
        if (!out_depth || !out_alpha) return sg_failf("%s: null pointer (out_depth / out_alpha)", who);
    }
    if (scene) {
        if (!geom_ws || !binning_ws || !image_ws || !out_color || !radii) return sg_failf("%s: null pointer", who);
        if (s->sh_coeffs < (s->sh_degree + 1) * (s->sh_degree + 1)) return sg_failf("%s: sh_coeffs smaller than (sh_degree+1)^2", who);
    } else if (skin) {
        if (sg_check_skin(skin, P, true)) return sg_failf("%s: bad skin inputs (J in 1..64, ext_tfs all or none)", who);
        if (sg_check_placement(who, fb, skin)) return 1;
        if (P < 0 || !geom_ws || !binning_ws || !image_ws || !out_color || (P > 0 && (!shs || !opacities || !scales || !radii)))
            return sg_failf("%s: null pointer", who);
        if (s->sh_coeffs < (s->sh_degree + 1) * (s->sh_degree + 1)) return sg_failf("%s: sh_coeffs smaller than (sh_degree+1)^2", who);
    } else {
        if (sg_check_placement(who, fb, nullptr)) return 1;
        if (P < 0 || !geom_ws || !binning_ws || !image_ws || !out_color || (P > 0 && (!means3D || !opacities || !radii)))
            return sg_failf("%s: null pointer", who);
        if (P > 0 && ((shs != nullptr) == (colors_precomp != nullptr))) return sg_failf("%s: provide exactly one of shs / colors_precomp", who);
        if (P > 0 && (((scales != nullptr) && (rotations != nullptr)) == (cov3D_precomp != nullptr)))
            return sg_failf("%s: provide exactly one of (scales,rotations) / cov3D_precomp", who);
        if (shs && (s->sh_coeffs < (s->sh_degree + 1) * (s->sh_degree + 1))) return sg_failf("%s: sh_coeffs smaller than (sh_degree+1)^2", who);
    }
    SgLayout L;
    sg_layout(P, c.W, c.H, cap, &L);
    SgBatch bt;
    if (sg_make_batch(fb, P, c, L, cap, &bt)) return sg_failf("%s: bad frame batch (K in 1..16, camera_stride 0|1, transl_stride 0|3)", who);
    SgGeom g = sg_geom_view(geom_ws, L);
    SgBin b = sg_bin_view(binning_ws, L);
    SgImg im = sg_img_view(image_ws, L);
    // header + tile counters: zeroed here unless the caller vouches for them (SG_FLAG_WS_CLEAN; the forward composite
    // leaves them zeroed for the next call).  (The early pair count -- one mapped host word -- serves single-frame calls.)
    const bool do_bin = !(c.flags & SG_FLAG_FORWARD_COMPOSITE), do_comp = !(c.flags & SG_FLAG_FORWARD_BINNING);
    if (!do_bin && !do_comp) return sg_failf("%s: SG_FLAG_FORWARD_BINNING and SG_FLAG_FORWARD_COMPOSITE exclude each other", who);
    if (do_bin) {
        if (bt.K == 1) sg_arm_count(s, &c, num_rendered_host);
        if (!(c.flags & SG_FLAG_WS_CLEAN)) {
            const size_t zb = (L.bin_tile_count - L.bin_header) + sg_ctr_count((uint32_t)c.gx, (uint32_t)c.gy) * 4;
            for (int f = 0; f < bt.K; f++) sg_zero_async((char *)b.header + (size_t)f * bt.bin, zb, st);
        }
        if (scene) sg_launch_scene_fwd(c, bt, scene_S, scene, g, b, cap, radii, posed_xyz, posed_rotq, posed_scales, st);
        else if (skin) sg_launch_skin_fwd(c, bt, P, skin, shs, opacities, scales, g, b, cap, radii, posed_xyz, posed_rotq, posed_scales, st);
        else sg_launch_preprocess_fwd_ordered(c, bt, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, g, b, cap,
                                              radii, order, st);
        SG_CHECK_LAST("preprocess_fwd", s, st);
        sg_launch_binning(c, bt, P, radii, g, b, cap, write_point_keys, st);
        SG_CHECK_LAST("binning", s, st);
    }
    if (do_comp) {
        SgAuxFwd ax = sg_aux_fwd_view(aux_ws, g, out_depth, out_alpha);
        ax.ws = sg_aux_bytes(cap); ax.map = (size_t)c.W * (size_t)c.H;       // (frame f of a K-frame call; unused by one frame)
        sg_launch_render_fwd(c, bt, g, b, cap, im, out_color, write_point_keys, st, aux ? &ax : nullptr);
        SG_CHECK_LAST("render_fwd", s, st);
    }
    if (!do_bin) return 0;
    if (bt.K == 1) return sg_finish_count(s, c, binning_ws, num_rendered_host, stream);
    return num_rendered_host ? sg_read_counts(binning_ws, bt.bin, bt.K, num_rendered_host, stream) : 0;
}

extern "C" int sg_rasterize_forward(const SgRasterSettings *s, int P, const float *means3D, const float *shs,
                                    const float *colors_precomp, const float *opacities, const float *scales,
                                    const float *rotations, const float *cov3D_precomp, void *geom_ws,
                                    void *binning_ws, size_t cap, void *image_ws, float *out_color,
                                    int32_t *radii, int write_point_keys, int64_t *num_rendered_host, void *stream)
{
    return sg_forward_impl("sg_rasterize_forward", s, &SG_ONE_FRAME, P, nullptr, means3D, shs, colors_precomp, opacities, scales,
                           rotations, cov3D_precomp, geom_ws, binning_ws, cap, image_ws, out_color, radii, nullptr, nullptr, nullptr,
                           write_point_keys, num_rendered_host, stream);
}

extern "C" int sg_rasterize_forward_frames(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const float *means3D,
                                           const float *shs, const float *colors_precomp, const float *opacities,
                                           const float *scales, const float *rotations, const float *cov3D_precomp, void *geom_ws,
                                           void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                                           int64_t *num_rendered_host, void *stream)
{
    return sg_forward_impl("sg_rasterize_forward_frames", s, fb, P, nullptr, means3D, shs, colors_precomp, opacities, scales,
                           rotations, cov3D_precomp, geom_ws, binning_ws, cap, image_ws, out_color, radii, nullptr, nullptr, nullptr,
                           0, num_rendered_host, stream);
}

extern "C" int sg_read_num_rendered(const void *binning_ws, int64_t *num_rendered_host, void *stream)
{
    if (!binning_ws || !num_rendered_host) return sg_set_error("sg_read_num_rendered: null pointer", hipSuccess);
    return sg_read_counts(binning_ws, 0, 1, num_rendered_host, stream);      // header words 0 (R) and 1 (bit 0: R > capacity, bit 1: long list)
}

extern "C" int sg_read_num_rendered_frames(const void *binning_ws, int P, int width, int height, size_t cap, int K,
                                           int64_t *num_rendered_host, void *stream)
{
    SgLayout L;
    if (!binning_ws || !num_rendered_host || K < 1 || K > SG_MAX_FRAMES) return sg_set_error("sg_read_num_rendered_frames: bad argument", hipSuccess);
    if (sg_layout(P, width, height, cap, &L)) return 1;
    return sg_read_counts(binning_ws, L.bin_bytes, K, num_rendered_host, stream);
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// Every backward entry point checks, in this order: settings, the flags of the maps, accumulate (refused with the maps), skin inputs,
// the frame batch's placement bits (forward-only: refused), aux_ws (sg_bwd_check); then returns 0 for P <= 0, checks its other
// pointers and last the rest of its frame batch (sg_bwd_layout).
static int sg_bwd_check(const char *who, const SgRasterSettings *s, SgCam *c, SgAux aux, int accumulate, bool skinned,
                        const SgSkinInputs *skin, int P, const void *aux_ws, const SgFrameBatch *fb)
{
    if (sg_make_cam(s, c)) return sg_failf("%s: bad settings", who);
    if (aux && sg_aux_flags(who, c->flags, aux == SG_AUX_FRAMES)) return 1;
    if (aux && accumulate) return sg_failf("%s: accumulate != 0 is not supported with depth / alpha maps", who);
    if (skinned && sg_check_skin(skin, P, false)) return sg_failf("%s: bad skin inputs (ext_tfs are forward-only)", who);
    if (sg_check_placement(who, fb, nullptr)) return 1;
    if (aux && !aux_ws) return sg_failf("%s: null pointer (aux_ws)", who);
    return 0;
}
static int sg_bwd_layout(const char *who, const SgFrameBatch *fb, int P, const SgCam &c, size_t cap, SgLayout *L, SgBatch *bt)
{
    sg_layout(P, c.W, c.H, cap, L);
    return sg_make_batch(fb, P, c, *L, cap, bt) ? sg_failf("%s: bad frame batch", who) : 0;
}

// first half: per-tile composite -> one gradient record per (tile, Gaussian) pair in bwd_ws; with the maps also the dL/dz plane
// of aux_ws (of every frame's aux workspace)
static int sg_records_impl(const char *who, const SgRasterSettings *s, const SgFrameBatch *fb, int P, const void *geom_ws,
                           const void *binning_ws, size_t cap, const void *image_ws, void *bwd_ws, const float *dL_dout_color,
                           void *stream, SgAux aux = SG_AUX_NONE, void *aux_ws = nullptr, const float *dL_ddepth = nullptr,
                           const float *dL_dalpha = nullptr)
{
    hipStream_t st = (hipStream_t)stream;
    SgCam c;
    SgLayout L;
    SgBatch bt;
    if (sg_bwd_check(who, s, &c, aux, 0, false, nullptr, P, aux_ws, fb)) return 1;
    if (P <= 0) return 0;
    if (!geom_ws || !binning_ws || !image_ws || !bwd_ws || !dL_dout_color) return sg_failf("%s: null pointer", who);
    if (sg_bwd_layout(who, fb, P, c, cap, &L, &bt)) return 1;
    SgGeom g = sg_geom_view((void *)geom_ws, L);
    SgBin b = sg_bin_view((void *)binning_ws, L);
    SgImg im = sg_img_view((void *)image_ws, L);
    SgAuxBwd ax = sg_aux_bwd_view(aux_ws, cap, g, dL_ddepth, dL_dalpha);
    if (aux == SG_AUX_FRAMES) { ax.ws = sg_aux_bytes(cap); ax.map = (size_t)c.W * (size_t)c.H; }
    sg_launch_render_bwd(c, bt, g, b, cap, im, dL_dout_color, sg_rec_view(bwd_ws, cap), st, aux ? &ax : nullptr);
    SG_CHECK_LAST(aux ? "render_bwd_aux" : "render_bwd", s, st);
    return 0;
}

// second half: per Gaussian, the sum of its records (with the maps: and of its dL/dz) and the chain rule; accumulate != 0: += into
// the gradient outputs
static int sg_gaussians_impl(const char *who, const SgRasterSettings *s, const SgFrameBatch *fb, int P, const float *means3D,
                             const float *shs, const float *colors_precomp, const float *opacities, const float *scales,
                             const float *rotations, const float *cov3D_precomp, const int32_t *radii, const void *geom_ws,
                             const void *binning_ws, size_t cap, void *bwd_ws, int accumulate, float *dL_dmeans3D,
                             float *dL_dmeans2D, float *dL_dsh, float *dL_dcolors, float *dL_dopacity, float *dL_dscales,
                             float *dL_drotations, float *dL_dcov3D, void *stream, SgAux aux = SG_AUX_NONE, void *aux_ws = nullptr)
{
    hipStream_t st = (hipStream_t)stream;
    SgCam c;
    SgLayout L;
    SgBatch bt;
    if (sg_bwd_check(who, s, &c, aux, accumulate, false, nullptr, P, aux_ws, fb)) return 1;
    if (P <= 0) return 0;
    if (!means3D || !radii || !geom_ws || !binning_ws || !bwd_ws || !dL_dmeans3D || !dL_dmeans2D || !dL_dopacity)
        return sg_failf("%s: null pointer", who);
    if (shs && !dL_dsh) return sg_failf("%s: dL_dsh missing", who);
    if (sg_bwd_layout(who, fb, P, c, cap, &L, &bt)) return 1;
    SgGeom g = sg_geom_view((void *)geom_ws, L);
    SgBin b = sg_bin_view((void *)binning_ws, L);
    sg_launch_preprocess_bwd(c, bt, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii, g,
                             sg_rec_view(bwd_ws, cap), cap, b.header, sg_lds_hist(c.gx, c.gy) ? b.rec_valid : nullptr,
                             bt.K > 1 ? (float4 *)((char *)bwd_ws + (size_t)bt.K * L.bwd_bytes) : nullptr,     // (sg_frames_layout: the a9 block)
                             dL_dmeans3D, dL_dmeans2D, shs ? dL_dsh : nullptr,
                             dL_dcolors, dL_dopacity, cov3D_precomp ? nullptr : dL_dscales,
                             cov3D_precomp ? nullptr : dL_drotations, dL_dcov3D, accumulate, st, sg_aux_dz(aux_ws, cap));
    SG_CHECK_LAST(aux ? "preprocess_bwd_aux" : "preprocess_bwd", s, st);
    return 0;
}

// the skinned second half: the LBS-fused per-Gaussian backward (frame f's dL/dz plane, K frames: at + f sg_aux_bytes)
static int sg_skin_gaussians_impl(const char *who, const SgRasterSettings *s, const SgFrameBatch *fb, int P, const SgSkinInputs *skin,
                                  const float *shs, const float *scales, const int32_t *radii, const void *geom_ws,
                                  const void *binning_ws, size_t cap, const void *bwd_ws, float *skin_ws, int accumulate,
                                  const float *dL_dposed_xyz_in, const float *dL_dposed_rotq_in, float *dL_dxyz_canon,
                                  float *dL_drot_canon, float *dL_dscales, float *dL_dopacity, float *dL_dsh, float *dL_dmeans2D,
                                  float *dL_dA, float *dL_dtransl, void *stream, SgAux aux = SG_AUX_NONE, void *aux_ws = nullptr)
{
    hipStream_t st = (hipStream_t)stream;
    SgCam c;
    SgLayout L;
    SgBatch bt;
    if (sg_bwd_check(who, s, &c, aux, accumulate, true, skin, P, aux_ws, fb)) return 1;
    if (P <= 0) return 0;
    if (!shs || !scales || !radii || !geom_ws || !binning_ws || !bwd_ws || !skin_ws || !dL_dxyz_canon || !dL_dscales ||
        !dL_dopacity || !dL_dsh || !dL_dmeans2D || !dL_dA)
        return sg_failf("%s: null pointer", who);
    if (sg_bwd_layout(who, fb, P, c, cap, &L, &bt)) return 1;
    SgGeom g = sg_geom_view((void *)geom_ws, L);
    SgBin b = sg_bin_view((void *)binning_ws, L);
    sg_launch_skin_bwd(c, bt, P, skin, shs, scales, radii, g, sg_rec_view(bwd_ws, cap), cap, b.header, sg_lds_hist(c.gx, c.gy) ? b.rec_valid : nullptr,
                       dL_dposed_xyz_in, dL_dposed_rotq_in,
                       skin_ws, dL_dxyz_canon, dL_drot_canon, dL_dscales, dL_dopacity, dL_dsh, dL_dmeans2D, dL_dA,
                       dL_dtransl, accumulate, st, sg_aux_dz(aux_ws, cap), aux == SG_AUX_FRAMES ? sg_aux_bytes(cap) : 0);
    SG_CHECK_LAST(aux ? "skin_bwd_aux" : "skin_bwd", s, st);
    return 0;
}

// the whole backward of one view (sg_rasterize_backward / _aux): every pointer of both halves is checked before the first launch
static int sg_rasterize_backward_impl(const char *who, const SgRasterSettings *s, int P, const float *means3D, const float *shs,
                                      const float *colors_precomp, const float *opacities, const float *scales,
                                      const float *rotations, const float *cov3D_precomp, const int32_t *radii,
                                      const void *geom_ws, const void *binning_ws, size_t cap, const void *image_ws,
                                      void *bwd_ws, const float *dL_dout_color, float *dL_dmeans3D, float *dL_dmeans2D,
                                      float *dL_dsh, float *dL_dcolors, float *dL_dopacity, float *dL_dscales,
                                      float *dL_drotations, float *dL_dcov3D, void *stream, SgAux aux = SG_AUX_NONE,
                                      void *aux_ws = nullptr, const float *dL_ddepth = nullptr, const float *dL_dalpha = nullptr)
{
    SgCam c;
    if (sg_bwd_check(who, s, &c, aux, 0, false, nullptr, P, aux_ws, &SG_ONE_FRAME)) return 1;
    if (P <= 0) return 0;
    if (!means3D || !radii || !geom_ws || !binning_ws || !image_ws || !bwd_ws || !dL_dout_color || !dL_dmeans3D ||
        !dL_dmeans2D || !dL_dopacity)
        return sg_failf("%s: null pointer", who);
    if (shs && !dL_dsh) return sg_failf("%s: dL_dsh missing", who);
    int rc = sg_records_impl(who, s, &SG_ONE_FRAME, P, geom_ws, binning_ws, cap, image_ws, bwd_ws, dL_dout_color, stream, aux, aux_ws,
                             dL_ddepth, dL_dalpha);
    if (rc) return rc;
    return sg_gaussians_impl(who, s, &SG_ONE_FRAME, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, radii,
                             geom_ws, binning_ws, cap, bwd_ws, 0, dL_dmeans3D, dL_dmeans2D, dL_dsh, dL_dcolors, dL_dopacity,
                             dL_dscales, dL_drotations, dL_dcov3D, stream, aux, aux_ws);
}

extern "C" int sg_rasterize_backward(const SgRasterSettings *s, int P, const float *means3D, const float *shs,
                                     const float *colors_precomp, const float *opacities, const float *scales,
                                     const float *rotations, const float *cov3D_precomp, const int32_t *radii,
                                     const void *geom_ws, const void *binning_ws, size_t cap, const void *image_ws,
                                     void *bwd_ws, const float *dL_dout_color, float *dL_dmeans3D,
                                     float *dL_dmeans2D, float *dL_dsh, float *dL_dcolors, float *dL_dopacity,
                                     float *dL_dscales, float *dL_drotations, float *dL_dcov3D, void *stream)
{
    return sg_rasterize_backward_impl("sg_rasterize_backward", s, P, means3D, shs, colors_precomp, opacities, scales, rotations,
                                      cov3D_precomp, radii, geom_ws, binning_ws, cap, image_ws, bwd_ws, dL_dout_color, dL_dmeans3D,
                                      dL_dmeans2D, dL_dsh, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, stream);
}

extern "C" int sg_rasterize_backward_records_frames(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const void *geom_ws,
                                                    const void *binning_ws, size_t cap, const void *image_ws, void *bwd_ws,
                                                    const float *dL_dout_color, void *stream)
{
    return sg_records_impl("sg_rasterize_backward_records_frames", s, fb, P, geom_ws, binning_ws, cap, image_ws, bwd_ws, dL_dout_color,
                           stream);
}
extern "C" int sg_rasterize_backward_records(const SgRasterSettings *s, int P, const void *geom_ws, const void *binning_ws,
                                             size_t cap, const void *image_ws, void *bwd_ws, const float *dL_dout_color,
                                             void *stream)
{
    return sg_records_impl("sg_rasterize_backward_records", s, &SG_ONE_FRAME, P, geom_ws, binning_ws, cap, image_ws, bwd_ws,
                           dL_dout_color, stream);
}

extern "C" int sg_rasterize_backward_gaussians_frames(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const float *means3D,
                                                      const float *shs, const float *colors_precomp, const float *opacities,
                                                      const float *scales, const float *rotations, const float *cov3D_precomp,
                                                      const int32_t *radii, const void *geom_ws, const void *binning_ws, size_t cap,
                                                      void *bwd_ws, int accumulate, float *dL_dmeans3D, float *dL_dmeans2D,
                                                      float *dL_dsh, float *dL_dcolors, float *dL_dopacity, float *dL_dscales,
                                                      float *dL_drotations, float *dL_dcov3D, void *stream)
{
    return sg_gaussians_impl("sg_rasterize_backward_gaussians_frames", s, fb, P, means3D, shs, colors_precomp, opacities, scales,
                             rotations, cov3D_precomp, radii, geom_ws, binning_ws, cap, bwd_ws, accumulate, dL_dmeans3D, dL_dmeans2D,
                             dL_dsh, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, stream);
}
extern "C" int sg_rasterize_backward_gaussians(const SgRasterSettings *s, int P, const float *means3D, const float *shs,
                                               const float *colors_precomp, const float *opacities, const float *scales,
                                               const float *rotations, const float *cov3D_precomp, const int32_t *radii,
                                               const void *geom_ws, const void *binning_ws, size_t cap, const void *bwd_ws,
                                               int accumulate, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dsh,
                                               float *dL_dcolors, float *dL_dopacity, float *dL_dscales, float *dL_drotations,
                                               float *dL_dcov3D, void *stream)
{
    return sg_gaussians_impl("sg_rasterize_backward_gaussians", s, &SG_ONE_FRAME, P, means3D, shs, colors_precomp, opacities, scales,
                             rotations, cov3D_precomp, radii, geom_ws, binning_ws, cap, (void *)bwd_ws /* K = 1: read only */,
                             accumulate, dL_dmeans3D, dL_dmeans2D, dL_dsh, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations,
                             dL_dcov3D, stream);
}

extern "C" size_t sg_skin_ws_floats(int P) { return sg_skin_slab_floats(P > 0 ? P : 1, 1); }
extern "C" size_t sg_skin_ws_floats_frames(int P, int K) { return sg_skin_slab_floats(P > 0 ? P : 1, K > 0 ? K : 1); }

extern "C" int sg_skinned_forward(const SgRasterSettings *s, int P, const SgSkinInputs *skin, const float *shs,
                                  const float *opacities, const float *scales, void *geom_ws, void *binning_ws,
                                  size_t cap, void *image_ws, float *out_color, int32_t *radii, float *posed_xyz,
                                  float *posed_rotq, float *posed_scales, int64_t *num_rendered_host, void *stream)
{
    return sg_forward_impl("sg_skinned_forward", s, &SG_ONE_FRAME, P, skin, nullptr, shs, nullptr, opacities, scales, nullptr, nullptr,
                           geom_ws, binning_ws, cap, image_ws, out_color, radii, posed_xyz, posed_rotq, posed_scales, 0,
                           num_rendered_host, stream);
}
extern "C" int sg_skinned_forward_frames(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const SgSkinInputs *skin,
                                         const float *shs, const float *opacities, const float *scales, void *geom_ws,
                                         void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                                         float *posed_xyz, float *posed_rotq, float *posed_scales, int64_t *num_rendered_host,
                                         void *stream)
{
    return sg_forward_impl("sg_skinned_forward_frames", s, fb, P, skin, nullptr, shs, nullptr, opacities, scales, nullptr, nullptr,
                           geom_ws, binning_ws, cap, image_ws, out_color, radii, posed_xyz, posed_rotq, posed_scales, 0,
                           num_rendered_host, stream);
}

// the whole skinned backward of one view (sg_skinned_backward / _aux): every pointer of both halves is checked before the first launch
static int sg_skinned_backward_impl(const char *who, const SgRasterSettings *s, int P, const SgSkinInputs *skin, const float *shs,
                                    const float *scales, const int32_t *radii, const void *geom_ws, const void *binning_ws, size_t cap,
                                    const void *image_ws, void *bwd_ws, float *skin_ws, const float *dL_dout_color,
                                    const float *dL_dposed_xyz_in, const float *dL_dposed_rotq_in, float *dL_dxyz_canon,
                                    float *dL_drot_canon, float *dL_dscales, float *dL_dopacity, float *dL_dsh, float *dL_dmeans2D,
                                    float *dL_dA, float *dL_dtransl, void *stream, SgAux aux = SG_AUX_NONE, void *aux_ws = nullptr,
                                    const float *dL_ddepth = nullptr, const float *dL_dalpha = nullptr)
{
    SgCam c;
    if (sg_bwd_check(who, s, &c, aux, 0, true, skin, P, aux_ws, &SG_ONE_FRAME)) return 1;
    if (P <= 0) return 0;
    if (!shs || !scales || !radii || !geom_ws || !binning_ws || !image_ws || !bwd_ws || !skin_ws || !dL_dout_color ||
        !dL_dxyz_canon || !dL_dscales || !dL_dopacity || !dL_dsh || !dL_dmeans2D || !dL_dA)
        return sg_failf("%s: null pointer", who);
    int rc = sg_records_impl(who, s, &SG_ONE_FRAME, P, geom_ws, binning_ws, cap, image_ws, bwd_ws, dL_dout_color, stream, aux, aux_ws,
                             dL_ddepth, dL_dalpha);
    if (rc) return rc;
    return sg_skin_gaussians_impl(who, s, &SG_ONE_FRAME, P, skin, shs, scales, radii, geom_ws, binning_ws, cap, bwd_ws, skin_ws, 0,
                                  dL_dposed_xyz_in, dL_dposed_rotq_in, dL_dxyz_canon, dL_drot_canon, dL_dscales, dL_dopacity, dL_dsh,
                                  dL_dmeans2D, dL_dA, dL_dtransl, stream, aux, aux_ws);
}

extern "C" int sg_skinned_backward(const SgRasterSettings *s, int P, const SgSkinInputs *skin, const float *shs,
                                   const float *opacities, const float *scales, const int32_t *radii,
                                   const void *geom_ws, const void *binning_ws, size_t cap, const void *image_ws,
                                   void *bwd_ws, float *skin_ws, const float *dL_dout_color,
                                   const float *dL_dposed_xyz_in, const float *dL_dposed_rotq_in, float *dL_dxyz_canon,
                                   float *dL_drot_canon, float *dL_dscales, float *dL_dopacity, float *dL_dsh,
                                   float *dL_dmeans2D, float *dL_dA, float *dL_dtransl, void *stream)
{
    (void)opacities;
    return sg_skinned_backward_impl("sg_skinned_backward", s, P, skin, shs, scales, radii, geom_ws, binning_ws, cap, image_ws, bwd_ws,
                                    skin_ws, dL_dout_color, dL_dposed_xyz_in, dL_dposed_rotq_in, dL_dxyz_canon, dL_drot_canon,
                                    dL_dscales, dL_dopacity, dL_dsh, dL_dmeans2D, dL_dA, dL_dtransl, stream);
}

extern "C" int sg_skinned_backward_gaussians_frames(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const SgSkinInputs *skin,
                                                    const float *shs, const float *opacities, const float *scales,
                                                    const int32_t *radii, const void *geom_ws, const void *binning_ws, size_t cap,
                                                    const void *bwd_ws, float *skin_ws, int accumulate,
                                                    const float *dL_dposed_xyz_in, const float *dL_dposed_rotq_in,
                                                    float *dL_dxyz_canon, float *dL_drot_canon, float *dL_dscales,
                                                    float *dL_dopacity, float *dL_dsh, float *dL_dmeans2D, float *dL_dA,
                                                    float *dL_dtransl, void *stream)
{
    (void)opacities;
    return sg_skin_gaussians_impl("sg_skinned_backward_gaussians_frames", s, fb, P, skin, shs, scales, radii, geom_ws, binning_ws, cap,
                                  bwd_ws, skin_ws, accumulate, dL_dposed_xyz_in, dL_dposed_rotq_in, dL_dxyz_canon, dL_drot_canon,
                                  dL_dscales, dL_dopacity, dL_dsh, dL_dmeans2D, dL_dA, dL_dtransl, stream);
}
extern "C" int sg_skinned_backward_gaussians(const SgRasterSettings *s, int P, const SgSkinInputs *skin, const float *shs,
                                             const float *opacities, const float *scales, const int32_t *radii,
                                             const void *geom_ws, const void *binning_ws, size_t cap, const void *bwd_ws,
                                             float *skin_ws, int accumulate, const float *dL_dposed_xyz_in,
                                             const float *dL_dposed_rotq_in, float *dL_dxyz_canon, float *dL_drot_canon,
                                             float *dL_dscales, float *dL_dopacity, float *dL_dsh, float *dL_dmeans2D,
                                             float *dL_dA, float *dL_dtransl, void *stream)
{
    (void)opacities;
    return sg_skin_gaussians_impl("sg_skinned_backward_gaussians", s, &SG_ONE_FRAME, P, skin, shs, scales, radii, geom_ws, binning_ws,
                                  cap, bwd_ws, skin_ws, accumulate, dL_dposed_xyz_in, dL_dposed_rotq_in, dL_dxyz_canon, dL_drot_canon,
                                  dL_dscales, dL_dopacity, dL_dsh, dL_dmeans2D, dL_dA, dL_dtransl, stream);
}

// ---- depth and alpha maps (ABI 8) ----------------------------------------------------------------------------------------------
extern "C" int sg_rasterize_forward_aux(const SgRasterSettings *s, int P, const float *means3D, const float *shs,
                                        const float *colors_precomp, const float *opacities, const float *scales,
                                        const float *rotations, const float *cov3D_precomp, void *geom_ws,
                                        void *binning_ws, size_t cap, void *image_ws, float *out_color,
                                        int32_t *radii, int write_point_keys, int64_t *num_rendered_host, void *aux_ws,
                                        float *out_depth, float *out_alpha, void *stream)
{
    return sg_forward_impl("sg_rasterize_forward_aux", s, &SG_ONE_FRAME, P, nullptr, means3D, shs, colors_precomp, opacities, scales,
                           rotations, cov3D_precomp, geom_ws, binning_ws, cap, image_ws, out_color, radii, nullptr, nullptr, nullptr,
                           write_point_keys, num_rendered_host, stream, SG_AUX_ONE, aux_ws, out_depth, out_alpha);
}

extern "C" int sg_skinned_forward_aux(const SgRasterSettings *s, int P, const SgSkinInputs *skin, const float *shs,
                                      const float *opacities, const float *scales, void *geom_ws, void *binning_ws,
                                      size_t cap, void *image_ws, float *out_color, int32_t *radii, float *posed_xyz,
                                      float *posed_rotq, float *posed_scales, int64_t *num_rendered_host, void *aux_ws,
                                      float *out_depth, float *out_alpha, void *stream)
{
    return sg_forward_impl("sg_skinned_forward_aux", s, &SG_ONE_FRAME, P, skin, nullptr, shs, nullptr, opacities, scales, nullptr, nullptr,
                           geom_ws, binning_ws, cap, image_ws, out_color, radii, posed_xyz, posed_rotq, posed_scales, 0,
                           num_rendered_host, stream, SG_AUX_ONE, aux_ws, out_depth, out_alpha);
}

extern "C" int sg_rasterize_backward_aux(const SgRasterSettings *s, int P, const float *means3D, const float *shs,
                                         const float *colors_precomp, const float *opacities, const float *scales,
                                         const float *rotations, const float *cov3D_precomp, const int32_t *radii,
                                         const void *geom_ws, const void *binning_ws, size_t cap, const void *image_ws,
                                         void *bwd_ws, const float *dL_dout_color, float *dL_dmeans3D,
                                         float *dL_dmeans2D, float *dL_dsh, float *dL_dcolors, float *dL_dopacity,
                                         float *dL_dscales, float *dL_drotations, float *dL_dcov3D, void *aux_ws,
                                         const float *dL_ddepth, const float *dL_dalpha, void *stream)
{
    return sg_rasterize_backward_impl("sg_rasterize_backward_aux", s, P, means3D, shs, colors_precomp, opacities, scales, rotations,
                                      cov3D_precomp, radii, geom_ws, binning_ws, cap, image_ws, bwd_ws, dL_dout_color, dL_dmeans3D,
                                      dL_dmeans2D, dL_dsh, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, stream,
                                      SG_AUX_ONE, aux_ws, dL_ddepth, dL_dalpha);
}

extern "C" int sg_skinned_backward_aux(const SgRasterSettings *s, int P, const SgSkinInputs *skin, const float *shs,
                                       const float *opacities, const float *scales, const int32_t *radii,
                                       const void *geom_ws, const void *binning_ws, size_t cap, const void *image_ws,
                                       void *bwd_ws, float *skin_ws, const float *dL_dout_color,
                                       const float *dL_dposed_xyz_in, const float *dL_dposed_rotq_in, float *dL_dxyz_canon,
                                       float *dL_drot_canon, float *dL_dscales, float *dL_dopacity, float *dL_dsh,
                                       float *dL_dmeans2D, float *dL_dA, float *dL_dtransl, void *aux_ws, const float *dL_ddepth,
                                       const float *dL_dalpha, void *stream)
{
    (void)opacities;
    return sg_skinned_backward_impl("sg_skinned_backward_aux", s, P, skin, shs, scales, radii, geom_ws, binning_ws, cap, image_ws, bwd_ws,
                                    skin_ws, dL_dout_color, dL_dposed_xyz_in, dL_dposed_rotq_in, dL_dxyz_canon, dL_drot_canon,
                                    dL_dscales, dL_dopacity, dL_dsh, dL_dmeans2D, dL_dA, dL_dtransl, stream, SG_AUX_ONE, aux_ws,
                                    dL_ddepth, dL_dalpha);
}

// ---- depth and alpha maps of K frames (ABI 8, entry points added) ----------------------------------------------------------------
extern "C" int sg_skinned_forward_frames_aux(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const SgSkinInputs *skin,
                                             const float *shs, const float *opacities, const float *scales, void *geom_ws,
                                             void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                                             float *posed_xyz, float *posed_rotq, float *posed_scales, int64_t *num_rendered_host,
                                             void *aux_ws, float *out_depth, float *out_alpha, void *stream)
{
    return sg_forward_impl("sg_skinned_forward_frames_aux", s, fb, P, skin, nullptr, shs, nullptr, opacities, scales, nullptr, nullptr,
                           geom_ws, binning_ws, cap, image_ws, out_color, radii, posed_xyz, posed_rotq, posed_scales, 0,
                           num_rendered_host, stream, SG_AUX_FRAMES, aux_ws, out_depth, out_alpha);
}

// the K frames' backward composites with the depth / alpha adjoints (whichever op produced the frames)
extern "C" int sg_rasterize_backward_records_frames_aux(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const void *geom_ws,
                                                        const void *binning_ws, size_t cap, const void *image_ws, void *bwd_ws,
                                                        const float *dL_dout_color, void *aux_ws, const float *dL_ddepth,
                                                        const float *dL_dalpha, void *stream)
{
    return sg_records_impl("sg_rasterize_backward_records_frames_aux", s, fb, P, geom_ws, binning_ws, cap, image_ws, bwd_ws,
                           dL_dout_color, stream, SG_AUX_FRAMES, aux_ws, dL_ddepth, dL_dalpha);
}

extern "C" int sg_skinned_backward_gaussians_frames_aux(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const SgSkinInputs *skin,
                                                        const float *shs, const float *opacities, const float *scales,
                                                        const int32_t *radii, const void *geom_ws, const void *binning_ws, size_t cap,
                                                        const void *bwd_ws, float *skin_ws, int accumulate,
                                                        const float *dL_dposed_xyz_in, const float *dL_dposed_rotq_in,
                                                        float *dL_dxyz_canon, float *dL_drot_canon, float *dL_dscales,
                                                        float *dL_dopacity, float *dL_dsh, float *dL_dmeans2D, float *dL_dA,
                                                        float *dL_dtransl, void *aux_ws, void *stream)
{
    (void)opacities;
    return sg_skin_gaussians_impl("sg_skinned_backward_gaussians_frames_aux", s, fb, P, skin, shs, scales, radii, geom_ws, binning_ws,
                                  cap, bwd_ws, skin_ws, accumulate, dL_dposed_xyz_in, dL_dposed_rotq_in, dL_dxyz_canon, dL_drot_canon,
                                  dL_dscales, dL_dopacity, dL_dsh, dL_dmeans2D, dL_dA, dL_dtransl, stream, SG_AUX_FRAMES, aux_ws);
}

// ---- work order (include/sings_order.h) ------------------------------------------------------------------------------------------
extern "C" int sg_rasterize_forward_frames_ordered(const SgRasterSettings *s, const SgFrameBatch *fb, int P, const float *means3D,
                                                   const float *shs, const float *colors_precomp, const float *opacities,
                                                   const float *scales, const float *rotations, const float *cov3D_precomp,
                                                   void *geom_ws, void *binning_ws, size_t cap, void *image_ws, float *out_color,
                                                   int32_t *radii, int64_t *num_rendered_host, const uint32_t *order, int order_len,
                                                   void *stream)
{
    return sg_forward_impl("sg_rasterize_forward_frames_ordered", s, fb, P, nullptr, means3D, shs, colors_precomp, opacities, scales,
                           rotations, cov3D_precomp, geom_ws, binning_ws, cap, image_ws, out_color, radii, nullptr, nullptr, nullptr,
                           0, num_rendered_host, stream, SG_AUX_NONE, nullptr, nullptr, nullptr, order, order_len);
}

extern "C" int sg_work_order_codes(int P, const float *means3D, void *ws, uint32_t *codes, void *stream)
{
    if (P < 0) return sg_failf("sg_work_order_codes: P = %d", P);
    if (P == 0) return 0;
    if (!means3D || !ws || !codes) return sg_failf("sg_work_order_codes: null pointer");
    sg_launch_morton_codes(P, means3D, (float *)ws, codes, (hipStream_t)stream);
    return sg_launched("sg_work_order_codes");
}

// ---- several avatars in one frame (include/sings_scene.h) ------------------------------------------------------------------------
// Everything of the scene is checked here, before the shared forward sees it: -> Ptot, or -1 with the error set
static long long sg_check_scene(const char *who, int K, int camera_stride, int S, const SgSceneAvatar *av)
{
    if (S < 1 || S > SG_SCENE_MAX_AVATARS) { sg_failf("%s: S = %d outside 1..%d", who, S, SG_SCENE_MAX_AVATARS); return -1; }
    if (K < 1 || K > SG_MAX_FRAMES) { sg_failf("%s: K = %d outside 1..%d", who, K, SG_MAX_FRAMES); return -1; }
    if (camera_stride != 0 && camera_stride != 1) { sg_failf("%s: camera_stride = %d, not 0 or 1", who, camera_stride); return -1; }
    if (!av) { sg_failf("%s: null pointer (avatars)", who); return -1; }
    long long total = 0;
    for (int i = 0; i < S; i++) {
        const SgSceneAvatar &a = av[i];
        if (a.P < 1) { sg_failf("%s: avatar %d: P = %d, at least one Gaussian is needed", who, i, a.P); return -1; }
        if (a.J < 1 || a.J > 64) { sg_failf("%s: avatar %d: J = %d outside 1..64", who, i, a.J); return -1; }
        if (a.rot_format != SG_ROT_CANON_MATRIX && a.rot_format != SG_ROT_CANON_6D) {
            sg_failf("%s: avatar %d: unknown rot_format %d", who, i, a.rot_format); return -1;
        }
        if (a.reserved != 0) { sg_failf("%s: avatar %d: reserved = %d, must be 0", who, i, a.reserved); return -1; }
        const int e = (a.ext_trans != nullptr) + (a.ext_rot != nullptr) + (a.ext_scale != nullptr);
        if (e != 0 && e != 3) { sg_failf("%s: avatar %d: ext_trans / ext_rot / ext_scale must be all or none", who, i); return -1; }
        if (!a.xyz_canon || !a.lbs_weights || !a.scales || !a.opacities || !a.shs || !a.A) {
            sg_failf("%s: avatar %d: null pointer", who, i); return -1;
        }
        total += a.P;
    }
    if (total > 0x7fffffffll) { sg_failf("%s: %lld Gaussians in the scene, at most 2^31 - 1", who, total); return -1; }
    return total;
}

static int sg_scene_impl(const char *who, const SgRasterSettings *s, int K, int camera_stride, int S, const SgSceneAvatar *avatars,
                         void *geom_ws, void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                         float *posed_xyz, float *posed_rotq, float *posed_scales, int64_t *num_rendered_host, void *stream,
                         SgAux aux, void *aux_ws, float *out_depth, float *out_alpha)
{
    const long long P = sg_check_scene(who, K, camera_stride, S, avatars);
    if (P < 0) return 1;
    const SgFrameBatch fb = { K, camera_stride, 0, 0 };
    return sg_forward_impl(who, s, &fb, (int)P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, geom_ws,
                           binning_ws, cap, image_ws, out_color, radii, posed_xyz, posed_rotq, posed_scales, 0, num_rendered_host,
                           stream, aux, aux_ws, out_depth, out_alpha, nullptr, 0, avatars, S);
}

extern "C" int sg_scene_forward_frames(const SgRasterSettings *s, int K, int camera_stride, int S, const SgSceneAvatar *avatars,
                                       void *geom_ws, void *binning_ws, size_t cap, void *image_ws, float *out_color, int32_t *radii,
                                       float *posed_xyz, float *posed_rotq, float *posed_scales, int64_t *num_rendered_host,
                                       void *stream)
{
    return sg_scene_impl("sg_scene_forward_frames", s, K, camera_stride, S, avatars, geom_ws, binning_ws, cap, image_ws, out_color,
                         radii, posed_xyz, posed_rotq, posed_scales, num_rendered_host, stream, SG_AUX_NONE, nullptr, nullptr, nullptr);
}

extern "C" int sg_scene_forward_frames_aux(const SgRasterSettings *s, int K, int camera_stride, int S, const SgSceneAvatar *avatars,
                                           void *geom_ws, void *binning_ws, size_t cap, void *image_ws, float *out_color,
                                           int32_t *radii, float *posed_xyz, float *posed_rotq, float *posed_scales,
                                           int64_t *num_rendered_host, void *aux_ws, float *out_depth, float *out_alpha, void *stream)
{
    return sg_scene_impl("sg_scene_forward_frames_aux", s, K, camera_stride, S, avatars, geom_ws, binning_ws, cap, image_ws,
                         out_color, radii, posed_xyz, posed_rotq, posed_scales, num_rendered_host, stream, SG_AUX_FRAMES, aux_ws,
                         out_depth, out_alpha);
}
