// extern "C" boundary of libsings_hip.so (see include/sings_hip.h for the contract and the
// reference interfaces each entry point replaces).
#include "sg_common.h"

#include <chrono>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <string.h>
#include <utility>
#include <vector>

static thread_local char g_err[512] = "";

static int sg_fail(const char *what, hipError_t e)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, e == hipSuccess ? "invalid argument" : hipGetErrorString(e));
    return 1;
}

// sg_fail of an argument error whose text is formatted (the entry point's name first: "%s: ...", who)
static int sg_failf(const char *fmt, ...)
{
    char msg[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return sg_fail(msg, hipSuccess);
}

#define SG_CHECK_LAST(what, s, st)                                           \
    do {                                                                     \
        hipError_t e_ = hipGetLastError();                                   \
        if (e_ != hipSuccess) return sg_fail(what, e_);                      \
        if ((s)->debug) {                                                    \
            e_ = hipStreamSynchronize(st);                                   \
            if (e_ != hipSuccess) return sg_fail(what, e_);                  \
        }                                                                    \
    } while (0)

extern "C" const char *sg_version(void) { return "sings_hip 0.8 (gfx950, abi 8)"; }
extern "C" int sg_abi_version(void) { return SG_ABI_VERSION; }
extern "C" const char *sg_last_error(void) { return g_err; }
int sg_set_error(const char *what, hipError_t e) { return sg_fail(what, e); }

extern "C" int sg_layout(int P, int width, int height, size_t cap, SgLayout *L)
{
    if (!L || P < 0 || width <= 0 || height <= 0) return sg_fail("sg_layout", hipSuccess);
    const size_t gx = (width + SG_TILE - 1) / SG_TILE, gy = (height + SG_TILE - 1) / SG_TILE, T = gx * gy;
    if (T >= SG_MAX_TILES) return sg_fail("sg_layout: image has 2^20 tiles or more (work items pack the tile id into 20 bits)", hipSuccess);
    const size_t Pn = P > 0 ? P : 1, hw = (size_t)width * height;
    size_t o = 0;
    // ONE 64-B line per Gaussian: (recA, recB, recC, pad) -- the composite kernels gather the three vectors of a list entry, and as
    // three arrays that was three 64-B lines of HBM / L2 traffic per entry (3 x 780 k x 64 B = 150 of the 170 MB the backward
    // composite moved at cfg3)
    L->geom_recA = o; L->geom_recB = o + 16; L->geom_recC = o + 32; o = sg_align(o + Pn * SG_REC_STRIDE * 16);
    L->geom_depth = o; o = sg_align(o + Pn * 4);
    L->geom_flags = o; o = sg_align(o + Pn * 4);
    L->geom_slot = o; o = sg_align(o + Pn * 8);
    L->geom_bytes = o;
    o = 0;
    L->bin_header = o; o = sg_align(o + 256);
    L->bin_tile_count = o; o = sg_align(o + sg_ctr_count((uint32_t)gx, (uint32_t)gy) * 4);
    L->bin_ranges = o; o = sg_align(o + T * 8);
    L->bin_cursor = o; o = sg_align(o + T * 4);
    L->bin_pair_keys = o; o = sg_align(o + (cap + 1) * 8);
    L->bin_point_list = o; o = sg_align(o + (cap + 1) * 4);
    L->bin_point_keys = o; o = sg_align(o + (cap + 1) * 8);
    L->bin_pair_gid = o; o = sg_align(o + (cap + 1) * 4);
    L->bin_pair_tile = o; o = sg_align(o + (cap + 1) * 4);
    L->bin_pair_local = o; o = sg_align(o + (cap + 1) * 4);
    L->bin_sort_items = o; o = sg_align(o + (size_t)sg_sort_items_cap(T, cap) * 16);
    L->bin_rank_items = o; o = sg_align(o + (size_t)sg_rank_items_cap(cap) * 8);
    L->bin_items = o; o = sg_align(o + (size_t)sg_items_cap(T, cap) * 4);
    L->bin_ck_start = o; o = sg_align(o + T * 4);
    L->bin_plan = o; o = sg_align(o + T * 16);
    L->bin_pair_mask = o; o = sg_align(o + 4 * (size_t)sg_mask_plane(cap));     // four planes: sg_split_long
    L->bin_item_w = o; o = sg_align(o + (size_t)sg_items_cap(T, cap) * 4);       // backward work-item weights
    L->bin_item_perm = o; o = sg_align(o + (size_t)sg_items_cap(T, cap) * 4);
    L->bin_rec_valid = o; o = sg_align(o + cap + 16);                                // one byte per gradient record (few-tile frames)
    L->bin_tile_keys = o; o = sg_align(o + T * (sg_lds_hist((int)gx, (int)gy) ? (size_t)SG_TILE_ROW_LONG : (size_t)SG_TILE_KEY_PITCH) * 8);     // direct binning (sg_key_pitch)
    L->bin_bytes = o;
    o = 0;
    L->img_final_T = o; o = sg_align(o + hw * 4);
    L->img_n_contrib = o; o = sg_align(o + hw * 4);
    L->img_ckpt = o; o = sg_align(o + (size_t)sg_ckpt_cap(cap) * (256 * 16));
    L->img_bytes = o;
    L->bwd_bytes = sg_rec_bytes(cap);
    return 0;
}

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

extern "C" int sg_signal_alloc(int slots, void **host_out, void **device_out)
{
    if (slots <= 0 || !host_out || !device_out) return sg_fail("sg_signal_alloc", hipSuccess);
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, (size_t)slots * 8, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) { if (h) (void)hipHostFree(h); return sg_fail("sg_signal_alloc", e); }
    memset(h, 0, (size_t)slots * 8);
    *host_out = h; *device_out = d;
    return 0;
}
extern "C" int sg_signal_free(void *host)
{
    if (!host) return 0;
    hipError_t e = hipHostFree(host);
    return e == hipSuccess ? 0 : sg_fail("sg_signal_free", e);
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

extern "C" int sg_frames_layout(int P, int width, int height, size_t cap, int K, SgLayout *one, size_t *geom_bytes, size_t *binning_bytes,
                                size_t *image_bytes, size_t *bwd_bytes)
{
    SgLayout L;
    if (K < 1 || K > SG_MAX_FRAMES) return sg_fail("sg_frames_layout: K must be 1..16", hipSuccess);
    if (sg_layout(P, width, height, cap, &L)) return 1;
    if (one) *one = L;
    if (geom_bytes) *geom_bytes = L.geom_bytes * K;
    if (binning_bytes) *binning_bytes = L.bin_bytes * K;
    if (image_bytes) *image_bytes = L.img_bytes * K;
    if (bwd_bytes) *bwd_bytes = L.bwd_bytes * K + sg_a9_bytes(P, K);      // (+ the record sums [K][P][12] of the K-camera backward)
    return 0;
}

// the K pair counts for the caller: one strided copy of (R, flags) of every frame's header behind the forward, then a wait
static int sg_read_counts(const void *binning_ws, size_t bin_stride, int K, int64_t *num_rendered_host, void *stream)
{
    uint32_t r[2 * SG_MAX_FRAMES];
    hipError_t e = hipMemcpy2DAsync(r, 8, binning_ws, bin_stride ? bin_stride : 8, 8, (size_t)K, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return sg_fail("sg_read_num_rendered", e);
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

// K consecutive single-view aux workspaces (frame f's at + f sg_aux_bytes); `null_msg`: the error of a null aux_bytes
static int sg_aux_layout_k(int P, int width, int height, size_t cap, int K, size_t *aux_bytes, const char *null_msg)
{
    SgLayout L;
    if (K < 1 || K > SG_MAX_FRAMES) return sg_fail("sg_frames_aux_layout: K must be 1..16", hipSuccess);
    if (!aux_bytes) return sg_fail(null_msg, hipSuccess);
    if (sg_layout(P, width, height, cap, &L)) return 1;          // (the same size checks)
    *aux_bytes = sg_aux_bytes(cap) * (size_t)K;
    return 0;
}
extern "C" int sg_aux_layout(int P, int width, int height, size_t cap, size_t *aux_bytes)
{
    return sg_aux_layout_k(P, width, height, cap, 1, aux_bytes, "sg_aux_layout");
}
extern "C" int sg_frames_aux_layout(int P, int width, int height, size_t cap, int K, size_t *aux_bytes)
{
    return sg_aux_layout_k(P, width, height, cap, K, aux_bytes, "sg_frames_aux_layout: null pointer");
}

static int sg_forward_impl(const char *who, const SgRasterSettings *s, const SgFrameBatch *fb, int P, const SgSkinInputs *skin,
                           const float *means3D, const float *shs, const float *colors_precomp, const float *opacities,
                           const float *scales, const float *rotations, const float *cov3D_precomp, void *geom_ws, void *binning_ws,
                           size_t cap, void *image_ws, float *out_color, int32_t *radii, float *posed_xyz, float *posed_rotq,
                           float *posed_scales, int write_point_keys, int64_t *num_rendered_host, void *stream,
                           SgAux aux = SG_AUX_NONE, void *aux_ws = nullptr, float *out_depth = nullptr, float *out_alpha = nullptr)
{
    hipStream_t st = (hipStream_t)stream;
    SgCam c;
    if (aux && !aux_ws) return sg_failf("%s: null pointer (aux_ws)", who);
    if (sg_make_cam(s, &c)) return sg_failf("%s: bad settings", who);
    if (aux) {
        if (sg_aux_flags(who, c.flags, aux == SG_AUX_FRAMES)) return 1;
        if (!out_depth || !out_alpha) return sg_failf("%s: null pointer (out_depth / out_alpha)", who);
    }
    if (skin) {
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
        if (skin) sg_launch_skin_fwd(c, bt, P, skin, shs, opacities, scales, g, b, cap, radii, posed_xyz, posed_rotq, posed_scales, st);
        else sg_launch_preprocess_fwd(c, bt, P, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, g, b, cap, radii, st);
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
    if (!binning_ws || !num_rendered_host) return sg_fail("sg_read_num_rendered: null pointer", hipSuccess);
    return sg_read_counts(binning_ws, 0, 1, num_rendered_host, stream);      // header words 0 (R) and 1 (bit 0: R > capacity, bit 1: long list)
}

extern "C" int sg_read_num_rendered_frames(const void *binning_ws, int P, int width, int height, size_t cap, int K,
                                           int64_t *num_rendered_host, void *stream)
{
    SgLayout L;
    if (!binning_ws || !num_rendered_host || K < 1 || K > SG_MAX_FRAMES) return sg_fail("sg_read_num_rendered_frames: bad argument", hipSuccess);
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

__global__ void sg_mark_visible_kernel(int P, const float *__restrict__ means3D, const float *__restrict__ view,
                                       uint8_t *__restrict__ present)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float x = means3D[3 * i], y = means3D[3 * i + 1], z = means3D[3 * i + 2];
    float vz = view[2] * x + view[6] * y + view[10] * z + view[14];
    present[i] = vz > 0.2f ? 1 : 0;
}

extern "C" int sg_mark_visible(int P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                               uint8_t *present, void *stream)
{
    (void)projmatrix;
    if (P <= 0) return 0;
    if (!means3D || !viewmatrix || !present) return sg_fail("sg_mark_visible: null pointer", hipSuccess);
    hipLaunchKernelGGL(sg_mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, means3D,
                       viewmatrix, present);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_mark_visible", e);
}

extern "C" size_t sg_photo_loss_ws_bytes(int width, int height)
{
    return width > 0 && height > 0 ? sg_photo_loss_ws_bytes_impl(width, height) : 0;
}

extern "C" int sg_photo_loss_frames(int K, int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                                    size_t gt_stride, const float *mask, size_t mask_stride, const float *bg, void *ws,
                                    float *pred_out, float *gt_out, float *losses, const float *upstream, float *dL_draw, void *stream)
{
    if (width <= 0 || height <= 0 || K < 1 || K > SG_MAX_FRAMES) return sg_fail("sg_photo_loss: bad image size / K not in 1..16", hipSuccess);
    if (!raw || !gt_rgb || !mask || !bg || !ws || (!losses && !dL_draw))
        return sg_fail("sg_photo_loss: null pointer", hipSuccess);
    sg_launch_photo_loss(K, width, height, l1_w, ssim_w, raw, gt_rgb, mask, bg, ws, pred_out, gt_out, losses, upstream,
                         dL_draw, gt_stride, mask_stride, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sg_fail("sg_photo_loss", e);
    return 0;
}
extern "C" int sg_photo_loss(int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                             const float *mask, const float *bg, void *ws, float *pred_out, float *gt_out,
                             float *losses, const float *upstream, float *dL_draw, void *stream)
{
    return sg_photo_loss_frames(1, width, height, l1_w, ssim_w, raw, gt_rgb, 0, mask, 0, bg, ws, pred_out, gt_out, losses, upstream,
                                dL_draw, stream);
}

extern "C" int sg_photo_loss_backward_frames(int K, int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                                             size_t gt_stride, const float *mask, size_t mask_stride, const float *bg, const void *ws,
                                             const float *upstream, int upstream_stride, float *dL_draw, void *stream)
{
    if (K < 1 || K > SG_MAX_FRAMES || width <= 0 || height <= 0 || !raw || !gt_rgb || !mask || !bg || !ws || !dL_draw)
        return sg_fail("sg_photo_loss_backward_frames: bad arguments (K in 1..16, no null pointers)", hipSuccess);
    if (upstream_stride != 0 && upstream_stride != 2) return sg_fail("sg_photo_loss_backward_frames: upstream_stride must be 0 or 2", hipSuccess);
    sg_launch_photo_loss_bwd(K, width, height, l1_w, ssim_w, raw, gt_rgb, mask, bg, ws, upstream, dL_draw, gt_stride, mask_stride,
                             (hipStream_t)stream, upstream ? upstream_stride : 0);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_photo_loss_backward_frames", e);
}
extern "C" int sg_photo_loss_backward(int width, int height, float l1_w, float ssim_w, const float *raw, const float *gt_rgb,
                                      const float *mask, const float *bg, const void *ws, const float *upstream,
                                      float *dL_draw, void *stream)
{
    if (width <= 0 || height <= 0) return sg_fail("sg_photo_loss_backward: bad image size", hipSuccess);
    if (!raw || !gt_rgb || !mask || !bg || !ws || !dL_draw) return sg_fail("sg_photo_loss_backward: null pointer", hipSuccess);
    sg_launch_photo_loss_bwd(1, width, height, l1_w, ssim_w, raw, gt_rgb, mask, bg, ws, upstream, dL_draw, 0, 0, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sg_fail("sg_photo_loss_backward", e);
    return 0;
}

// ---- stand-alone lbs_extra (a9)
extern "C" int sg_lbs_forward(int P, int J, const float *lbs_weights, const float *A, const float *v, float *T_out,
                              float *verts_out, void *stream)
{
    if (P <= 0 || J < 1 || J > 64 || !lbs_weights || !A || !v || !verts_out)
        return sg_fail("sg_lbs_forward: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_lbs_fwd(P, J, lbs_weights, A, v, T_out, verts_out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_lbs_forward", e);
}
extern "C" int sg_lbs_backward(int P, int J, const float *lbs_weights, const float *A, const float *v, const float *dT,
                               const float *dverts, float *ws, float *dv, float *dA, void *stream)
{
    if (P <= 0 || J < 1 || J > 64 || !lbs_weights || !A || !v || !ws || !dA || (!dT && !dverts))
        return sg_fail("sg_lbs_backward: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_lbs_bwd(P, J, lbs_weights, A, v, dT, dverts, ws, dv, dA, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_lbs_backward", e);
}

// ---- SMPL kinematic chain (a10)
extern "C" int sg_joint_transforms(int B, int J, const float *pose, const float *joints_rest, const int32_t *parents,
                                   const float *post, float *A_out, void *stream)
{
    if (B <= 0 || J < 1 || J > 64 || !pose || !joints_rest || !parents || !A_out)
        return sg_fail("sg_joint_transforms: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_joint_transforms(B, J, pose, joints_rest, (const int *)parents, post, nullptr, A_out, nullptr, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_joint_transforms", e);
}
extern "C" int sg_joint_transforms_backward(int B, int J, const float *pose, const float *joints_rest, const int32_t *parents,
                                            const float *post, const float *dA, float *dpose, float *djoints, void *stream)
{
    if (B <= 0 || J < 1 || J > 64 || !pose || !joints_rest || !parents || !dA || !dpose)
        return sg_fail("sg_joint_transforms_backward: bad argument (1 <= J <= 64)", hipSuccess);
    sg_launch_joint_transforms(B, J, pose, joints_rest, (const int *)parents, post, dA, dpose, djoints, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_joint_transforms_backward", e);
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
        return sg_fail("sg_pose_transforms: bad argument (1 <= J <= 64, 0 <= NBu <= 23, NBu < J; tail_pose for J - 1 - NBu joints; "
                       "transl and transl_out together)", hipSuccess);
    sg_launch_pose_transforms(K, F, J, NBu, (const int *)frame_idx, global_orient, body_pose, tail_pose, transl, joints_rest,
                              (const int *)parents, post, A_out, aa_out, transl_out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_pose_transforms", e);
}
extern "C" int sg_pose_transforms_backward(int K, int F, int J, int NBu, const int32_t *frame_idx, const float *global_orient,
                                           const float *body_pose, const float *aa, const float *joints_rest, const int32_t *parents,
                                           const float *post, const float *dA, const float *d_transl_rows, float *d_global_orient,
                                           float *d_body_pose, float *d_transl, void *stream)
{
    if (!sg_pose_shape_ok(K, F, J, NBu) || !frame_idx || !global_orient || !body_pose || !aa || !joints_rest || !parents || !dA ||
        !d_global_orient || !d_body_pose || (d_transl_rows == nullptr) != (d_transl == nullptr))
        return sg_fail("sg_pose_transforms_backward: bad argument (1 <= J <= 64, 0 <= NBu <= 23, NBu < J; d_transl_rows and d_transl "
                       "together)", hipSuccess);
    sg_launch_pose_transforms_bwd(K, F, J, NBu, (const int *)frame_idx, global_orient, body_pose, aa, joints_rest, (const int *)parents,
                                  post, dA, d_transl_rows, d_global_orient, d_body_pose, d_transl, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_pose_transforms_backward", e);
}

// ---- stand-alone matrix_to_quaternion (a11)
extern "C" int sg_matrix_to_quaternion(int N, const float *matrices, float *quaternions, void *stream)
{
    if (N <= 0 || !matrices || !quaternions) return sg_fail("sg_matrix_to_quaternion: bad argument", hipSuccess);
    sg_launch_m2q(N, matrices, nullptr, quaternions, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_matrix_to_quaternion", e);
}
extern "C" int sg_matrix_to_quaternion_backward(int N, const float *matrices, const float *dq, float *dmatrices, void *stream)
{
    if (N <= 0 || !matrices || !dq || !dmatrices) return sg_fail("sg_matrix_to_quaternion_backward: bad argument", hipSuccess);
    sg_launch_m2q(N, matrices, dq, dmatrices, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_matrix_to_quaternion_backward", e);
}

// ---- decoder layers as fused MFMA kernels (f3)
extern "C" int sg_linear_forward(int N, int Cin, int Cout, int act, const float *x, const float *W, const float *bias,
                                 const float *row_offset, float *z_out, float *h_out, void *stream)
{
    if (N <= 0 || !x || !W || !h_out || act < 0 || act > 3) return sg_fail("sg_linear_forward: bad argument", hipSuccess);
    if (sg_launch_linear_fwd(N, Cin, Cout, act, x, W, bias, row_offset, z_out, h_out, (hipStream_t)stream))
        return sg_fail("sg_linear_forward: 1 <= Cin, Cout <= 128", hipSuccess);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_linear_forward", e);
}
static int sg_linear_backward_impl(const char *who, int N, int Cin, int Cout, int act, const float *z, const float *row_offset,
                                   const float *dh, const float *W, float *dz_out, float *dx_out, void *stream, int accumulate)
{
    if (N <= 0 || !dh || !W || !dx_out || act < 0 || act > 3 || (act != 0 && !z)) return sg_fail(who, hipSuccess);
    if (accumulate && (Cin & 31)) return sg_fail("sg_linear_backward_accumulate: Cin must be a multiple of 32", hipSuccess);
    if (sg_launch_linear_bwd(N, Cin, Cout, act, z, row_offset, dh, W, dz_out, dx_out, (hipStream_t)stream, accumulate))
        return sg_fail("sg_linear_backward: 1 <= Cin, Cout <= 128 (accumulate: N Cin < 2^29)", hipSuccess);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail(who, e);
}
extern "C" int sg_linear_backward(int N, int Cin, int Cout, int act, const float *z, const float *row_offset, const float *dh,
                                  const float *W, float *dz_out, float *dx_out, void *stream)
{
    return sg_linear_backward_impl("sg_linear_backward: bad argument", N, Cin, Cout, act, z, row_offset, dh, W, dz_out, dx_out, stream, 0);
}
// (declared here, not in sg_common.h: that header is one of the sources the committed PMC profiles are keyed on)
int sg_launch_linear_bwd_fan(int N, int Cin, int Cout, int act, const float *z, const float *dh, const float *W, float *dz_out,
                             float *dx_out, const SgLinearSide *side, hipStream_t st);
extern "C" int sg_linear_backward_fan(int N, int Cin, int Cout, int act, const float *z, const float *dh, const float *W,
                                      float *dz_out, float *dx_out, const SgLinearSide side[2], void *stream)
{
    if (N <= 0 || !dh || !W || !dx_out || !side || act < 0 || act > 3 || (act != 0 && !z))
        return sg_fail("sg_linear_backward_fan: bad argument", hipSuccess);
    for (int i = 0; i < 2; i++) {
        const SgLinearSide &s = side[i];
        if (s.cout < 0 || s.cout > 16 || (s.cout && (!s.dh || !s.W || (s.act != 0 && s.act != 2) || (s.act == 2 && !s.aux))))
            return sg_fail("sg_linear_backward_fan: a head needs dh, W, act 0 | 2 (with aux)", hipSuccess);
    }
    if (side[0].cout + side[1].cout == 0) return sg_fail("sg_linear_backward_fan: no head (use sg_linear_backward)", hipSuccess);
    if (sg_launch_linear_bwd_fan(N, Cin, Cout, act, z, dh, W, dz_out, dx_out, side, (hipStream_t)stream))
        return sg_fail("sg_linear_backward_fan: Cin a multiple of 32 <= 128, Cout a multiple of 4 <= 128, heads <= 16 columns", hipSuccess);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_linear_backward_fan", e);
}
extern "C" int sg_linear_backward_accumulate(int N, int Cin, int Cout, int act, const float *z, const float *row_offset,
                                             const float *dh, const float *W, float *dz_out, float *dx_out, void *stream)
{
    return sg_linear_backward_impl("sg_linear_backward_accumulate: bad argument", N, Cin, Cout, act, z, row_offset, dh, W, dz_out, dx_out,
                                   stream, 1);
}

// ---- the other rotation conversions (a11)
extern "C" int sg_rotation_convert(int op, int N, const float *in, float *out, void *stream)
{
    if (N <= 0 || !in || !out) return sg_fail("sg_rotation_convert: bad argument", hipSuccess);
    if (sg_launch_rot_map(op, N, in, nullptr, out, (hipStream_t)stream)) return sg_fail("sg_rotation_convert: unknown op", hipSuccess);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_rotation_convert", e);
}
extern "C" int sg_rotation_convert_backward(int op, int N, const float *in, const float *d_out, float *d_in, void *stream)
{
    if (N <= 0 || !in || !d_out || !d_in) return sg_fail("sg_rotation_convert_backward: bad argument", hipSuccess);
    if (sg_launch_rot_map(op, N, in, d_out, d_in, (hipStream_t)stream)) return sg_fail("sg_rotation_convert_backward: unknown op", hipSuccess);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_rotation_convert_backward", e);
}
extern "C" int sg_quaternion_multiply(int N, const float *a, const float *b, float *out, void *stream)
{
    if (N <= 0 || !a || !b || !out) return sg_fail("sg_quaternion_multiply: bad argument", hipSuccess);
    sg_launch_qmul(N, a, b, nullptr, out, nullptr, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_quaternion_multiply", e);
}
extern "C" int sg_quaternion_multiply_backward(int N, const float *a, const float *b, const float *d_out, float *da, float *db,
                                               void *stream)
{
    if (N <= 0 || !a || !b || !d_out || !da || !db) return sg_fail("sg_quaternion_multiply_backward: bad argument", hipSuccess);
    sg_launch_qmul(N, a, b, d_out, da, db, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_quaternion_multiply_backward", e);
}

// ---- attribute decode (f3)
extern "C" size_t sg_triplane_ws_bytes(const SgTriplane *tp) { return sg_tp_check(tp) ? 0 : sg_triplane_ws_bytes_impl(tp); }
extern "C" size_t sg_triplane_bwd_ws_bytes(const SgTriplane *tp, int N)
{
    return sg_tp_check(tp) || N <= 0 ? 0 : sg_triplane_bwd_ws_bytes_impl(tp, N);
}
extern "C" int sg_triplane_forward(const SgTriplane *tp, int N, const float *xyz, void *ws, float *feats, void *stream)
{
    if (sg_tp_check(tp)) return sg_fail("sg_triplane_forward: bad plane description (feat must be 32, 1..4 scales)", hipSuccess);
    if (N <= 0 || !xyz || !ws || !feats) return sg_fail("sg_triplane_forward: bad argument", hipSuccess);
    sg_launch_triplane_fwd(tp, N, xyz, ws, feats, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_triplane_forward", e);
}
extern "C" int sg_triplane_backward(const SgTriplane *tp, int N, const float *xyz, void *ws, const float *dfeats,
                                    float *const dplanes[4][3], float *dxyz, void *stream)
{
    if (sg_tp_check(tp)) return sg_fail("sg_triplane_backward: bad plane description", hipSuccess);
    if (N <= 0 || !xyz || !ws || !dfeats || !dplanes) return sg_fail("sg_triplane_backward: bad argument", hipSuccess);
    if (sg_launch_triplane_bwd(tp, N, xyz, ws, dfeats, dplanes, dxyz, (hipStream_t)stream))
        return sg_fail("sg_triplane_backward: memset", hipGetLastError());
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_triplane_backward", e);
}
extern "C" int sg_triplane_backward_prepare(const SgTriplane *tp, int N, const float *xyz, void *ws, void *stream)
{
    if (sg_tp_check(tp)) return sg_fail("sg_triplane_backward_prepare: bad plane description", hipSuccess);
    if (N <= 0 || !xyz || !ws) return sg_fail("sg_triplane_backward_prepare: bad argument", hipSuccess);
    sg_launch_triplane_bwd_prepare(tp, N, xyz, ws, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_triplane_backward_prepare", e);
}
extern "C" int sg_triplane_backward_prepared(const SgTriplane *tp, int N, const float *xyz, void *ws, const float *dfeats,
                                             float *const dplanes[4][3], float *dxyz, void *stream)
{
    if (sg_tp_check(tp)) return sg_fail("sg_triplane_backward_prepared: bad plane description", hipSuccess);
    if (N <= 0 || !xyz || !ws || !dfeats || !dplanes) return sg_fail("sg_triplane_backward_prepared: bad argument", hipSuccess);
    sg_launch_triplane_bwd_run(tp, N, xyz, ws, dfeats, dplanes, dxyz, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_triplane_backward_prepared", e);
}
// (declared here, not in sg_common.h: that header is one of the sources the committed PMC profiles are keyed on)
void sg_launch_scales_head(int N, const float *z, float *scales, float *aux, const float *dscales, const float *daux, float *dz,
                           hipStream_t st);
extern "C" int sg_scales_head_forward(int N, const float *z, float *scales_out, float *aux_out, void *stream)
{
    if (N <= 0 || !z || !scales_out || !aux_out) return sg_fail("sg_scales_head_forward: bad argument", hipSuccess);
    sg_launch_scales_head(N, z, scales_out, aux_out, nullptr, nullptr, nullptr, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_scales_head_forward", e);
}
extern "C" int sg_scales_head_backward(int N, const float *z, const float *dscales, const float *daux, float *dz, void *stream)
{
    if (N <= 0 || !z || !dz || (!dscales && !daux)) return sg_fail("sg_scales_head_backward: bad argument", hipSuccess);
    sg_launch_scales_head(N, z, nullptr, nullptr, dscales, daux, dz, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_scales_head_backward", e);
}
extern "C" size_t sg_bias_act_ws_bytes(int N, int C) { return sg_bias_act_ws_bytes_impl(N > 0 ? N : 1, C > 0 ? C : 1); }
extern "C" int sg_bias_act_forward(int N, int C, int act, const float *y, const float *bias, const float *row_offset,
                                   float *z_out, float *h_out, void *stream)
{
    if (N <= 0 || C <= 0 || act < 0 || act > 3 || !y || !h_out) return sg_fail("sg_bias_act_forward: bad argument", hipSuccess);
    sg_launch_bias_act_fwd(N, C, act, y, bias, row_offset, z_out, h_out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_bias_act_forward", e);
}
extern "C" int sg_bias_act_backward(int N, int C, int act, const float *z, const float *row_offset, const float *dh,
                                    void *ws, float *dz, float *dbias, void *stream)
{
    if (N <= 0 || C <= 0 || C > 128 || act < 0 || act > 3 || !z || !dh || !ws || !dz)
        return sg_fail("sg_bias_act_backward: bad argument (C <= 128)", hipSuccess);
    sg_launch_bias_act_bwd(N, C, act, z, row_offset, dh, ws, dz, dbias, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_bias_act_backward", e);
}

extern "C" size_t sg_weight_grad_ws_bytes(int N, int Cout, int Cin)
{
    return N > 0 && Cout > 0 && Cin > 0 ? sg_weight_grad_ws_bytes_impl(N, Cout, Cin) : 0;
}
extern "C" int sg_weight_grad(int N, int Cout, int Cin, const float *dz, const float *x, void *ws, float *dW, float *db,
                              void *stream)
{
    if (N <= 0 || !dz || !x || !ws || !dW) return sg_fail("sg_weight_grad: bad argument", hipSuccess);
    if (sg_launch_weight_grad(N, Cout, Cin, dz, x, ws, dW, db, (hipStream_t)stream))
        return sg_fail("sg_weight_grad: Cin must be 32/64/96/128 and Cout <= 128", hipSuccess);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_weight_grad", e);
}

// ---- regularisers (f1)
extern "C" size_t sg_reg_ws_bytes(int rows) { return sg_reg_ws_bytes_impl(rows > 0 ? rows : 1); }
extern "C" size_t sg_knn_ws_bytes(int N) { return sg_knn_ws_bytes_impl(N > 0 ? N : 1); }

#define SG_RET_LAST(what)                                     \
    do {                                                      \
        hipError_t e_ = hipGetLastError();                    \
        if (e_ != hipSuccess) return sg_fail(what, e_);       \
        return 0;                                             \
    } while (0)

extern "C" int sg_region_laplacian(int V, int C, const float *x, const int *row_ptr, const int *col,
                                   const float *deg_inv, const float *vscale, void *ws, float *g_ws, float *loss,
                                   const float *upstream, float *dL_dx, void *stream)
{
    if (V <= 0 || C <= 0 || !x || !row_ptr || !col || !deg_inv || !vscale || !ws || !g_ws || (!loss && !dL_dx))
        return sg_fail("sg_region_laplacian: bad argument", hipSuccess);
    sg_launch_region_laplacian(V, C, x, row_ptr, col, deg_inv, vscale, ws, g_ws, loss, upstream, dL_dx, (hipStream_t)stream);
    SG_RET_LAST("sg_region_laplacian");
}

// (declared here, not in sg_common.h: that header is one of the sources the committed PMC profiles are keyed on)
void sg_launch_rows_laplacian(int R, int V, int C, const float *x, const int *row_ptr, const int *col, const float *val,
                              const float *rscale, const int *t_row_ptr, const int *t_row, const float *t_val, void *ws, float *g_ws,
                              float *loss, const float *upstream, float *dL_dx, hipStream_t st);
extern "C" int sg_rows_laplacian(int R, int V, int C, const float *x, const int *row_ptr, const int *col, const float *val,
                                 const float *rscale, const int *t_row_ptr, const int *t_row, const float *t_val, void *ws,
                                 float *g_ws, float *loss, const float *upstream, float *dL_dx, void *stream)
{
    if (R <= 0 || V <= 0 || C <= 0 || !x || !row_ptr || !col || !val || !rscale || !ws || !g_ws || (!loss && !dL_dx) ||
        (dL_dx && (!t_row_ptr || !t_row || !t_val)))
        return sg_fail("sg_rows_laplacian: bad argument", hipSuccess);
    sg_launch_rows_laplacian(R, V, C, x, row_ptr, col, val, rscale, t_row_ptr, t_row, t_val, ws, g_ws, loss, upstream, dL_dx,
                             (hipStream_t)stream);
    SG_RET_LAST("sg_rows_laplacian");
}

extern "C" int sg_mesh_edge_loss(int V, int E, const float *x, const int *row_ptr, const int *col, void *ws,
                                 float *loss, const float *upstream, float *dL_dx, void *stream)
{
    if (V <= 0 || E <= 0 || !x || !row_ptr || !col || !ws || (!loss && !dL_dx))
        return sg_fail("sg_mesh_edge_loss: bad argument", hipSuccess);
    sg_launch_mesh_edge(V, E, x, row_ptr, col, ws, loss, upstream, dL_dx, (hipStream_t)stream);
    SG_RET_LAST("sg_mesh_edge_loss");
}

extern "C" int sg_l2norm_reg(int N, const float *xyz_offsets, const float *scales, const float *opacity,
                             const float *lambdas6, void *ws, float *loss, const float *upstream, float *d_offsets,
                             float *d_scales, float *d_opacity, void *stream)
{
    if (N <= 0 || !lambdas6 || !ws || (!xyz_offsets && !scales && !opacity))
        return sg_fail("sg_l2norm_reg: bad argument", hipSuccess);
    sg_launch_l2norm(N, xyz_offsets, scales, opacity, lambdas6, ws, loss, upstream, d_offsets, d_scales, d_opacity,
                     (hipStream_t)stream);
    SG_RET_LAST("sg_l2norm_reg");
}

extern "C" int sg_gaussian_edge_loss(int N, int K, const float *xyz, const float *scales, void *ws,
                                     float *mean_edge_out, float *loss, const float *upstream, float *d_scales,
                                     void *stream)
{
    if (N < K || !xyz || !ws) return sg_fail("sg_gaussian_edge_loss: bad argument (need N >= K)", hipSuccess);
    if (sg_launch_knn_edge(N, K, xyz, scales, ws, mean_edge_out, loss, upstream, d_scales, (hipStream_t)stream))
        return sg_fail("sg_gaussian_edge_loss: K must be 5, 9 or 17", hipSuccess);
    SG_RET_LAST("sg_gaussian_edge_loss");
}

extern "C" int sg_gaussian_edge_prepare(int N, const float *xyz, void *ws, void *stream)
{
    if (N < 1 || !xyz || !ws) return sg_fail("sg_gaussian_edge_prepare: bad argument", hipSuccess);
    sg_launch_knn_prepare(N, xyz, ws, (hipStream_t)stream);
    SG_RET_LAST("sg_gaussian_edge_prepare");
}

extern "C" int sg_gaussian_edge_finish(int N, int K, const float *scales, void *ws, float *mean_edge_out, float *loss,
                                       const float *upstream, float *d_scales, void *stream)
{
    if (N < K || !ws) return sg_fail("sg_gaussian_edge_finish: bad argument (need N >= K)", hipSuccess);
    if (sg_launch_knn_finish(N, K, scales, ws, mean_edge_out, loss, upstream, d_scales, (hipStream_t)stream))
        return sg_fail("sg_gaussian_edge_finish: K must be 5, 9 or 17", hipSuccess);
    SG_RET_LAST("sg_gaussian_edge_finish");
}

// ---- per-kernel event timing ------------------------------------------------------------
__global__ void __launch_bounds__(256) sg_zero_kernel(uint32_t *__restrict__ p, size_t words)
{
    // 16-B stores over the aligned middle, 4-B stores at the ragged ends
    const size_t head = ((16 - ((uintptr_t)p & 15)) & 15) >> 2;
    const size_t h = head < words ? head : words, v4 = (words - h) >> 2, tail = h + 4 * v4;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)gridDim.x * 256;
    if (i < h) p[i] = 0u;
    uint4 *q = (uint4 *)(p + h);
    for (size_t k = i; k < v4; k += n) q[k] = make_uint4(0u, 0u, 0u, 0u);
    if (tail + i < words) p[tail + i] = 0u;
}
void sg_zero_async(void *p, size_t bytes, hipStream_t st)
{
    const size_t words = bytes >> 2;
    if (!words) return;
    size_t blocks = (words / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(sg_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (uint32_t *)p, words);
}

// ---- measurement: the denominator of the HBM roofline ----------------------------------------------------------------
// A plain 16-byte-per-lane copy (grid-stride, nothing else): what the box's HBM sustains for a read + a write stream.  bench.py
// times it over >= 1 GiB and quotes `roofline.peak` from it ("float4-copy bandwidth measured on the same box").
// Four independent 16-byte loads per lane, all issued before the first store (a grid-stride loop of ONE load -> store per trip
// keeps one request in flight per wave and measured 4.6 TB/s on the part the guide quotes at 6.3); NT: non-temporal loads and
// stores (a once-touched stream need not displace L2 / Infinity Cache lines).  bench.py takes the better of the two.
typedef float sg_f32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__global__ void __launch_bounds__(256) sg_copy_probe_kernel(sg_f32x4 *__restrict__ dst, const sg_f32x4 *__restrict__ src, size_t n)
{
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    sg_f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const size_t i = base + 256 * u;
        if (i < n) v[u] = NT ? __builtin_nontemporal_load(src + i) : src[i];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const size_t i = base + 256 * u;
        if (i < n) { if (NT) __builtin_nontemporal_store(v[u], dst + i); else dst[i] = v[u]; }
    }
}
extern "C" int sg_copy_probe(void *dst, const void *src, size_t bytes, int non_temporal, void *stream)
{
    if (!dst || !src || (bytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15))
        return sg_fail("sg_copy_probe: 16-byte aligned buffers and a multiple of 16 bytes", hipSuccess);
    if (!bytes) return 0;
    const size_t n = bytes >> 4;
    const size_t blocks = (n + 1023) / 1024;
    if (blocks > 0x7fffffffull) return sg_fail("sg_copy_probe: more than 2^41 bytes", hipSuccess);
    if (non_temporal)
        hipLaunchKernelGGL(sg_copy_probe_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (sg_f32x4 *)dst, (const sg_f32x4 *)src, n);
    else
        hipLaunchKernelGGL(sg_copy_probe_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (sg_f32x4 *)dst, (const sg_f32x4 *)src, n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sg_fail("sg_copy_probe", e);
}

static bool g_prof_on = false;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_ev[SG_NUM_KERNELS];
static hipEvent_t g_prof_open[SG_NUM_KERNELS];

void sg_prof_begin(int id, hipStream_t st)
{
    if (!g_prof_on) return;
    hipEvent_t e;
    (void)hipEventCreate(&e);
    (void)hipEventRecord(e, st);
    g_prof_open[id] = e;
}
void sg_prof_end(int id, hipStream_t st)
{
    if (!g_prof_on) return;
    hipEvent_t e;
    (void)hipEventCreate(&e);
    (void)hipEventRecord(e, st);
    g_prof_ev[id].push_back(std::make_pair(g_prof_open[id], e));
}
extern "C" int sg_profile_enable(int on) { g_prof_on = on != 0; return 0; }
extern "C" int sg_profile_collect(double *total_ms, int64_t *launches, int n)
{
    if (!total_ms || !launches || n < SG_NUM_KERNELS) return sg_fail("sg_profile_collect", hipSuccess);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return sg_fail("sg_profile_collect", e);
    for (int k = 0; k < SG_NUM_KERNELS; k++) {
        for (auto &p : g_prof_ev[k]) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, p.first, p.second);
            total_ms[k] += ms; launches[k] += 1;
            (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second);
        }
        g_prof_ev[k].clear();
    }
    return 0;
}
extern "C" const char *sg_kernel_name(int id)
{
    static const char *names[SG_NUM_KERNELS] = { "sg_preprocess_fwd_kernel", "sg_photo_loss_kernels", "sg_tile_scan_kernel",
                                                 "sg_tile_scatter_kernel", "sg_tile_sort_kernel", "sg_render_fwd_kernel",
                                                 "sg_render_bwd_kernel", "sg_preprocess_bwd_kernel" };
    return id >= 0 && id < SG_NUM_KERNELS ? names[id] : "?";
}
