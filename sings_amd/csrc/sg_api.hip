// The core of the extern "C" boundary of libsings_hip.so (see include/sings_hip.h for the contract): the error state, the
// workspace layouts, the signal words, the small device helpers every module uses and the event profiler.  The rasterizer's
// entry points are in sg_api_raster.hip, the other modules' wrappers in sg_api_ops.hip.
#include "sg_host.h"

#include <string.h>
#include <utility>
#include <vector>

static thread_local char g_err[512] = "";

extern "C" const char *sg_version(void) { return "sings_hip 0.8 (gfx950, abi 8)"; }
extern "C" int sg_abi_version(void) { return SG_ABI_VERSION; }
extern "C" const char *sg_last_error(void) { return g_err; }
int sg_set_error(const char *what, hipError_t e)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, e == hipSuccess ? "invalid argument" : hipGetErrorString(e));
    return 1;
}

extern "C" int sg_layout(int P, int width, int height, size_t cap, SgLayout *L)
{
    if (!L || P < 0 || width <= 0 || height <= 0) return sg_set_error("sg_layout", hipSuccess);
    const size_t gx = (width + SG_TILE - 1) / SG_TILE, gy = (height + SG_TILE - 1) / SG_TILE, T = gx * gy;
    if (T >= SG_MAX_TILES) return sg_set_error("sg_layout: image has 2^20 tiles or more (work items pack the tile id into 20 bits)", hipSuccess);
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

extern "C" int sg_frames_layout(int P, int width, int height, size_t cap, int K, SgLayout *one, size_t *geom_bytes, size_t *binning_bytes,
                                size_t *image_bytes, size_t *bwd_bytes)
{
    SgLayout L;
    if (K < 1 || K > SG_MAX_FRAMES) return sg_set_error("sg_frames_layout: K must be 1..16", hipSuccess);
    if (sg_layout(P, width, height, cap, &L)) return 1;
    if (one) *one = L;
    if (geom_bytes) *geom_bytes = L.geom_bytes * K;
    if (binning_bytes) *binning_bytes = L.bin_bytes * K;
    if (image_bytes) *image_bytes = L.img_bytes * K;
    if (bwd_bytes) *bwd_bytes = L.bwd_bytes * K + sg_a9_bytes(P, K);      // (+ the per-frame rows of the K-camera backward)
    return 0;
}

// K consecutive single-view aux workspaces (frame f's at + f sg_aux_bytes); `null_msg`: the error of a null aux_bytes
static int sg_aux_layout_k(int P, int width, int height, size_t cap, int K, size_t *aux_bytes, const char *null_msg)
{
    SgLayout L;
    if (K < 1 || K > SG_MAX_FRAMES) return sg_set_error("sg_frames_aux_layout: K must be 1..16", hipSuccess);
    if (!aux_bytes) return sg_set_error(null_msg, hipSuccess);
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

extern "C" int sg_signal_alloc(int slots, void **host_out, void **device_out)
{
    if (slots <= 0 || !host_out || !device_out) return sg_set_error("sg_signal_alloc", hipSuccess);
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, (size_t)slots * 8, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) { if (h) (void)hipHostFree(h); return sg_set_error("sg_signal_alloc", e); }
    memset(h, 0, (size_t)slots * 8);
    *host_out = h; *device_out = d;
    return 0;
}
extern "C" int sg_signal_free(void *host)
{
    if (!host) return 0;
    hipError_t e = hipHostFree(host);
    return e == hipSuccess ? 0 : sg_set_error("sg_signal_free", e);
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
    if (!means3D || !viewmatrix || !present) return sg_set_error("sg_mark_visible: null pointer", hipSuccess);
    hipLaunchKernelGGL(sg_mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, means3D,
                       viewmatrix, present);
    return sg_launched("sg_mark_visible");
}

// ---- zeroing a workspace range without a memset node --------------------------------------------------------------
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
        return sg_set_error("sg_copy_probe: 16-byte aligned buffers and a multiple of 16 bytes", hipSuccess);
    if (!bytes) return 0;
    const size_t n = bytes >> 4;
    const size_t blocks = (n + 1023) / 1024;
    if (blocks > 0x7fffffffull) return sg_set_error("sg_copy_probe: more than 2^41 bytes", hipSuccess);
    if (non_temporal)
        hipLaunchKernelGGL(sg_copy_probe_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (sg_f32x4 *)dst, (const sg_f32x4 *)src, n);
    else
        hipLaunchKernelGGL(sg_copy_probe_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (sg_f32x4 *)dst, (const sg_f32x4 *)src, n);
    return sg_launched("sg_copy_probe");
}

// ---- per-kernel event timing ------------------------------------------------------------
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
    if (!total_ms || !launches || n < SG_NUM_KERNELS) return sg_set_error("sg_profile_collect", hipSuccess);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return sg_set_error("sg_profile_collect", e);
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
