// Validation metrics of K rendered frames: per-channel MSE / PSNR and the mean of the SSIM map, ONE pass over the image planes.
//
// Replaces, per validation frame of SinGaussianTrainer.validate (sings/rec/trainer/gs_trainer.py:577-585), the chain
//   image = clamp(rendered, 0, 1)                                 gs_renderer_single.py:96
//   image, gt = image * mask, gt * mask                           gs_trainer.py:580-582 (dataset `zju` only)
//   psnr(image, gt).mean()                                        utils/image/image.py:15-17 (per-channel mse, mean of three PSNRs)
//   ssim(image, gt).mean()                                        losses/utils.py:39-70 (unmasked, unscaled)
// -- about thirty torch kernels per frame -- by two launches for K frames:
//   sg_metrics_kernel        : the marching scheme of sg_loss.hip without its gradient half.  One WAVE per (channel, strip of 64
//                              columns, chunk of R rows), marching down the rows.  Per step it loads one row (coalesced, two rows in
//                              flight), clamps / masks it, applies the 11-tap window ACROSS lanes through a wave-private LDS row and
//                              DOWN the rows in a register ring of the last 11 row results (the row loop is unrolled by 11: static ring
//                              slots).  Five rows behind the loads the SSIM value of a row exists.  A strip loads 74 columns and emits
//                              all 64 whose window it holds; a chunk of R rows reads R + 10.  The squared difference is summed where a
//                              pixel is STAGED: the 74 loaded columns contain the strip's own 64 exactly once (lanes 5-63 of the first
//                              load, lanes 0-4 of the second), so every plane is read once -- there is no centre-row load.
//                              No workgroup barrier, no atomics.  Each lane sums in fp64 down its rows, the wave in a fixed butterfly.
//   sg_metrics_reduce_kernel : fixed-order fp64 sum of the per-wave partials of a frame -> metrics[frame][8]
// The chunking depends on W and H alone, so a frame's partials and their order -- its bits -- are the same for every K and every
// position in the batch.  Algorithmic bytes per pixel: 3 channels x (pred 4 + gt 4) = 24, + 4 with a mask.
#include "sg_common.h"
#include "sg_host.h"
#include "../../include/sings_eval.h"

#define SGM_LN SG_METRICS_STRIP_COLS      // lanes of a strip = columns it emits
#define SGM_PITCH (SGM_LN + 16)           // staged row: 64 + 10 halo columns
#define SGM_UNITS 2048                    // units (waves) ONE frame aims for: eight per CU
#define SGM_RUN 12                        // consecutive units (3 channels x 4 strips) dealt to one XCD
#define SGM_RCP(v) __builtin_amdgcn_rcpf(v)   // as sg_loss.hip: 1 ulp, far inside the fp32 noise of the window sums

static_assert(SGM_LN == 64, "a strip is one wave wide");

struct SgMetricsArgs {
    int W, H;
    float w[11];                          // the reference's fp32 window: exp(-(x-5)^2 / (2 * 1.5^2)), normalised
    size_t gt_stride, mask_stride, ws_stride;   // floats, floats, bytes between consecutive frames
    int R, nstrips, nchunks, ncell, units;      // rows per chunk, strips, chunks, strips x chunks, waves per frame (3 ncell)
    int xcd_rot;                          // frame f deals its runs of units to the XCDs starting at XCD f * xcd_rot
};

typedef float sgm_f2 __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t sgm_rsrc;

__device__ __forceinline__ float sgm_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ int sgm_clampi(int v, int hi) { return v < 0 ? 0 : (v < hi ? v : hi - 1); }
// image planes as raw buffers: descriptor and row offset in SGPRs, the lane's column offset in a VGPR that never changes
__device__ __forceinline__ sgm_rsrc sgm_make_rsrc(const void *p, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, (int)(uint32_t)bytes, 0x00020000);
}
__device__ __forceinline__ float sgm_buf_ld(sgm_rsrc r, uint32_t voff, uint32_t soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
// LDS hand-off inside ONE wave: the LDS executes a wave's instructions in order, only the compiler must not move the loads up
__device__ __forceinline__ void sgm_wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double sgm_wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the six distinct window weights in VECTOR registers (a vector instruction with an SGPR source issues at half rate on gfx950:
// LAB.md 6.2); the asm keeps the compiler from recognising them as uniform
struct SgmW { float w[11]; };
__device__ __forceinline__ SgmW sgm_weights(const SgMetricsArgs &a)
{
    SgmW w;
#pragma unroll
    for (int k = 0; k < 6; k++) { float v; asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(a.w[k])); w.w[k] = v; w.w[10 - k] = v; }
    return w;
}

template <bool MASK> struct SgmCtx {
    sgm_rsrc pred, gt, mask;
    sgm_f2 *sIn;                  // [2][SGM_PITCH] staged rows (x, y)
    int H, R0, R1, lane;
    uint32_t pitch;               // bytes per image row
    uint32_t o0, o1;              // byte offsets in a row of the two columns a lane loads (the second: lanes 0-9)
    bool in0, in1, incol;         // those columns lie inside the image; the lane's own result column does
    bool own0;                    // the strip's own pixel of this lane is the one of its first load (lanes 5-63), else of its second
};
template <bool MASK> struct SgmSt {
    float hw[5][11];              // ring of the last 11 rows of the horizontally windowed x, y, x^2, y^2, x y
    float pin[2][MASK ? 6 : 4];   // the next two input rows, in flight: pred, target (, mask) at the lane's two columns
    double acc_se, acc_ssim;
};

template <bool MASK>
__device__ __forceinline__ void sgm_prefetch_row(const SgmCtx<MASK> &c, float (&pin)[MASK ? 6 : 4], int y)
{
    const uint32_t r = (uint32_t)sgm_clampi(y, c.H) * c.pitch;   // (rows outside count as zeros where they are USED)
    pin[0] = sgm_buf_ld(c.pred, c.o0, r); pin[1] = sgm_buf_ld(c.gt, c.o0, r);
    pin[2] = sgm_buf_ld(c.pred, c.o1, r); pin[3] = sgm_buf_ld(c.gt, c.o1, r);
    if (MASK) { pin[4] = sgm_buf_ld(c.mask, c.o0, r); pin[5] = sgm_buf_ld(c.mask, c.o1, r); }
}

// 11-tap sum in the fixed order k = 0..10 (the first tap is a product)
#define SGM_WIN11(acc, expr) { acc = w.w[0] * (expr(0)); acc = fmaf(w.w[1], expr(1), acc); acc = fmaf(w.w[2], expr(2), acc);     \
    acc = fmaf(w.w[3], expr(3), acc); acc = fmaf(w.w[4], expr(4), acc); acc = fmaf(w.w[5], expr(5), acc);                        \
    acc = fmaf(w.w[6], expr(6), acc); acc = fmaf(w.w[7], expr(7), acc); acc = fmaf(w.w[8], expr(8), acc);                        \
    acc = fmaf(w.w[9], expr(9), acc); acc = fmaf(w.w[10], expr(10), acc); }

// One row step.  PH = t mod 11 is the ring slot the new row goes to; slot (PH + 1 + k) mod 11 holds the row k rows below the oldest.
template <bool MASK, bool CLAMP, int PH>
__device__ __forceinline__ void sgm_step(const SgmW &w, const SgmCtx<MASK> &c, SgmSt<MASK> &s, int t)
{
    const int yin = c.R0 - 5 + t;
    sgm_f2 *sIn = c.sIn + (t & 1) * SGM_PITCH;
    // (1) the row that arrived -> x = [clamped] pred [* mask], y = gt [* mask] (zero outside the image: conv2d's zero padding)
    {
        const bool rowok = (unsigned)yin < (unsigned)c.H;
        const bool k0 = rowok && c.in0, k1 = rowok && c.in1;
        float x0 = CLAMP ? sgm_clamp01(s.pin[0][0]) : s.pin[0][0], y0 = s.pin[0][1];
        float x1 = CLAMP ? sgm_clamp01(s.pin[0][2]) : s.pin[0][2], y1 = s.pin[0][3];
        if (MASK) { const float m0 = s.pin[0][4], m1 = s.pin[0][5]; x0 *= m0; y0 *= m0; x1 *= m1; y1 *= m1; }
        x0 = k0 ? x0 : 0.0f; y0 = k0 ? y0 : 0.0f; x1 = k1 ? x1 : 0.0f; y1 = k1 ? y1 : 0.0f;
        sIn[c.lane] = sgm_f2{ x0, y0 };
        if (c.lane < 10) sIn[SGM_LN + c.lane] = sgm_f2{ x1, y1 };
        // squared difference of the strip's own pixel of this row (a column outside the image: 0 - 0)
        if (yin >= c.R0 && yin < c.R1) {
            const double d = (double)(c.own0 ? x0 - y0 : x1 - y1);
            s.acc_se = fma(d, d, s.acc_se);
        }
    }
#pragma unroll
    for (int q = 0; q < (MASK ? 6 : 4); q++) s.pin[0][q] = s.pin[1][q];
    sgm_prefetch_row<MASK>(c, s.pin[1], yin + 2);
    sgm_wave_lds_sync();
    // (2) 11-tap window across the lanes
    {
        sgm_f2 v[11];
#pragma unroll
        for (int k = 0; k < 11; k++) v[k] = sIn[c.lane + k];
        float h0, h1, h2, h3, h4;
        {
            const float wx = w.w[0] * v[0].x, wy = w.w[0] * v[0].y;
            h0 = wx; h1 = wy; h2 = wx * v[0].x; h3 = wy * v[0].y; h4 = wx * v[0].y;
        }
#pragma unroll
        for (int k = 1; k < 11; k++) {
            const float wx = w.w[k] * v[k].x, wy = w.w[k] * v[k].y;
            h0 += wx; h1 += wy;
            h2 = fmaf(wx, v[k].x, h2); h3 = fmaf(wy, v[k].y, h3); h4 = fmaf(wx, v[k].y, h4);
        }
        s.hw[0][PH] = h0; s.hw[1][PH] = h1; s.hw[2][PH] = h2; s.hw[3][PH] = h3; s.hw[4][PH] = h4;
    }
    if (t < 10) return;
    // (3) window down the rows: statistics and SSIM value of row yin - 5 (always a row of this chunk: t < R1 - R0 + 10)
    {
        float st[5];
#pragma unroll
        for (int q = 0; q < 5; q++) {
#define SGM_RING(k) s.hw[q][(PH + 1 + (k)) % 11]
            SGM_WIN11(st[q], SGM_RING)
#undef SGM_RING
        }
        const float mu1 = st[0], mu2 = st[1], e11 = st[2], e22 = st[3], e12 = st[4];
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = e11 - mu1s, s2 = e22 - mu2s, s12 = e12 - mu12;
        const float A = mu1s + mu2s + C1, B = s1 + s2 + C2, Cn = 2.0f * mu12 + C1, D = 2.0f * s12 + C2;
        const float m = (Cn * D) * (SGM_RCP(A) * SGM_RCP(B));
        s.acc_ssim += c.incol ? (double)m : 0.0;
    }
}

// unit of workgroup b (as sg_loss.hip): runs of SGM_RUN consecutive units -- the three channels of neighbouring strips: shared mask,
// shared halo columns -- stay on one XCD's L2 (workgroup b runs on XCD b % 8), the runs are dealt round-robin to the XCDs, frame f
// starting at XCD f * (runs mod 8).  Placement only: which workgroup computes a unit does not change the unit's result.
__device__ __forceinline__ int sgm_unit_of_block(int b, int shift)
{
    const int xcd = (b - shift) & 7, slot = b >> 3;
    return ((slot / SGM_RUN) * 8 + xcd) * SGM_RUN + slot % SGM_RUN;
}
static inline int sgm_blocks(int units) { return ((units + 8 * SGM_RUN - 1) / (8 * SGM_RUN)) * (8 * SGM_RUN); }

// The 55-register ring, the 22 taps of the staged row, the rows in flight; the compiler packs the (x, y) chains into v_pk_* pairs
// (this file is built with the library's default flags), whose even-aligned operands bring it to 128 VGPRs without a mask -- four
// waves per SIMD -- and 132 with one: three (held to four, the masked kernel spilled four registers to scratch).  LAB.md has both
// timed against a build without the SLP vectoriser (100 / 104 VGPRs).
template <bool MASK, bool CLAMP>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MASK ? 3 : 4, 4)))
sg_metrics_kernel(SgMetricsArgs a, const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask,
                  char *__restrict__ ws)
{
    __shared__ sgm_f2 sIn[2][SGM_PITCH];
    const int u = sgm_unit_of_block(blockIdx.x, (int)blockIdx.y * a.xcd_rot);
    if (u >= a.units) return;
    const int lane = threadIdx.x, frame = blockIdx.y;
    const int ch = u % 3, strip = (u / 3) % a.nstrips, chunk = u / (3 * a.nstrips);
    const SgmW w = sgm_weights(a);
    SgmCtx<MASK> c;
    c.sIn = &sIn[0][0];
    c.H = a.H; c.lane = lane; c.pitch = (uint32_t)a.W * 4u;
    c.R0 = chunk * a.R; c.R1 = c.R0 + a.R < a.H ? c.R0 + a.R : a.H;
    {
        const int col = strip * SGM_LN + lane;                   // the column whose window statistics this lane holds
        const int l0 = col - 5, l1 = l0 + SGM_LN;                // the columns it loads for the row window (the second: lanes 0-9)
        c.in0 = l0 >= 0 && l0 < a.W; c.in1 = lane < 10 && l1 < a.W; c.incol = col < a.W;
        c.o0 = 4u * (uint32_t)sgm_clampi(l0, a.W); c.o1 = lane < 10 ? 4u * (uint32_t)sgm_clampi(l1, a.W) : c.o0;
        c.own0 = lane >= 5;                                      // columns strip * 64 + 0..58 here, + 59..63 in lanes 0-4's second load
    }
    {
        const size_t hw = (size_t)a.W * a.H, plane = hw * 4;
        c.pred = sgm_make_rsrc(pred + (size_t)frame * 3 * hw + ch * hw, plane);
        c.gt = sgm_make_rsrc(gt + (size_t)frame * a.gt_stride + ch * hw, plane);
        c.mask = sgm_make_rsrc(MASK ? mask + (size_t)frame * a.mask_stride : nullptr, MASK ? plane : 0);
    }
    SgmSt<MASK> s;
#pragma unroll
    for (int k = 0; k < 11; k++)
#pragma unroll
        for (int q = 0; q < 5; q++) s.hw[q][k] = 0.0f;
    s.acc_se = 0.0; s.acc_ssim = 0.0;
    const int T = (c.R1 - c.R0) + 10;
    sgm_prefetch_row<MASK>(c, s.pin[0], c.R0 - 5);
    sgm_prefetch_row<MASK>(c, s.pin[1], c.R0 - 4);
    for (int t0 = 0; t0 < T; t0 += 11) {
#define SGM_STEP(PH) if (t0 + PH < T) sgm_step<MASK, CLAMP, PH>(w, c, s, t0 + PH)
        SGM_STEP(0); SGM_STEP(1); SGM_STEP(2); SGM_STEP(3); SGM_STEP(4); SGM_STEP(5); SGM_STEP(6); SGM_STEP(7); SGM_STEP(8); SGM_STEP(9); SGM_STEP(10);
#undef SGM_STEP
    }
    const double se = sgm_wave_sum_f64(s.acc_se), ss = sgm_wave_sum_f64(s.acc_ssim);
    // partials of a frame: [channel][chunk x strip] pairs (sum of squared differences, sum of the SSIM map)
    if (lane == 0)
        ((double2 *)(ws + (size_t)frame * a.ws_stride))[(size_t)ch * a.ncell + (size_t)chunk * a.nstrips + strip] = make_double2(se, ss);
}

// one workgroup per frame: the partials of each channel in a fixed order (thread t: cells t, t + 256, ...; butterfly; four waves)
__global__ void __launch_bounds__(256)
sg_metrics_reduce_kernel(SgMetricsArgs a, const char *__restrict__ ws, float *__restrict__ metrics)
{
    __shared__ double sR[4][6];
    const double2 *part = (const double2 *)(ws + (size_t)blockIdx.x * a.ws_stride);
    metrics += (size_t)SG_METRICS_FLOATS * blockIdx.x;
    const int tid = threadIdx.x;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        double t0 = 0.0, t1 = 0.0;
        for (int i = tid; i < a.ncell; i += 256) { const double2 p = part[(size_t)ch * a.ncell + i]; t0 += p.x; t1 += p.y; }
        t0 = sgm_wave_sum_f64(t0); t1 = sgm_wave_sum_f64(t1);
        if ((tid & 63) == 0) { sR[tid >> 6][2 * ch] = t0; sR[tid >> 6][2 * ch + 1] = t1; }
    }
    __syncthreads();
    if (tid == 0) {
        const double hw = (double)a.W * (double)a.H;
        double psum = 0.0, ssum = 0.0;
        for (int ch = 0; ch < 3; ch++) {
            const double se = (sR[0][2 * ch] + sR[1][2 * ch]) + (sR[2][2 * ch] + sR[3][2 * ch]);
            ssum += (sR[0][2 * ch + 1] + sR[1][2 * ch + 1]) + (sR[2][2 * ch + 1] + sR[3][2 * ch + 1]);
            const double mse = se / hw;
            // 20 log10(1 / sqrt(mse)) in fp64, rounded once; a channel that equals its target: +inf, as the reference's 1 / 0
            const double ps = mse == 0.0 ? (double)INFINITY : 20.0 * log10(1.0 / sqrt(mse));
            metrics[ch] = (float)mse; metrics[3 + ch] = (float)ps;
            psum += ps;
        }
        metrics[6] = (float)(psum / 3.0);
        metrics[7] = (float)(ssum / (3.0 * hw));
    }
}

// strips x chunks of ONE frame, from W and H alone (a frame's partials must not depend on K): about SGM_UNITS units, chunks of at
// least SG_METRICS_CHUNK_ROWS rows
static bool sg_metrics_args(int W, int H, size_t gt_stride, size_t mask_stride, SgMetricsArgs &a)
{
    if (W < 1 || H < 1 || (size_t)W * (size_t)H >= ((size_t)1 << 30)) return false;
    a.W = W; a.H = H; a.gt_stride = gt_stride; a.mask_stride = mask_stride;
    sg_ssim_window(a.w);                                      // (sg_host.h: the reference's fp32 window, bit for bit)
    a.nstrips = (W + SGM_LN - 1) / SGM_LN;
    const int most = (H + SG_METRICS_CHUNK_ROWS - 1) / SG_METRICS_CHUNK_ROWS;
    int nch = SGM_UNITS / (3 * a.nstrips);
    nch = nch < 1 ? 1 : (nch > most ? most : nch);
    a.R = (H + nch - 1) / nch;
    a.nchunks = (H + a.R - 1) / a.R;
    a.ncell = a.nstrips * a.nchunks;
    a.units = 3 * a.ncell;
    a.xcd_rot = ((a.units + SGM_RUN - 1) / SGM_RUN) % 8;
    a.ws_stride = ((size_t)a.units * sizeof(double2) + 255) & ~(size_t)255;
    return true;
}

extern "C" size_t sg_image_metrics_ws_bytes(int K, int width, int height)
{
    SgMetricsArgs a;
    if (K < 1 || K > 65535 || !sg_metrics_args(width, height, 0, 0, a)) return 0;
    return (size_t)K * a.ws_stride;
}

extern "C" int sg_image_metrics_frames(int K, int width, int height, int flags, const float *pred, const float *gt, size_t gt_stride,
                                       const float *mask, size_t mask_stride, void *ws, float *metrics, void *stream)
{
    SgMetricsArgs a;
    if (K < 1 || K > 65535) return sg_set_error("sg_image_metrics_frames: K must be 1..65535", hipSuccess);
    if (!sg_metrics_args(width, height, gt_stride, mask_stride, a))
        return sg_set_error("sg_image_metrics_frames: width and height must be >= 1 (and fewer than 2^30 pixels)", hipSuccess);
    if (flags & ~SG_METRICS_CLAMP) return sg_failf("sg_image_metrics_frames: unknown flag bits 0x%x", flags & ~SG_METRICS_CLAMP);
    if (!pred || !gt || !ws || !metrics) return sg_set_error("sg_image_metrics_frames: null pointer", hipSuccess);
    if (!mask && mask_stride) return sg_set_error("sg_image_metrics_frames: mask_stride without a mask", hipSuccess);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(sgm_blocks(a.units), K);
    const bool clamp = (flags & SG_METRICS_CLAMP) != 0;
#define SGM_LAUNCH(M, C) hipLaunchKernelGGL((sg_metrics_kernel<M, C>), grid, dim3(64), 0, st, a, pred, gt, mask, (char *)ws)
    if (mask) { if (clamp) SGM_LAUNCH(true, true); else SGM_LAUNCH(true, false); }
    else      { if (clamp) SGM_LAUNCH(false, true); else SGM_LAUNCH(false, false); }
#undef SGM_LAUNCH
    hipLaunchKernelGGL(sg_metrics_reduce_kernel, dim3(K), dim3(256), 0, st, a, (const char *)ws, metrics);
    return sg_launched("sg_image_metrics_frames");
}
