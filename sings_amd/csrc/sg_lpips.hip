// LPIPS-VGG (the `lpips` 0.1 package, net='vgg', version='0.1', eval mode) and the patch glue of the reference's LPIPS term
// (sings/rec/losses/loss.py:71-80): forward value and the gradient w.r.t. the first input.
//
//   scaling      xs = (x' - shift) / scale,  x' = x or 2x - 1 (normalize)
//   trunk        VGG16 `features` up to relu5_3: 13 3x3 convs (padding 1, bias, ReLU), MaxPool2d(2,2) in front of slices 2..5;
//                slice outputs relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
//   head         per slice: n = f / (sqrt(sum_c f^2) + 1e-10) for both inputs, d = lin . (n0 - n1)^2, mean over H x W; summed
//
// Layout: activations are channel-minor (NHWC), the two inputs stacked as 2B images (in0 = images 0..B-1, in1 = B..2B-1).
// Convs with Cin >= 64 are an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products): M = pixels of ONE image, N = Cout,
// K = 9 Cin ordered (tap, ci).  A workgroup owns a 64-pixel x 64-column tile (four waves of 32 x 32); a K chunk is one tap and 32
// input channels, staged through LDS (double-buffered; the next chunk's loads are in flight during the current chunk's MFMAs).
// The reduction index is permuted inside a chunk (MFMA step s pairs k = s and k = 16 + s) so that a lane reads its next four
// operands with one 16-B LDS read (the same trick as sg_linear.hip).  Bias and ReLU are the epilogue.
// The input gradient is the same tile loop with the weights transposed and flipped, W'[ci][co][2-ky][2-kx] (packed once by the
// host), and the ReLU select of the layer's own output (y > 0 ? g : 0) fused into the operand load.
// Determinism: every sum runs in a fixed order, no atomics; no tile spans two images, so a patch's value does not depend on what
// else is in the batch.
#include "sg_host.h"

namespace {

constexpr int LP_NCONV = 13;
const int lp_cin[LP_NCONV] = { 3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512 };
const int lp_cout[LP_NCONV] = { 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512 };
const int lp_level[LP_NCONV] = { 0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4 };
const int lp_slice_layer[5] = { 1, 3, 6, 9, 12 };                           // relu1_2 .. relu5_3
const int lp_slice_ch[5] = { 64, 128, 256, 512, 512 };

inline size_t lp_align(size_t v, size_t a) { return (v + a - 1) / a * a; }

// weight offsets (floats): conv l: W (l = 0: [64][3][3][3] as torch; else [Cout][9][Cin], k = tap * Cin + ci), bias [Cout],
// W' (l >= 1: [Cin][9][Cout] = W[co][ci][2-ky][2-kx]); lin k [C_k]; shift [3]; scale [3]
struct LpWeights { size_t off[SG_LPIPS_NUM_OFFSETS]; size_t total; };
LpWeights lp_weights()
{
    LpWeights w;
    size_t o = 0;
    for (int l = 0; l < LP_NCONV; l++) {
        const size_t nw = (size_t)lp_cout[l] * lp_cin[l] * 9;
        w.off[3 * l] = o; o = lp_align(o + nw, 4);
        w.off[3 * l + 1] = o; o = lp_align(o + lp_cout[l], 4);
        w.off[3 * l + 2] = o; o = lp_align(o + (l ? nw : 0), 4);
    }
    for (int k = 0; k < 5; k++) { w.off[3 * LP_NCONV + k] = o; o = lp_align(o + lp_slice_ch[k], 4); }
    w.off[3 * LP_NCONV + 5] = o; o = lp_align(o + 3, 4);
    w.off[3 * LP_NCONV + 6] = o; o = lp_align(o + 3, 4);
    w.total = o;
    return w;
}

// workspace (bytes, 256-aligned pieces): y_l [2B][H_l][W_l][Cout_l] (13), pool outputs and argmax [2B][H][W][C] (4 + 4),
// per-pixel head terms [B][H_k W_k] (5), two gradient buffers [B][H W][64] (the largest activation of one input)
struct LpPlan {
    int H[5], W[5];
    size_t y[LP_NCONV], pool[4], arg[4], dpix[5], g[2], total;
};
bool lp_plan(int B, int H, int W, LpPlan &p)
{
    if (B < 1 || H < SG_LPIPS_MIN_SIZE || W < SG_LPIPS_MIN_SIZE) return false;
    if ((double)2 * B * H * W * 64 >= 2147483647.0) return false;          // int element indices inside the kernels
    p.H[0] = H; p.W[0] = W;
    for (int k = 1; k < 5; k++) { p.H[k] = p.H[k - 1] / 2; p.W[k] = p.W[k - 1] / 2; }
    size_t o = 0;
    const size_t NI = 2 * (size_t)B;
    for (int l = 0; l < LP_NCONV; l++) {
        const int v = lp_level[l];
        p.y[l] = o; o = lp_align(o + NI * p.H[v] * p.W[v] * lp_cout[l] * 4, 256);
    }
    for (int q = 0; q < 4; q++) {
        const size_t n = NI * p.H[q + 1] * p.W[q + 1] * lp_slice_ch[q];
        p.pool[q] = o; o = lp_align(o + n * 4, 256);
        p.arg[q] = o; o = lp_align(o + n, 256);
    }
    for (int k = 0; k < 5; k++) { p.dpix[k] = o; o = lp_align(o + (size_t)B * p.H[k] * p.W[k] * 4, 256); }
    for (int i = 0; i < 2; i++) { p.g[i] = o; o = lp_align(o + (size_t)B * H * W * 64 * 4, 256); }
    p.total = o;
    return true;
}

// ---- conv1_1 (Cin = 3): plain vector code, the scaling layer fused into the operand load ---------------------------------------
// y0[img][p][co] = relu(b[co] + sum W[co][c][ky][kx] xs[img][c][y+ky-1][x+kx-1]); one thread per (image, pixel, output channel)
__global__ void __launch_bounds__(256) lp_conv1_fwd(int B, int H, int W, int normalize, const float *__restrict__ in0,
                                                    const float *__restrict__ in1, const float *__restrict__ Wt,
                                                    const float *__restrict__ bias, const float *__restrict__ shift,
                                                    const float *__restrict__ scale, float *__restrict__ y)
{
    const int HW = H * W;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * B * HW * 64) return;
    const int co = idx & 63, pix = idx >> 6;
    const int img = pix / HW, p = pix - img * HW;
    const int py = p / W, px = p - py * W;
    const float *src = img < B ? in0 + (size_t)img * 3 * HW : in1 + (size_t)(img - B) * 3 * HW;
    float acc = 0.0f;
    for (int c = 0; c < 3; c++) {
        const float sh = shift[c], sc = scale[c];
        for (int ky = 0; ky < 3; ky++) {
            const int yy = py + ky - 1;
            if (yy < 0 || yy >= H) continue;
            for (int kx = 0; kx < 3; kx++) {
                const int xx = px + kx - 1;
                if (xx < 0 || xx >= W) continue;
                float v = src[(size_t)c * HW + yy * W + xx];
                if (normalize) v = 2.0f * v - 1.0f;
                v = (v - sh) / sc;
                acc = fmaf(Wt[((co * 3 + c) * 3 + ky) * 3 + kx], v, acc);
            }
        }
    }
    const float z = acc + bias[co];
    y[idx] = z > 0.0f ? z : 0.0f;
}

// dL/din0[b][c][a][e] = (sum_{co,ky,kx} W[co][c][ky][kx] dz[b][a-ky+1][e-kx+1][co]) / scale[c] (x 2 if normalize),
// dz = y0 > 0 ? g : 0 (ReLU's backward is a select).  One thread per (image < B, channel, pixel).
__global__ void __launch_bounds__(256) lp_conv1_bwd(int B, int H, int W, int normalize, const float *__restrict__ y0,
                                                    const float *__restrict__ g, const float *__restrict__ Wt,
                                                    const float *__restrict__ scale, float *__restrict__ din0)
{
    const int HW = H * W;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * 3 * HW) return;
    const int img = idx / (3 * HW), r = idx - img * 3 * HW, c = r / HW, p = r - c * HW;
    const int py = p / W, px = p - py * W;
    float acc = 0.0f;
    for (int ky = 0; ky < 3; ky++) {
        const int yy = py - ky + 1;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; kx++) {
            const int xx = px - kx + 1;
            if (xx < 0 || xx >= W) continue;
            const size_t q = ((size_t)img * HW + yy * W + xx) * 64;
            for (int co = 0; co < 64; co++) {
                const float dz = y0[q + co] > 0.0f ? g[q + co] : 0.0f;
                acc = fmaf(Wt[((co * 3 + c) * 3 + ky) * 3 + kx], dz, acc);
            }
        }
    }
    float d = acc / scale[c];
    if (normalize) d = 2.0f * d;
    din0[idx] = d;
}

// ---- 3x3 conv as an implicit GEMM on the matrix cores ---------------------------------------------------------------------------
// FWD: Y[img][p][co] = relu(bias[co] + sum_{tap,ci} X[img][p + tap][ci] Wp[co][tap][ci])
// BWD: Y[img][p][co] = sum_{tap,ci} (S > 0 ? X : 0)[img][p + tap][ci] Wp[co][tap][ci]   (X: gradient, S: the layer's output)
// CI a multiple of 32, CO a multiple of 64; grid (tiles_per_img * images, CO / 64), 256 threads.
#define LP_XS 36                                                            // floats per LDS row: 32 + 4 (conflict-free 16-B reads)
template <bool BWD>
__global__ void __launch_bounds__(256) lp_conv3x3(int H, int W, int CI, int CO, int tiles_per_img, const float *__restrict__ X,
                                                  const float *__restrict__ S, const float *__restrict__ Wp,
                                                  const float *__restrict__ bias, float *__restrict__ Y)
{
    __shared__ float sA[2][64 * LP_XS];                                    // [pixel][k]
    __shared__ float sB[2][64 * LP_XS];                                    // [output column][k]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int img = blockIdx.x / tiles_per_img, p0 = (blockIdx.x - img * tiles_per_img) * 64;
    const int co0 = blockIdx.y * 64;
    const int HW = H * W;
    const float *Ximg = X + (size_t)img * HW * CI;
    const float *Simg = BWD ? S + (size_t)img * HW * CI : nullptr;
    // staging: thread -> row r (pixel of the A tile, column of the B tile), floats 8q .. 8q + 7 of the 32-float chunk
    const int r = tid >> 2, q = tid & 3;
    const int p = p0 + r;
    const bool prow = p < HW;
    const int py = prow ? p / W : 0, px = prow ? p - py * W : 0;
    const int cpt = CI >> 5;                                               // chunks per tap
    const int nchunks = 9 * cpt;
    const float *wrow = Wp + (size_t)(co0 + r) * 9 * CI + 8 * q;
    float4 ra[2], rb[2];
    auto fetch = [&](int c) {
        const int tap = c / cpt, ci0 = (c - tap * cpt) * 32;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int yy = py + ky - 1, xx = px + kx - 1;
        const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        ra[0] = ra[1] = z4;
        if (prow && yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const size_t o = (size_t)(yy * W + xx) * CI + ci0 + 8 * q;
            ra[0] = *(const float4 *)(Ximg + o);
            ra[1] = *(const float4 *)(Ximg + o + 4);
            if (BWD) {
                const float4 s0 = *(const float4 *)(Simg + o), s1 = *(const float4 *)(Simg + o + 4);
                ra[0].x = s0.x > 0.0f ? ra[0].x : 0.0f; ra[0].y = s0.y > 0.0f ? ra[0].y : 0.0f;
                ra[0].z = s0.z > 0.0f ? ra[0].z : 0.0f; ra[0].w = s0.w > 0.0f ? ra[0].w : 0.0f;
                ra[1].x = s1.x > 0.0f ? ra[1].x : 0.0f; ra[1].y = s1.y > 0.0f ? ra[1].y : 0.0f;
                ra[1].z = s1.z > 0.0f ? ra[1].z : 0.0f; ra[1].w = s1.w > 0.0f ? ra[1].w : 0.0f;
            }
        }
        rb[0] = *(const float4 *)(wrow + (size_t)c * 32);
        rb[1] = *(const float4 *)(wrow + (size_t)c * 32 + 4);
    };
    auto stash = [&](int buf) {
        *(float4 *)&sA[buf][r * LP_XS + 8 * q] = ra[0];
        *(float4 *)&sA[buf][r * LP_XS + 8 * q + 4] = ra[1];
        *(float4 *)&sB[buf][r * LP_XS + 8 * q] = rb[0];
        *(float4 *)&sB[buf][r * LP_XS + 8 * q + 4] = rb[1];
    };
    const int pw = wave & 1, cw = wave >> 1;                               // this wave: pixels 32 pw.., columns 32 cw..
    const int j = lane & 31, h = lane >> 5;
    sg_v16f acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    fetch(0);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (int c = 0; c < nchunks; c++, buf ^= 1) {
        if (c + 1 < nchunks) fetch(c + 1);                                 // in flight during the MFMAs below
        // A operand: A[pixel j][k = 16 h + s], B operand: B[k = 16 h + s][column j]
        const float *arow = &sA[buf][(32 * pw + j) * LP_XS + 16 * h];
        const float *brow = &sB[buf][(32 * cw + j) * LP_XS + 16 * h];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const float4 a = *(const float4 *)(arow + 4 * v);
            const float4 b = *(const float4 *)(brow + 4 * v);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        if (c + 1 < nchunks) stash(buf ^ 1);                               // (that buffer was last read before the barrier below
        __syncthreads();                                                   //  of the previous iteration)
    }
    // epilogue: register i of lane (j, h) is pixel 32 pw + (i & 3) + 8 (i >> 2) + 4 h, column 32 cw + j (128-B row pieces)
    const int co = co0 + 32 * cw + j;
    const float bv = BWD ? 0.0f : bias[co];
    float *Yimg = Y + (size_t)img * HW * CO;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int pp = p0 + 32 * pw + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (pp < HW) {
            float v = acc[i];
            if (!BWD) { v += bv; v = v > 0.0f ? v : 0.0f; }
            Yimg[(size_t)pp * CO + co] = v;
        }
    }
}

// ---- MaxPool2d(2, 2): floor, first maximum in row-major order (torch: `val > max || isnan(val)`) ------------------------------
__global__ void __launch_bounds__(256) lp_pool_fwd(int NI, int H, int W, int C, const float *__restrict__ x, float *__restrict__ y,
                                                   uint8_t *__restrict__ arg)
{
    const int Ho = H / 2, Wo = W / 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= NI * Ho * Wo * C) return;
    const int c = idx % C, pix = idx / C;
    const int img = pix / (Ho * Wo), po = pix - img * Ho * Wo;
    const int yo = po / Wo, xo = po - yo * Wo;
    const float *base = x + ((size_t)img * H * W + (size_t)(2 * yo) * W + 2 * xo) * C + c;
    float best = base[0];
    int bi = 0;
    const float v1 = base[C], v2 = base[(size_t)W * C], v3 = base[(size_t)W * C + C];
    if (v1 > best || isnan(v1)) { best = v1; bi = 1; }
    if (v2 > best || isnan(v2)) { best = v2; bi = 2; }
    if (v3 > best || isnan(v3)) { best = v3; bi = 3; }
    y[idx] = best;
    arg[idx] = (uint8_t)bi;
}

// gradient at the pool's input: each input element takes its window's gradient if it was the chosen maximum (a gather, no atomics)
__global__ void __launch_bounds__(256) lp_pool_bwd(int NI, int H, int W, int C, const float *__restrict__ gy,
                                                   const uint8_t *__restrict__ arg, float *__restrict__ gx)
{
    const int Ho = H / 2, Wo = W / 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= NI * H * W * C) return;
    const int c = idx % C, pix = idx / C;
    const int img = pix / (H * W), p = pix - img * H * W;
    const int yy = p / W, xx = p - yy * W;
    const int yo = yy >> 1, xo = xx >> 1;
    float v = 0.0f;
    if (yo < Ho && xo < Wo) {
        const size_t o = ((size_t)img * Ho * Wo + (size_t)yo * Wo + xo) * C + c;
        if (arg[o] == (uint8_t)(((yy & 1) << 1) | (xx & 1))) v = gy[o];
    }
    gx[idx] = v;
}

// ---- head: channel norm, squared difference, lin, per pixel (one wave per pixel; fixed-order butterfly sums) ------------------
__device__ __forceinline__ float lp_wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// dpix[b][p] = sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2,  f0 = f[b], f1 = f[b + B]
__global__ void __launch_bounds__(256) lp_head_fwd(int B, int HW, int C, const float *__restrict__ f, const float *__restrict__ lin,
                                                   float *__restrict__ dpix)
{
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= B * HW) return;
    const int b = wid / HW, p = wid - b * HW;
    const float *f0 = f + ((size_t)b * HW + p) * C, *f1 = f + ((size_t)(b + B) * HW + p) * C;
    float s0 = 0.0f, s1 = 0.0f;
    for (int c = lane; c < C; c += 64) { s0 = fmaf(f0[c], f0[c], s0); s1 = fmaf(f1[c], f1[c], s1); }
    s0 = lp_wave_sum(s0); s1 = lp_wave_sum(s1);
    const float d0 = sqrtf(s0) + 1e-10f, d1 = sqrtf(s1) + 1e-10f;
    float acc = 0.0f;
    for (int c = lane; c < C; c += 64) {
        const float e = f0[c] / d0 - f1[c] / d1;
        acc = fmaf(lin[c], e * e, acc);
    }
    acc = lp_wave_sum(acc);
    if (lane == 0) dpix[wid] = acc;
}

// gradient of the slice's term w.r.t. f0, ADDED to g (accum) or written: q = (up[b] / HW) 2 lin (n0 - n1),
// df = q / (r + eps) - f0 (q . f0) / ((r + eps)^2 r),  r = |f0|.  r = 0 (an all-zero feature vector): 0 -- where torch forms
// a NaN that the slice's ReLU select then zeroes, every component of f0 is 0 and the select zeroes this value anyway.
__global__ void __launch_bounds__(256) lp_head_bwd(int B, int HW, int C, const float *__restrict__ f, const float *__restrict__ lin,
                                                   const float *__restrict__ up, int accum, float *__restrict__ g)
{
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= B * HW) return;
    const int b = wid / HW, p = wid - b * HW;
    const float *f0 = f + ((size_t)b * HW + p) * C, *f1 = f + ((size_t)(b + B) * HW + p) * C;
    float *gp = g + ((size_t)b * HW + p) * C;
    float s0 = 0.0f, s1 = 0.0f;
    for (int c = lane; c < C; c += 64) { s0 = fmaf(f0[c], f0[c], s0); s1 = fmaf(f1[c], f1[c], s1); }
    s0 = lp_wave_sum(s0); s1 = lp_wave_sum(s1);
    const float r0 = sqrtf(s0), d0 = r0 + 1e-10f, d1 = sqrtf(s1) + 1e-10f;
    const float gs = up[b] / (float)HW;
    float dot = 0.0f;
    for (int c = lane; c < C; c += 64) {
        const float qc = gs * lin[c] * 2.0f * (f0[c] / d0 - f1[c] / d1);
        dot = fmaf(qc, f0[c], dot);
    }
    dot = lp_wave_sum(dot);
    const float k2 = r0 > 0.0f ? dot / (d0 * d0 * r0) : 0.0f;
    for (int c = lane; c < C; c += 64) {
        float v = 0.0f;
        if (r0 > 0.0f) {
            const float qc = gs * lin[c] * 2.0f * (f0[c] / d0 - f1[c] / d1);
            v = qc / d0 - f0[c] * k2;
        }
        gp[c] = accum ? gp[c] + v : v;
    }
}

struct LpSlices { const float *dpix[5]; int hw[5]; };

// out[b] = sum_k mean_p dpix_k[b][p] (slices summed in order 1..5, as lpips does); one workgroup per image, fixed-order tree sums
__global__ void __launch_bounds__(256) lp_head_reduce(LpSlices s, float *__restrict__ out)
{
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float val = 0.0f;
    for (int k = 0; k < 5; k++) {
        const int hw = s.hw[k];
        const float *d = s.dpix[k] + (size_t)b * hw;
        float a = 0.0f;
        for (int p = tid; p < hw; p += 256) a += d[p];
        red[tid] = a;
        __syncthreads();
        for (int m = 128; m >= 1; m >>= 1) {
            if (tid < m) red[tid] += red[tid + m];
            __syncthreads();
        }
        const float mean = red[0] / (float)hw;
        val = k == 0 ? mean : val + mean;
        __syncthreads();
    }
    if (tid == 0) out[b] = val;
}

// ---- patches (loss.py:71-80 + utils/image/sampler.py) -------------------------------------------------------------------------
// The origins are device data and are not trusted: each is clamped into [0, H - P] x [0, W - P] before any address is formed.
__device__ __forceinline__ int lp_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float lp_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }   // torch.clamp (NaN stays)

// pred[k n + i][c][u][v] = min(clamp(raw, 0, 1) m + r (1 - m), 1),  gt[..] = (rgb m + bg (1 - m)) m + r (1 - m)  at the patch pixel
__global__ void __launch_bounds__(256) lp_patch_gather(int K, int n, int P, int H, int W, const float *__restrict__ raw,
                                                       const float *__restrict__ gt_rgb, const float *__restrict__ mask,
                                                       const float *__restrict__ bg, const float *__restrict__ bg_rand,
                                                       const int32_t *__restrict__ origins, float *__restrict__ pred,
                                                       float *__restrict__ gt)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int PP = P * P;
    if (idx >= K * n * 3 * PP) return;
    const int patch = idx / (3 * PP), rr = idx - patch * 3 * PP, c = rr / PP, e = rr - c * PP;
    const int u = e / P, v = e - u * P;
    const int k = patch / n;
    const int oy = lp_clampi(origins[2 * patch], H - P), ox = lp_clampi(origins[2 * patch + 1], W - P);
    const size_t HW = (size_t)H * W, pix = (size_t)(oy + u) * W + (ox + v);
    const size_t ci = ((size_t)k * 3 + c) * HW + pix;
    const float m = mask[(size_t)k * HW + pix], om = 1.0f - m, r = bg_rand[ci];
    const float img = lp_clamp01(raw[ci]) * m + r * om;
    pred[idx] = img > 1.0f ? 1.0f : img;                                    // .clip(max=1)
    const float gimg = gt_rgb[ci] * m + bg[c] * om;
    gt[idx] = gimg * m + r * om;
}

// dL/draw[k][c][y][x] = [0 <= raw <= 1] m [image_bg <= 1] sum_i dL/dpred[k n + i][c][y - oy_i][x - ox_i] over the patches of frame
// k that contain the pixel, in patch order (overlaps summed in a fixed order, no atomics)
__global__ void __launch_bounds__(256) lp_patch_scatter(int K, int n, int P, int H, int W, const float *__restrict__ raw,
                                                        const float *__restrict__ mask, const float *__restrict__ bg_rand,
                                                        const int32_t *__restrict__ origins, const float *__restrict__ gp,
                                                        float *__restrict__ draw)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (idx >= K * 3 * HW) return;
    const int k = idx / (3 * HW), rr = idx - k * 3 * HW, c = rr / HW, pix = rr - c * HW;
    const int y = pix / W, x = pix - y * W;
    const int PP = P * P;
    float acc = 0.0f;
    for (int i = 0; i < n; i++) {
        const int patch = k * n + i;
        const int oy = lp_clampi(origins[2 * patch], H - P), ox = lp_clampi(origins[2 * patch + 1], W - P);
        const int u = y - oy, v = x - ox;
        if (u >= 0 && u < P && v >= 0 && v < P) acc += gp[((size_t)patch * 3 + c) * PP + u * P + v];
    }
    const float rv = raw[idx], m = mask[(size_t)k * HW + pix];
    const float img = lp_clamp01(rv) * m + bg_rand[idx] * (1.0f - m);
    float d = img <= 1.0f ? acc : 0.0f;
    d = d * m;
    draw[idx] = (rv >= 0.0f && rv <= 1.0f) ? d : 0.0f;
}

inline unsigned lp_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

void lp_conv(bool bwd, int NI, int H, int W, int CI, int CO, const float *X, const float *S, const float *Wp, const float *bias,
             float *Y, hipStream_t st)
{
    const int tpi = (H * W + 63) / 64;
    const dim3 grid(tpi * NI, CO / 64);
    if (bwd) hipLaunchKernelGGL(lp_conv3x3<true>, grid, dim3(256), 0, st, H, W, CI, CO, tpi, X, S, Wp, bias, Y);
    else hipLaunchKernelGGL(lp_conv3x3<false>, grid, dim3(256), 0, st, H, W, CI, CO, tpi, X, S, Wp, bias, Y);
}

}  // namespace

extern "C" int sg_lpips_weights_layout(size_t *offsets, size_t *total_floats)
{
    if (!offsets || !total_floats) return sg_set_error("sg_lpips_weights_layout: null pointer");
    const LpWeights w = lp_weights();
    for (int i = 0; i < SG_LPIPS_NUM_OFFSETS; i++) offsets[i] = w.off[i];
    *total_floats = w.total;
    return 0;
}

extern "C" int sg_lpips_ws_bytes(int B, int height, int width, size_t *bytes)
{
    LpPlan p;
    if (!bytes) return sg_set_error("sg_lpips_ws_bytes: null pointer");
    if (!lp_plan(B, height, width, p)) return sg_set_error("sg_lpips_ws_bytes: B must be >= 1, H and W >= 16 (and 2 B H W 64 < 2^31)");
    *bytes = p.total;
    return 0;
}

extern "C" int sg_lpips_ws_layout(int B, int height, int width, size_t *offsets, size_t *total_bytes)
{
    LpPlan p;
    if (!offsets || !total_bytes) return sg_set_error("sg_lpips_ws_layout: null pointer");
    if (!lp_plan(B, height, width, p)) return sg_set_error("sg_lpips_ws_layout: B must be >= 1, H and W >= 16 (and 2 B H W 64 < 2^31)");
    size_t *o = offsets;                                                    // y_0..12, pool_0..3, arg_0..3, dpix_0..4, g_0..1
    for (int l = 0; l < LP_NCONV; l++) *o++ = p.y[l];
    for (int q = 0; q < 4; q++) *o++ = p.pool[q];
    for (int q = 0; q < 4; q++) *o++ = p.arg[q];
    for (int k = 0; k < 5; k++) *o++ = p.dpix[k];
    for (int i = 0; i < 2; i++) *o++ = p.g[i];
    *total_bytes = p.total;
    return 0;
}

extern "C" int sg_lpips_forward(int B, int height, int width, int normalize, const float *packed, const float *in0, const float *in1,
                                void *ws, float *out, void *stream)
{
    LpPlan p;
    if (!lp_plan(B, height, width, p)) return sg_set_error("sg_lpips_forward: B must be >= 1, H and W >= 16 (and 2 B H W 64 < 2^31)");
    if (!packed || !in0 || !in1 || !ws || !out) return sg_set_error("sg_lpips_forward: null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const LpWeights w = lp_weights();
    char *base = (char *)ws;
    auto Y = [&](int l) { return (float *)(base + p.y[l]); };
    const int NI = 2 * B;
    hipLaunchKernelGGL(lp_conv1_fwd, dim3(lp_blocks((size_t)NI * height * width * 64)), dim3(256), 0, st, B, height, width, normalize,
                       in0, in1, packed + w.off[0], packed + w.off[1], packed + w.off[3 * LP_NCONV + 5],
                       packed + w.off[3 * LP_NCONV + 6], Y(0));
    const float *x = Y(0);
    for (int l = 1; l < LP_NCONV; l++) {
        const int v = lp_level[l];
        if (lp_level[l - 1] != v) {                                        // MaxPool2d in front of slices 2..5
            const int qd = v - 1, Hi = p.H[qd], Wi = p.W[qd], C = lp_cin[l];
            hipLaunchKernelGGL(lp_pool_fwd, dim3(lp_blocks((size_t)NI * p.H[v] * p.W[v] * C)), dim3(256), 0, st, NI, Hi, Wi, C, x,
                               (float *)(base + p.pool[qd]), (uint8_t *)(base + p.arg[qd]));
            x = (const float *)(base + p.pool[qd]);
        }
        lp_conv(false, NI, p.H[v], p.W[v], lp_cin[l], lp_cout[l], x, nullptr, packed + w.off[3 * l], packed + w.off[3 * l + 1], Y(l), st);
        x = Y(l);
    }
    LpSlices s;
    for (int k = 0; k < 5; k++) {
        const int hw = p.H[k] * p.W[k];
        float *d = (float *)(base + p.dpix[k]);
        hipLaunchKernelGGL(lp_head_fwd, dim3(lp_blocks((size_t)B * hw * 64)), dim3(256), 0, st, B, hw, lp_slice_ch[k],
                           Y(lp_slice_layer[k]), packed + w.off[3 * LP_NCONV + k], d);
        s.dpix[k] = d; s.hw[k] = hw;
    }
    hipLaunchKernelGGL(lp_head_reduce, dim3(B), dim3(256), 0, st, s, out);
    return sg_launched("sg_lpips_forward");
}

extern "C" int sg_lpips_backward(int B, int height, int width, int normalize, const float *packed, const void *ws_c,
                                 const float *dL_dout, float *dL_din0, void *stream)
{
    LpPlan p;
    if (!lp_plan(B, height, width, p)) return sg_set_error("sg_lpips_backward: B must be >= 1, H and W >= 16 (and 2 B H W 64 < 2^31)");
    if (!packed || !ws_c || !dL_dout || !dL_din0) return sg_set_error("sg_lpips_backward: null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const LpWeights w = lp_weights();
    char *base = (char *)ws_c;                                             // (the gradient buffers and the pool argmax live in it)
    auto Y = [&](int l) { return (const float *)(base + p.y[l]); };
    float *gbuf[2] = { (float *)(base + p.g[0]), (float *)(base + p.g[1]) };
    int cur = 0;                                                           // gbuf[cur]: the gradient at the current activation
    int slice = 4;
    auto head = [&](int k, int accum) {
        const int hw = p.H[k] * p.W[k];
        hipLaunchKernelGGL(lp_head_bwd, dim3(lp_blocks((size_t)B * hw * 64)), dim3(256), 0, st, B, hw, lp_slice_ch[k],
                           Y(lp_slice_layer[k]), packed + w.off[3 * LP_NCONV + k], dL_dout, accum, gbuf[cur]);
    };
    head(slice, 0);
    for (int l = LP_NCONV - 1; l >= 1; l--) {
        const int v = lp_level[l];
        // gradient at conv l's input = conv(select(y_l > 0, g), W'_l)
        lp_conv(true, B, p.H[v], p.W[v], lp_cout[l], lp_cin[l], gbuf[cur], Y(l), packed + w.off[3 * l + 2], nullptr, gbuf[cur ^ 1], st);
        cur ^= 1;
        if (lp_level[l - 1] != v) {                                        // through the pool to the previous slice's output
            const int qd = v - 1, C = lp_cin[l];
            hipLaunchKernelGGL(lp_pool_bwd, dim3(lp_blocks((size_t)B * p.H[qd] * p.W[qd] * C)), dim3(256), 0, st, B, p.H[qd], p.W[qd],
                               C, gbuf[cur], (const uint8_t *)(base + p.arg[qd]), gbuf[cur ^ 1]);
            cur ^= 1;
            head(--slice, 1);
        }
    }
    hipLaunchKernelGGL(lp_conv1_bwd, dim3(lp_blocks((size_t)B * 3 * height * width)), dim3(256), 0, st, B, height, width, normalize,
                       Y(0), gbuf[cur], packed + w.off[0], packed + w.off[3 * LP_NCONV + 6], dL_din0);
    return sg_launched("sg_lpips_backward");
}

extern "C" int sg_lpips_patch_gather(int K, int n, int patch, int height, int width, const float *raw, const float *gt_rgb,
                                     const float *mask, const float *bg, const float *bg_rand, const int32_t *origins,
                                     float *pred_patches, float *gt_patches, void *stream)
{
    if (K < 1 || n < 1 || patch < 1 || patch > height || patch > width || (double)K * 3 * height * width >= 2147483647.0 ||
        (double)K * n * 3 * patch * patch >= 2147483647.0)
        return sg_set_error("sg_lpips_patch_gather: bad sizes (K, n >= 1, 1 <= patch <= H, W)");
    if (!raw || !gt_rgb || !mask || !bg || !bg_rand || !origins || !pred_patches || !gt_patches)
        return sg_set_error("sg_lpips_patch_gather: null pointer");
    hipLaunchKernelGGL(lp_patch_gather, dim3(lp_blocks((size_t)K * n * 3 * patch * patch)), dim3(256), 0, (hipStream_t)stream, K, n,
                       patch, height, width, raw, gt_rgb, mask, bg, bg_rand, origins, pred_patches, gt_patches);
    return sg_launched("sg_lpips_patch_gather");
}

extern "C" int sg_lpips_patch_scatter(int K, int n, int patch, int height, int width, const float *raw, const float *mask,
                                      const float *bg_rand, const int32_t *origins, const float *dL_dpred_patches, float *dL_draw,
                                      void *stream)
{
    if (K < 1 || n < 1 || patch < 1 || patch > height || patch > width || (double)K * 3 * height * width >= 2147483647.0 ||
        (double)K * n * 3 * patch * patch >= 2147483647.0)
        return sg_set_error("sg_lpips_patch_scatter: bad sizes (K, n >= 1, 1 <= patch <= H, W)");
    if (!raw || !mask || !bg_rand || !origins || !dL_dpred_patches || !dL_draw) return sg_set_error("sg_lpips_patch_scatter: null pointer");
    hipLaunchKernelGGL(lp_patch_scatter, dim3(lp_blocks((size_t)K * 3 * height * width)), dim3(256), 0, (hipStream_t)stream, K, n,
                       patch, height, width, raw, mask, bg_rand, origins, dL_dpred_patches, dL_draw);
    return sg_launched("sg_lpips_patch_scatter");
}
