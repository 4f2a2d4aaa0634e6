// Frames out as finished 8-bit sheets (sg_image_sheets; include/sings_sheet.h states the layout and both quantisation rules,
// tests/sheet_case.py holds the numpy restatement): K planar fp32 frames tiled make_grid-fashion, quantised and interleaved to HWC
// bytes in one launch -- the training picture, the validation grids, the turntable frames and the progress sheet of a run.
//
// Byte-bound: 12 bytes read and 3 written per tile pixel, 3 written per border pixel.  The launch is laid out over the OUTPUT: a
// thread takes 4 consecutive pixels of one sheet (rows run on: the 4 may cross a row end, a tile edge or the border), so its 12
// bytes are three 4-byte stores whenever the sheet's base is 4-byte aligned -- whatever the padding, which puts a tile's first
// pixel 3 * padding bytes into a sheet row.  The loads follow from there: when the 4 pixels lie in one tile row and that address
// is 16-byte aligned (padding 0 and W % 4 == 0: every frame of a turntable, the training picture), one 16-byte load per plane as in
// sg_u8.hip; elsewhere four scalar loads per plane, which a wave still issues over one contiguous run.  One 32-bit division pair per
// thread for the row and one for the column; the other three pixels step from the first.
#include "sg_host.h"
#include "../../include/sings_sheet.h"

struct SgSheetGeo {
    int W, H, pad, T, xmaps, ymaps, Ws, pair;
    uint32_t npix;                                    // Hs * Ws < 2^31
    size_t HW;
};

template <int QUANT>
__device__ __forceinline__ uint32_t sg_sheet_q(float x)
{
    if (QUANT == SG_SHEET_TRUNC) {
        const float v = fminf(fmaxf(x, 0.0f), 1.0f);              // (maxnum: NaN -> 0)
        return (uint32_t)(uint8_t)(v * 255.0f);
    }
    const float v = x * 255.0f + 0.5f;                            // two roundings (-ffp-contract=off)
    return (uint32_t)(uint8_t)fminf(fmaxf(v, 0.0f), 255.0f);
}

template <int QUANT>
__device__ __forceinline__ uint32_t sg_sheet_rgb(float r, float g, float b, int bgr)
{
    const uint32_t q0 = sg_sheet_q<QUANT>(r), q1 = sg_sheet_q<QUANT>(g), q2 = sg_sheet_q<QUANT>(b);
    return bgr ? (q2 | q1 << 8 | q0 << 16) : (q0 | q1 << 8 | q2 << 16);
}

// grid: (ceil(ceil(npix / 4) / 256), S); sheet blockIdx.y, pixels 4 t .. 4 t + 3 of its Hs * Ws
template <int QUANT>
__global__ void __launch_bounds__(SG_SHEET_BLOCK)
sg_image_sheets_kernel(SgSheetGeo g, float pad_value, int bgr, const float *__restrict__ a, const float *__restrict__ b,
                       const float *__restrict__ mask, uint8_t *__restrict__ out)
{
    const uint32_t t = blockIdx.x * SG_SHEET_BLOCK + threadIdx.x;
    if (t >= (g.npix + 3u) / 4u) return;
    const uint32_t r0 = 4u * t, n = g.npix - r0 < 4u ? g.npix - r0 : 4u;
    const uint32_t s = blockIdx.y;
    uint8_t *dst = out + ((size_t)s * g.npix + r0) * 3;
    const uint32_t padq = sg_sheet_rgb<QUANT>(pad_value, pad_value, pad_value, 0);
    const int cellW = g.W + g.pad, cellH = g.H + g.pad;
    int y = (int)(r0 / (uint32_t)g.Ws), x = (int)(r0 - (uint32_t)y * (uint32_t)g.Ws);
    // the row's cell and the row within its tile (negative: in the border above it); the same for the column
    int cy = y / cellH, oy = y - cy * cellH - g.pad;
    int cx = x / cellW, ox = x - cx * cellW - g.pad;
    uint32_t px[4] = {padq, padq, padq, padq};

    // frame of tile `tile` of this sheet and the tensor it comes from
    auto source = [&](int tile, size_t &f) -> const float * {
        if (g.pair) { f = (size_t)s * (size_t)(g.T / 2) + (size_t)(tile / 2); return (tile & 1) ? b : a; }
        f = (size_t)s * (size_t)g.T + (size_t)tile;
        return a;
    };

    bool done = false;
    if (n == 4u && oy >= 0 && cy < g.ymaps && ox >= 0 && ox + 3 < g.W && cx < g.xmaps && cy * g.xmaps + cx < g.T && g.HW % 4 == 0) {
        size_t f;
        const float *src = source(cy * g.xmaps + cx, f);
        const size_t off = (size_t)oy * (size_t)g.W + (size_t)ox;
        const float *p = src + f * 3 * g.HW + off;
        const float *m = mask ? mask + f * g.HW + off : nullptr;
        if ((((uintptr_t)p | (uintptr_t)m) & 15) == 0) {          // one tile row, 16-byte aligned planes (and mask row)
            float4 c0 = *(const float4 *)p, c1 = *(const float4 *)(p + g.HW), c2 = *(const float4 *)(p + 2 * g.HW);
            if (m) {
                const float4 w = *(const float4 *)m;
                c0.x *= w.x; c0.y *= w.y; c0.z *= w.z; c0.w *= w.w;
                c1.x *= w.x; c1.y *= w.y; c1.z *= w.z; c1.w *= w.w;
                c2.x *= w.x; c2.y *= w.y; c2.z *= w.z; c2.w *= w.w;
            }
            px[0] = sg_sheet_rgb<QUANT>(c0.x, c1.x, c2.x, bgr);
            px[1] = sg_sheet_rgb<QUANT>(c0.y, c1.y, c2.y, bgr);
            px[2] = sg_sheet_rgb<QUANT>(c0.z, c1.z, c2.z, bgr);
            px[3] = sg_sheet_rgb<QUANT>(c0.w, c1.w, c2.w, bgr);
            done = true;
        }
    }
    if (!done) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {                       // (fixed trip count: px[] stays in registers)
            if (i >= n) break;
            if (oy >= 0 && cy < g.ymaps && ox >= 0 && cx < g.xmaps && cy * g.xmaps + cx < g.T) {
                size_t f;
                const float *src = source(cy * g.xmaps + cx, f);
                const size_t off = (size_t)oy * (size_t)g.W + (size_t)ox;
                const float *p = src + f * 3 * g.HW + off;
                float c0 = p[0], c1 = p[g.HW], c2 = p[2 * g.HW];
                if (mask) {
                    const float w = mask[f * g.HW + off];
                    c0 *= w; c1 *= w; c2 *= w;
                }
                px[i] = sg_sheet_rgb<QUANT>(c0, c1, c2, bgr);
            }
            // the next pixel of the sheet: one column on, or the first column of the next row
            if (++x == g.Ws) {
                x = 0; cx = 0; ox = -g.pad;
                y++;
                if (++oy == g.H) { oy = -g.pad; cy++; }
            } else if (++ox == g.W) {
                ox = -g.pad; cx++;
            }
        }
    }
    if (n == 4u && ((uintptr_t)dst & 3) == 0) {
        uint32_t *d = (uint32_t *)dst;
        d[0] = px[0] | px[1] << 24;
        d[1] = px[1] >> 8 | px[2] << 16;
        d[2] = px[2] >> 16 | px[3] << 8;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            if (i >= n) break;
            dst[3 * i] = (uint8_t)px[i];
            dst[3 * i + 1] = (uint8_t)(px[i] >> 8);
            dst[3 * i + 2] = (uint8_t)(px[i] >> 16);
        }
    }
}

extern "C" int sg_image_sheets(int S, int T, int width, int height, int nrow, int padding, float pad_value, int quant, int bgr,
                               const float *a, const float *b, const float *mask, uint8_t *out, void *stream)
{
    const char *who = "sg_image_sheets";
    if (!a || !out) return sg_failf("%s: null pointer", who);
    if (S < 1 || T < 1 || width < 1 || height < 1 || nrow < 1)
        return sg_failf("%s: S = %d, T = %d, width = %d, height = %d, nrow = %d must all be >= 1", who, S, T, width, height, nrow);
    if (padding < 0) return sg_failf("%s: padding = %d is negative", who, padding);
    if (quant != SG_SHEET_TRUNC && quant != SG_SHEET_ROUND) return sg_failf("%s: unknown quant %d", who, quant);
    if (b && (T & 1)) return sg_failf("%s: T = %d is odd with a second tensor (the pair form takes tiles two by two)", who, T);
    if (S > SG_SHEET_MAX_SHEETS) return sg_failf("%s: S = %d sheets, at most %d per launch", who, S, SG_SHEET_MAX_SHEETS);
    const int xmaps = nrow < T ? nrow : T, ymaps = (T + xmaps - 1) / xmaps;
    const uint64_t Hs = (uint64_t)ymaps * ((uint64_t)height + (uint64_t)padding) + (uint64_t)padding;
    const uint64_t Ws = (uint64_t)xmaps * ((uint64_t)width + (uint64_t)padding) + (uint64_t)padding;
    if (Hs >= (1ull << 31) || Ws >= (1ull << 31) || Hs * Ws >= (1ull << 31))
        return sg_failf("%s: a sheet of %llu x %llu pixels, at most 2^31 - 1 per sheet", who, (unsigned long long)Ws,
                        (unsigned long long)Hs);
    SgSheetGeo g;
    g.W = width; g.H = height; g.pad = padding; g.T = T; g.xmaps = xmaps; g.ymaps = ymaps; g.Ws = (int)Ws; g.pair = b ? 1 : 0;
    g.npix = (uint32_t)(Hs * Ws);
    g.HW = (size_t)width * (size_t)height;
    const uint32_t threads = (g.npix + 3u) / 4u, blocks = (threads + SG_SHEET_BLOCK - 1) / SG_SHEET_BLOCK;
    dim3 grid(blocks, (unsigned)S), block(SG_SHEET_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    if (quant == SG_SHEET_TRUNC)
        hipLaunchKernelGGL(sg_image_sheets_kernel<SG_SHEET_TRUNC>, grid, block, 0, st, g, pad_value, bgr ? 1 : 0, a, b, mask, out);
    else
        hipLaunchKernelGGL(sg_image_sheets_kernel<SG_SHEET_ROUND>, grid, block, 0, st, g, pad_value, bgr ? 1 : 0, a, b, mask, out);
    return sg_launched(who);
}
