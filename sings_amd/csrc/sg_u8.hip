// Frames out as 8-bit HWC (sg_frames_to_u8): the last step of the reference's animation loop, gs_trainer.py:717-719 --
// `(clamp(x, 0, 1) * 255).astype(uint8)` on the host, then cvtColor to BGR -- as one launch over K planar fp32 frames.
//
// Byte-bound: 12 bytes read and 3 written per pixel.  A thread takes 4 consecutive pixels of one frame: one 16-byte load from each
// of the three planes (a wave reads three contiguous 1-KB runs) and three 4-byte stores of the 12 interleaved bytes (a contiguous
// 768-B run per wave).  When the plane size is not a multiple of 4 pixels (or a pointer is not aligned for that) the same thread
// shape reads scalars and writes single bytes.
#include "sg_host.h"

#define SG_U8_THREADS 256

__device__ __forceinline__ uint32_t sg_to_u8(float x)
{
    const float v = fminf(fmaxf(x, 0.0f), 1.0f);      // (maxnum: NaN -> 0)
    return (uint32_t)(uint8_t)(v * 255.0f);           // one fp32 multiply (-ffp-contract=off), truncation
}

// grid: (ceil(ceil(HW / 4) / 256), K); frame blockIdx.y, pixels 4 t .. 4 t + 3 of its HW
template <bool VEC>
__global__ void __launch_bounds__(SG_U8_THREADS)
sg_frames_to_u8_kernel(size_t HW, const float *__restrict__ rgb, int bgr, uint8_t *__restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * SG_U8_THREADS + threadIdx.x, p0 = 4 * t;
    if (p0 >= HW) return;
    const size_t f = blockIdx.y;
    const float *src = rgb + f * 3 * HW;
    uint8_t *dst = out + (f * HW + p0) * 3;
    const int c0 = bgr ? 2 : 0, c2 = bgr ? 0 : 2;     // plane written first / last
    if (VEC) {                                        // HW % 4 == 0: p0 + 3 < HW; planes 16-B and dst 4-B aligned (host check)
        const float4 a = *(const float4 *)(src + c0 * HW + p0);
        const float4 b = *(const float4 *)(src + HW + p0);
        const float4 c = *(const float4 *)(src + c2 * HW + p0);
        uint32_t *d = (uint32_t *)dst;
        d[0] = sg_to_u8(a.x) | sg_to_u8(b.x) << 8 | sg_to_u8(c.x) << 16 | sg_to_u8(a.y) << 24;
        d[1] = sg_to_u8(b.y) | sg_to_u8(c.y) << 8 | sg_to_u8(a.z) << 16 | sg_to_u8(b.z) << 24;
        d[2] = sg_to_u8(c.z) | sg_to_u8(a.w) << 8 | sg_to_u8(b.w) << 16 | sg_to_u8(c.w) << 24;
    } else {
        const size_t n = HW - p0 < 4 ? HW - p0 : 4;
        for (size_t i = 0; i < n; i++) {
            dst[3 * i] = (uint8_t)sg_to_u8(src[c0 * HW + p0 + i]);
            dst[3 * i + 1] = (uint8_t)sg_to_u8(src[HW + p0 + i]);
            dst[3 * i + 2] = (uint8_t)sg_to_u8(src[c2 * HW + p0 + i]);
        }
    }
}

extern "C" int sg_frames_to_u8(int K, int width, int height, const float *rgb, int bgr, uint8_t *out, void *stream)
{
    if (K < 1 || K > 65535) return sg_set_error("sg_frames_to_u8: K must be 1..65535", hipSuccess);
    if (width < 1 || height < 1) return sg_set_error("sg_frames_to_u8: width and height must be >= 1", hipSuccess);
    if (!rgb || !out) return sg_set_error("sg_frames_to_u8: null pointer", hipSuccess);
    const size_t HW = (size_t)width * (size_t)height, threads = (HW + 3) / 4, blocks = (threads + SG_U8_THREADS - 1) / SG_U8_THREADS;
    if (blocks > 0x7fffffffu) return sg_set_error("sg_frames_to_u8: image too large", hipSuccess);
    const bool vec = HW % 4 == 0 && ((uintptr_t)rgb & 15) == 0 && ((uintptr_t)out & 3) == 0;
    dim3 grid((unsigned)blocks, (unsigned)K), block(SG_U8_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(sg_frames_to_u8_kernel<true>, grid, block, 0, st, HW, rgb, bgr ? 1 : 0, out);
    else hipLaunchKernelGGL(sg_frames_to_u8_kernel<false>, grid, block, 0, st, HW, rgb, bgr ? 1 : 0, out);
    return sg_launched("sg_frames_to_u8");
}
