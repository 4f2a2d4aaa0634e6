// The training frames on the device (include/sings_feed.h states the rule; sings_amd/frame_feed.py holds its numpy twins).
//
// sg_frame_draw: one workgroup picks the step's K frames (and its background colour) from the counter in `state`.  The order of an
// epoch is a Fisher-Yates shuffle of the identity: the swap partners are Philox words, computed by the whole workgroup a batch at a
// time, and the swaps themselves -- a dependent chain -- are done by one lane in LDS (16-bit entries: F <= 16384).  That chain runs
// once per epoch, i.e. once per F draws; every other call reads K entries of the order kept in global memory.
//
// sg_frame_expand: byte-bound, 4 B read and 16 B written per pixel.  A thread takes 4 consecutive pixels of one frame: one 16-byte
// load of their 16 interleaved bytes (a wave reads a contiguous 1-KB run) and one 16-byte store into each of the four planes (a
// wave writes four contiguous 1-KB runs).  When H*W is not a multiple of 4 (or a pointer is not aligned for that) a thread takes one
// pixel instead: one dword in, four coalesced dword stores out.
#include "sg_host.h"
#include "../../include/sings_feed.h"
#include "sg_philox.h"

#define FD_BLOCK 256
#define FD_BATCH (4 * FD_BLOCK)          // swap partners per batch: one Philox block (four words) per thread

// sA (the order of epoch e, 16-bit) from the identity; every thread of the workgroup calls it, and sees sA complete on return
__device__ __forceinline__ void fd_build_order(uint32_t F, uint64_t e, uint32_t k0, uint32_t k1, uint16_t *sA, uint16_t *sJ)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < F; i += FD_BLOCK) sA[i] = (uint16_t)i;
    // step s = 0 .. F-2 swaps a[i] and a[j] with i = F-1-s, j = bounded(word_0(e, s), i + 1)
    for (uint32_t base = 0; base + 1u < F; base += FD_BATCH) {
        const uint32_t ctr[4] = { (uint32_t)e, (uint32_t)(e >> 32), 0u, base / 4u + tid };
        uint32_t w[4];
        sg_philox4x32(ctr, k0, k1, w);
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t s = base + 4u * tid + u;
            if (s + 1u < F) sJ[4u * tid + u] = (uint16_t)sg_bounded(w[u], F - s);             // (i + 1 = F - s)
        }
        __syncthreads();                                                                      // (the identity too, in the first batch)
        if (tid == 0) {
            const uint32_t n = F - 1u - base < FD_BATCH ? F - 1u - base : FD_BATCH;
            for (uint32_t q = 0; q < n; q++) {
                const uint32_t i = F - 1u - base - q, j = sJ[q];
                const uint16_t ai = sA[i], aj = sA[j];
                sA[i] = aj; sA[j] = ai;
            }
        }
        __syncthreads();
    }
    __syncthreads();                                                                          // (F = 1: no batch, no barrier above)
}

__global__ void __launch_bounds__(FD_BLOCK)
sg_frame_draw_kernel(uint32_t F, int K, int draw_bg, int64_t *__restrict__ state, int32_t *__restrict__ order,
                     int32_t *__restrict__ idx_out, float *__restrict__ bg_out)
{
    __shared__ uint16_t sA[SG_FEED_MAX_FRAMES], sJ[FD_BATCH];
    const uint32_t tid = threadIdx.x;
    const uint64_t c = (uint64_t)state[0], seed = (uint64_t)state[1];
    int64_t held = state[2];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    bool in_lds = false;                                                 // sA holds epoch `held` (uniform over the workgroup)
    for (int k = 0; k < K; k++) {
        const uint64_t t = c + (uint64_t)k, e = t / F;
        const uint32_t pos = (uint32_t)(t % F);
        if ((int64_t)e != held) {
            fd_build_order(F, e, k0, k1, sA, sJ);
            for (uint32_t i = tid; i < F; i += FD_BLOCK) order[i] = (int32_t)sA[i];
            held = (int64_t)e;
            in_lds = true;
        }
        if (tid == 0) idx_out[k] = in_lds ? (int32_t)sA[pos] : order[pos];
        __syncthreads();                                                 // (sA is read before the next epoch overwrites it)
    }
    if (tid == 0) {                                                      // (every thread has read the state: the barrier above, K >= 1)
        if (draw_bg) {
            const uint32_t ctr[4] = { (uint32_t)c, (uint32_t)(c >> 32), 1u, 0u };
            uint32_t w[4];
            sg_philox4x32(ctr, k0, k1, w);
            for (int i = 0; i < 3; i++) bg_out[i] = (float)(w[i] >> 8) * 0x1p-24f;            // (24 bits: exact)
        }
        state[0] = (int64_t)(c + (uint64_t)K);
        state[2] = held;
        state[3] = (int64_t)c;
    }
}

#define FE_THREADS 256

// grid: (ceil(ceil(HW / PIX) / 256), K) with PIX = 4 (VEC) or 1; frame blockIdx.y of the step, its pixels PIX t .. PIX t + PIX - 1
template <bool VEC>
__global__ void __launch_bounds__(FE_THREADS)
sg_frame_expand_kernel(size_t HW, int F, const uint8_t *__restrict__ store, const int32_t *__restrict__ idx, float *__restrict__ gt,
                       float *__restrict__ mask)
{
    const size_t t = (size_t)blockIdx.x * FE_THREADS + threadIdx.x, p0 = (VEC ? 4 : 1) * t;
    if (p0 >= HW) return;
    const size_t k = blockIdx.y;
    int f = idx[k];
    f = f < 0 ? 0 : f >= F ? F - 1 : f;
    const uint8_t *src = store + ((size_t)f * HW + p0) * 4;
    float *g = gt + k * 3 * HW + p0, *m = mask + k * HW + p0;
    if (VEC) {                                        // HW % 4 == 0: p0 + 3 < HW; every pointer 16-B aligned (host check)
        const uint4 v = *(const uint4 *)src;
        const uint32_t px[4] = { v.x, v.y, v.z, v.w };
        float o[4][4];                                // [channel][pixel]
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int ch = 0; ch < 4; ch++) o[ch][i] = (float)((px[i] >> (8 * ch)) & 0xffu) / 255.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) *(float4 *)(g + ch * HW) = make_float4(o[ch][0], o[ch][1], o[ch][2], o[ch][3]);
        *(float4 *)m = make_float4(o[3][0], o[3][1], o[3][2], o[3][3]);
    } else {
        const uint32_t v = *(const uint32_t *)src;    // (a pixel's four bytes: 4-B aligned with the store)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) g[ch * HW] = (float)((v >> (8 * ch)) & 0xffu) / 255.0f;
        m[0] = (float)(v >> 24) / 255.0f;
    }
}

extern "C" int sg_frame_draw(int F, int K, int draw_bg, int64_t *state, int32_t *order, int32_t *idx_out, float *bg_out, void *stream)
{
    const char *who = "sg_frame_draw";
    if (F < 1 || F > SG_FEED_MAX_FRAMES) return sg_failf("%s: F = %d outside 1..%d", who, F, SG_FEED_MAX_FRAMES);
    if (K < 1 || K > SG_FEED_MAX_K) return sg_failf("%s: K = %d outside 1..%d", who, K, SG_FEED_MAX_K);
    if (!state || !order || !idx_out) return sg_failf("%s: null pointer", who);
    if (draw_bg && !bg_out) return sg_failf("%s: draw_bg without bg_out", who);
    hipLaunchKernelGGL(sg_frame_draw_kernel, dim3(1), dim3(FD_BLOCK), 0, (hipStream_t)stream, (uint32_t)F, K, draw_bg ? 1 : 0, state,
                       order, idx_out, bg_out);
    return sg_launched(who);
}

extern "C" int sg_frame_expand(int K, int H, int W, int F, const uint8_t *store, const int32_t *idx, float *gt, float *mask,
                               void *stream)
{
    const char *who = "sg_frame_expand";
    if (K < 1 || K > SG_FEED_MAX_K) return sg_failf("%s: K = %d outside 1..%d", who, K, SG_FEED_MAX_K);
    if (H < 1 || W < 1) return sg_failf("%s: a %d x %d image has no pixel", who, H, W);
    if ((uint64_t)H * (uint64_t)W >= (1ull << 31)) return sg_failf("%s: a %d x %d image has 2^31 pixels or more", who, H, W);
    if (F < 1) return sg_failf("%s: F = %d, at least one frame is needed", who, F);
    if (!store || !idx || !gt || !mask) return sg_failf("%s: null pointer", who);
    const size_t HW = (size_t)H * (size_t)W;
    const bool vec = HW % 4 == 0 && (((uintptr_t)store | (uintptr_t)gt | (uintptr_t)mask) & 15) == 0;
    const size_t threads = vec ? HW / 4 : HW, blocks = (threads + FE_THREADS - 1) / FE_THREADS;
    dim3 grid((unsigned)blocks, (unsigned)K), block(FE_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(sg_frame_expand_kernel<true>, grid, block, 0, st, HW, F, store, idx, gt, mask);
    else hipLaunchKernelGGL(sg_frame_expand_kernel<false>, grid, block, 0, st, HW, F, store, idx, gt, mask);
    return sg_launched(who);
}
