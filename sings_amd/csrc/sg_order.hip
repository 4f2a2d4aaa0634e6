// The work order of a K-camera launch (include/sings_order.h): Morton codes of the Gaussians' positions.  Off the hot path -- an
// order is built once per change of the Gaussian set -- so the bounding box is one workgroup walking the array.
#include "sg_host.h"
#include "../../include/sings_order.h"

// box[0..2] = min, box[3..5] = max per axis; fminf / fmaxf ignore a NaN operand
__global__ void __launch_bounds__(1024)
sg_order_box_kernel(int P, const float *__restrict__ means3D, float *__restrict__ box)
{
    __shared__ float sLo[3][1024 / SG_WAVE], sHi[3][1024 / SG_WAVE];
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int i = threadIdx.x; i < P; i += 1024)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = means3D[3 * (size_t)i + k];
            lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v);
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], s, 64));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], s, 64));
        }
        if (lane == 0) { sLo[k][wave] = lo[k]; sHi[k][wave] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        float a = sLo[k][0], b = sHi[k][0];
        for (int w = 1; w < 1024 / SG_WAVE; w++) { a = fminf(a, sLo[k][w]); b = fmaxf(b, sHi[k][w]); }
        box[k] = a; box[3 + k] = b;
    }
}

__device__ __forceinline__ uint32_t sg_spread10(uint32_t v)          // bit b of v -> bit 3 b
{
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__global__ void __launch_bounds__(256)
sg_order_codes_kernel(int P, const float *__restrict__ means3D, const float *__restrict__ box, uint32_t *__restrict__ codes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint32_t code = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = box[k], ext = fmaxf(box[3 + k] - lo, 1e-12f);
        const float q = (means3D[3 * (size_t)i + k] - lo) * (1023.0f / ext);
        const uint32_t cell = q >= 1023.0f ? 1023u : q > 0.0f ? (uint32_t)q : 0u;      // (NaN: 0)
        code |= sg_spread10(cell) << k;
    }
    codes[i] = code;
}

void sg_launch_morton_codes(int P, const float *means3D, float *box, uint32_t *codes, hipStream_t st)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(sg_order_box_kernel, dim3(1), dim3(1024), 0, st, P, means3D, box);
    hipLaunchKernelGGL(sg_order_codes_kernel, dim3((P + 255) / 256), dim3(256), 0, st, P, means3D, box, codes);
}
