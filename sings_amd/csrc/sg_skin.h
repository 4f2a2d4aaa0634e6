// What the LBS-fused per-Gaussian kernels (sg_skin.hip) and the stand-alone lbs_extra (sg_lbs.hip) share: the workgroup shape
// (four waves of 64 Gaussians), the joint limit, and the staging of a wave's skinning-weight rows into LDS.
#pragma once
#include "sg_common.h"

#define SG_SKIN_THREADS 256
#define SG_SKIN_WAVES 4
#define SG_JMAX 64
#define SG_WSTRIDE 17

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- W . A on the matrix cores -----------------------------------------------------------
// Stages joints [16c, 16c+16) of the wave's 64 skinning-weight rows into sW[64][17] (zero padded).
__device__ __forceinline__ void sg_stage_w_chunk(const float *__restrict__ W, int J, int P, int g0, int c, int lane,
                                                 float *__restrict__ sW)
{
    if ((J & 3) == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int row = i * 16 + (lane >> 2), col = c * 16 + 4 * (lane & 3);
            float4 v = make_float4(0, 0, 0, 0);
            if (g0 + row < P && col < J) v = *(const float4 *)(W + (size_t)(g0 + row) * J + col);
            float *d = sW + row * SG_WSTRIDE + 4 * (lane & 3);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            int row = i * 4 + (lane >> 4), col = c * 16 + (lane & 15);
            float v = 0.0f;
            if (g0 + row < P && col < J) v = W[(size_t)(g0 + row) * J + col];
            sW[row * SG_WSTRIDE + (lane & 15)] = v;
        }
    }
}

// the same in two halves (J % 4 == 0): issue the loads of a chunk / put them into LDS -- the chunk loops below keep the
// next chunk's loads in flight while the matrix cores work on the current one
__device__ __forceinline__ void sg_w_fetch(const float *__restrict__ W, int J, int P, int g0, int c, int lane, float4 v[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = i * 16 + (lane >> 2), col = c * 16 + 4 * (lane & 3);
        v[i] = make_float4(0, 0, 0, 0);
        if (g0 + row < P && col < J) v[i] = *(const float4 *)(W + (size_t)(g0 + row) * J + col);
    }
}
__device__ __forceinline__ void sg_w_stash(const float4 v[4], int lane, float *__restrict__ sW)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float *d = sW + (i * 16 + (lane >> 2)) * SG_WSTRIDE + 4 * (lane & 3);
        d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
    }
}
