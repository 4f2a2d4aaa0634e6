// The fixed-order sum tail of the regularisers (sg_reg.hip), the k-NN edge loss (sg_knn.hip) and the fused mesh terms
// (sg_mesh_terms.hip): per-block partial sums, then one 256-thread workgroup that adds them in double in a fixed order.  No float
// atomics: two runs give the same bits.
#pragma once
#include "sg_common.h"

#define SG_RED_MAXQ 8
// block partial sums -> partial[blockIdx.x][q]; every thread passes its NQ values
template <int NQ>
__device__ __forceinline__ void sg_block_partials(float v[NQ], float *__restrict__ partial)
{
    __shared__ float sRed[4][SG_RED_MAXQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; q++) sRed[wave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        float t = 0.0f;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += sRed[w][threadIdx.x];
        partial[(size_t)blockIdx.x * SG_RED_MAXQ + threadIdx.x] = t;
    }
}

// sums[q] = sum over blocks of partial[b][q] in double, fixed order (one 256-thread workgroup)
__device__ __forceinline__ void sg_final_sums(const float *__restrict__ partial, int nblocks, int nq, double *sums /* LDS [SG_RED_MAXQ] */)
{
    __shared__ double sR[256];
    for (int q = 0; q < nq; q++) {
        double t = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += 256) t += (double)partial[(size_t)i * SG_RED_MAXQ + q];
        sR[threadIdx.x] = t;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sR[threadIdx.x] += sR[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[q] = sR[0];
        __syncthreads();
    }
}

// workgroups of 256 over n items, at least one (the partials of an empty input are one block of zeros)
static inline int sg_nb(int n) { return (n + 255) / 256 > 0 ? (n + 255) / 256 : 1; }

// out[0] = scale * sum of partial[0, nblocks)[0]   (sg_scalar_reduce_kernel, sg_reg.hip)
void sg_launch_scalar_reduce(const float *partial, int nblocks, float scale, float *out, hipStream_t st);

// the cotangent Laplacian's launcher (sg_reg.hip), called from sg_api_ops.hip
void sg_launch_rows_laplacian(int R, int V, int C, const float *x, const int *row_ptr, const int *col, const float *val,
                              const float *rscale, const int *t_row_ptr, const int *t_row, const float *t_val, void *ws, float *g_ws,
                              float *loss, const float *upstream, float *dL_dx, hipStream_t st);
