// Exclusive scan of n uint32 entries in three steps: 1024 entries per block, block sums, the sums scanned by one workgroup.
// prefix(i) = out[i] + bsum[i >> 10].  Device bodies only: the kernels are in the files that launch them (the k-NN cells of
// sg_knn.hip, the row / flag / unique-count scans of sg_mesh.hip, the key counters of the tri-plane sort in sg_decode.hip).
#pragma once
#include "sg_common.h"

// inclusive scan of v over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T sg_wave_incl_scan(T v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
    return v;
}

// step 1, a workgroup of 256, four entries per thread: out[i] = the sum of the entries in front of i within its block of 1024,
// bsum[blockIdx.x] = the block's sum.  value(i) is entry i.  Workgroups beyond n return (uniformly).
template <typename Value>
__device__ __forceinline__ void sg_scan_block(int n, Value value, uint32_t *__restrict__ out, uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t sW[4];
    if ((long long)blockIdx.x * 1024 >= n) return;
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = base + k < n ? value(base + k) : 0u; s += v[k]; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = sg_wave_incl_scan(s, lane);
    if (lane == 63) sW[wave] = incl;
    __syncthreads();
    uint32_t off = 0;
    for (int w = 0; w < wave; w++) off += sW[w];
    uint32_t ex = off + incl - s;
#pragma unroll
    for (int k = 0; k < 4; k++) { if (base + k < n) out[base + k] = ex; ex += v[k]; }
    if (threadIdx.x == 255) bsum[blockIdx.x] = ex;
}

// step 2, ONE workgroup of 1024: the block sums of n entries scanned in place, serially over chunks of 1024 sums with a carry.
// Returns the sum of all entries (to every thread).
__device__ __forceinline__ uint32_t sg_scan_block_sums(int n, uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t sW[16];
    __shared__ uint32_t carry;
    const int nb = (int)(((long long)n + 1023) / 1024);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const uint32_t v = i < nb ? bsum[i] : 0u;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint32_t incl = sg_wave_incl_scan(v, lane);
        if (lane == 63) sW[wave] = incl;
        __syncthreads();
        uint32_t off = carry;
        for (int w = 0; w < wave; w++) off += sW[w];
        if (i < nb) bsum[i] = off + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = off + incl;
        __syncthreads();
    }
    return carry;
}
