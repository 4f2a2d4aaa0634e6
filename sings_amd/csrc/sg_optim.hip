// The Adam step of the training loop as ONE launch over every parameter of every group (sg_adam_step): what
// `torch.optim.Adam.step()` does with a chain of _foreach_* launches (gs_trainer.py:240-262), elementwise over the flat gradient
// arena and two flat moment buffers of the same layout.
//
// Byte-bound: 28 B per element (read g, p, m, v; write p, m, v), no atomics, no LDS.  Everything that changes from step to step
// (learning rate, bias corrections) is a row of a table in device memory, so a captured launch replays with the step's values.
//
// Work is cut into chunks of SG_ADAM_CHUNK consecutive elements of ONE segment (= one parameter tensor); a workgroup takes chunks
// c = blockIdx.x, + gridDim.x, ...  A chunk's segment record and its group's row are wave-uniform.  Where the parameter pointer and
// the arena offset are misaligned by the SAME number of floats, a chunk is up to 3 scalar elements, 16-byte quads, up to 3 scalar
// elements; where they differ (arena offsets are sum(numel): a bias of 3 floats shifts every later segment) no quad is aligned
// in both, and the chunk is done one float per lane, lanes consecutive.
//
// The arithmetic is the contract (include/sings_hip.h), fp32, in this order, nothing contracted (-ffp-contract=off), division and
// square root correctly rounded, denormals kept.
#include "sg_host.h"

#define SG_ADAM_THREADS 256
#define SG_ADAM_CHUNK 4096                       // elements: 4 quads per lane
#define SG_ADAM_MAX_BLOCKS 2048

struct SgAdamRow { float w1, b2, w2, c2, eps, neg_step; };

__device__ __forceinline__ void sg_adam_update(float g, float &p, float &m, float &v, const SgAdamRow &h)
{
    m = m + (g - m) * h.w1;
    v = v * h.b2 + (h.w2 * g) * g;
    const float d = sqrtf(v) / h.c2 + h.eps;
    p = p + (h.neg_step * m) / d;
}

__device__ __forceinline__ void sg_adam_update4(const float4 &g, float4 &p, float4 &m, float4 &v, const SgAdamRow &h)
{
    sg_adam_update(g.x, p.x, m.x, v.x, h);
    sg_adam_update(g.y, p.y, m.y, v.y, h);
    sg_adam_update(g.z, p.z, m.z, v.z, h);
    sg_adam_update(g.w, p.w, m.w, v.w, h);
}

__device__ __forceinline__ void sg_adam_scalar(size_t i, const float *g, float *p, float *m, float *v, const SgAdamRow &h)
{
    float pi = p[i], mi = m[i], vi = v[i];
    sg_adam_update(g[i], pi, mi, vi, h);
    p[i] = pi; m[i] = mi; v[i] = vi;
}

// segments [S][4] int64: parameter address, arena offset (floats), element count, group;  chunks [C][2] int32: segment, first element
__global__ void __launch_bounds__(SG_ADAM_THREADS)
sg_adam_step_kernel(int n_chunks, const int64_t *__restrict__ segments, const int32_t *__restrict__ chunks,
                    const float *__restrict__ hyper, const float *__restrict__ grad, float *__restrict__ exp_avg,
                    float *__restrict__ exp_avg_sq)
{
    const uint32_t tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t *rec = segments + 4 * (size_t)chunks[2 * c];
        float *p = (float *)(uintptr_t)rec[0];
        const size_t off = (size_t)rec[1], count = (size_t)rec[2];
        // (volatile: vector loads, so that the multipliers sit in VGPRs -- a uniform load would leave them in SGPRs, and a vector
        // instruction with an SGPR source issues at half rate)
        const volatile float *row = hyper + 8 * (size_t)rec[3];
        const SgAdamRow h = {row[0], row[1], row[2], row[3], row[4], row[5]};
        const float *g = grad + off;
        float *m = exp_avg + off, *v = exp_avg_sq + off;
        const size_t s = (size_t)(uint32_t)chunks[2 * c + 1];
        const size_t e = count - s < SG_ADAM_CHUNK ? count : s + SG_ADAM_CHUNK;
        const uint32_t ap = (uint32_t)((uintptr_t)p >> 2) & 3u, aa = (uint32_t)off & 3u;      // (grad / moment bases: 16-B aligned)
        if (ap != aa) {
            for (size_t i = s + tid; i < e; i += SG_ADAM_THREADS)
                sg_adam_scalar(i, g, p, m, v, h);
            continue;
        }
        size_t vs = s + ((4u - ((ap + (uint32_t)s) & 3u)) & 3u);        // first element of the chunk that is 16-B aligned
        if (vs > e) vs = e;
        const size_t nq = (e - vs) >> 2, ve = vs + 4 * nq;
        const uint32_t nh = (uint32_t)(vs - s), nt = (uint32_t)(e - ve);                 // <= 3 each
        if (tid < nh + nt)
            sg_adam_scalar(tid < nh ? s + tid : ve + (tid - nh), g, p, m, v, h);
        const float4 *g4 = (const float4 *)(g + vs);
        float4 *p4 = (float4 *)(p + vs), *m4 = (float4 *)(m + vs), *v4 = (float4 *)(v + vs);
        if (nq == SG_ADAM_CHUNK / 4) {                                    // a full chunk: 16 loads in flight per lane
            float4 gg[4], pp[4], mm[4], vv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t q = tid + j * SG_ADAM_THREADS;
                gg[j] = g4[q]; pp[j] = p4[q]; mm[j] = m4[q]; vv[j] = v4[q];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t q = tid + j * SG_ADAM_THREADS;
                sg_adam_update4(gg[j], pp[j], mm[j], vv[j], h);
                p4[q] = pp[j]; m4[q] = mm[j]; v4[q] = vv[j];
            }
        } else {
            for (size_t q = tid; q < nq; q += SG_ADAM_THREADS) {
                const float4 gq = g4[q];
                float4 pq = p4[q], mq = m4[q], vq = v4[q];
                sg_adam_update4(gq, pq, mq, vq, h);
                p4[q] = pq; m4[q] = mq; v4[q] = vq;
            }
        }
    }
}

extern "C" size_t sg_adam_chunk_elements(void) { return SG_ADAM_CHUNK; }

extern "C" int sg_adam_step(int n_segments, int n_chunks, int n_groups, const int64_t *segments, const int32_t *chunks,
                            const float *hyper, const float *grad_flat, float *exp_avg, float *exp_avg_sq, void *stream)
{
    if (n_segments < 0 || n_chunks < 0 || n_groups < 1 || (n_chunks > 0 && n_segments < 1))
        return sg_set_error("sg_adam_step: n_segments, n_chunks must be >= 0 (chunks need a segment), n_groups >= 1", hipSuccess);
    if (!segments || !chunks || !hyper || !grad_flat || !exp_avg || !exp_avg_sq)
        return sg_set_error("sg_adam_step: null pointer", hipSuccess);
    if ((((uintptr_t)grad_flat | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0)
        return sg_set_error("sg_adam_step: grad_flat, exp_avg and exp_avg_sq must be 16-byte aligned", hipSuccess);
    if (grad_flat == exp_avg || grad_flat == exp_avg_sq || exp_avg == exp_avg_sq)
        return sg_set_error("sg_adam_step: grad_flat, exp_avg and exp_avg_sq must be three buffers", hipSuccess);
    if (n_chunks == 0) return 0;
    const unsigned blocks = n_chunks < SG_ADAM_MAX_BLOCKS ? (unsigned)n_chunks : SG_ADAM_MAX_BLOCKS;
    hipLaunchKernelGGL(sg_adam_step_kernel, dim3(blocks), dim3(SG_ADAM_THREADS), 0, (hipStream_t)stream, n_chunks, segments, chunks,
                       hyper, grad_flat, exp_avg, exp_avg_sq);
    return sg_launched("sg_adam_step");
}
