// The densification statistics of a step behind a gate in device memory (include/sings_density.h states the rule;
// sings_amd/density.py holds its numpy twin).
//
// One thread per Gaussian, the K frames in ascending order in registers, at most one store per array.  Byte-bound and tiny: per
// Gaussian 4 B of radius per frame, 8 of the 12 B of a gradient row per VISIBLE frame (the third column is never loaded; a wave's
// 64 rows are one contiguous 768-B run), and a read and a write of three floats when some frame saw it.  At 150 000 Gaussians and
// one frame that is under 5 MB: the launch is there for what it replaces (a chain of torch launches over [K,N]) and for the gate.
// The gate is one uniform load: every wave tests it and leaves before it has touched an array.
#include "sg_host.h"
#include "../../include/sings_density.h"

__global__ void __launch_bounds__(SG_DENSITY_BLOCK)
sg_density_stats_kernel(int K, int N, const float *__restrict__ grad, const int32_t *__restrict__ radii,
                        const int32_t *__restrict__ gate, float *__restrict__ accum, float *__restrict__ denom,
                        float *__restrict__ max_radii)
{
    if (gate != nullptr && *gate == 0) return;
    const size_t i = (size_t)blockIdx.x * SG_DENSITY_BLOCK + threadIdx.x;
    if (i >= (size_t)N) return;
    float sum = 0.0f, widest = 0.0f;
    int seen = 0;
    for (int k = 0; k < K; k++) {
        const size_t row = (size_t)k * (size_t)N + i;
        const int32_t r = radii[row];
        if (r <= 0) continue;                            // skipped, not multiplied by zero: the gradient is not even loaded
        const float gx = grad[3 * row], gy = grad[3 * row + 1];
        sum += sqrtf(fmaf(gx, gx, gy * gy));             // (0 + the first norm is that norm: K - 1 rounded additions)
        widest = fmaxf(widest, (float)r);
        seen++;
    }
    if (seen == 0) return;                               // no frame saw it: the row keeps its bits
    accum[i] += sum;
    float d = denom[i];
    for (int s = 0; s < seen; s++) d += 1.0f;            // denom += 1 per visible frame, as the rule says it (K <= 16 additions)
    denom[i] = d;
    max_radii[i] = fmaxf(max_radii[i], widest);
}

extern "C" int sg_density_stats(int K, int N, const float *grad, const int32_t *radii, const int32_t *gate, float *accum,
                                float *denom, float *max_radii, void *stream)
{
    const char *who = "sg_density_stats";
    if (N < 0) return sg_failf("%s: N = %d is negative", who, N);
    if (K < 1 || K > SG_DENSITY_MAX_K) return sg_failf("%s: K = %d outside 1..%d", who, K, SG_DENSITY_MAX_K);
    if (N == 0) return 0;
    if (!grad || !radii || !accum || !denom || !max_radii) return sg_failf("%s: null pointer", who);
    const unsigned blocks = (unsigned)(((size_t)N + SG_DENSITY_BLOCK - 1) / SG_DENSITY_BLOCK);
    hipLaunchKernelGGL(sg_density_stats_kernel, dim3(blocks), dim3(SG_DENSITY_BLOCK), 0, (hipStream_t)stream, K, N, grad, radii,
                       gate, accum, denom, max_radii);
    return sg_launched(who);
}
