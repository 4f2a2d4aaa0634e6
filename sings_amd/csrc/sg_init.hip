// The start of a SinGS training run on the device (sings_hybrid.py:608-741): the initial values `SinGS.initialize` takes from the
// body mesh, the loss of `SinGS.init_attrs`' pre-fit (six MSE terms, value and gradient in one march) and its ReduceLROnPlateau
// scheduler as a state machine in device memory.
//
// Not throughput kernels: at SMPL scale (110 k vertices, 330 k edges, 220 k faces) every array is a few MB.  What the reference pays
// for is a Python loop over the vertices with a scan of the edge list in each iteration (:688-696) and a host read per pre-fit step
// (:661-667); here that is a handful of launches, one host read for the error flags, and a step that replays from a HIP graph.
//
//   incident rows   first[v] / second[v]: the two smallest row indices of the edge list that contain v.  Two launches over the edges
//                   with an integer atomicMin per endpoint (the second skips rows equal to first): a minimum of integers does not
//                   depend on the order the atomics land in.
//   normals         per face the unit normal times the corner angle, added to the corner's accumulator in 64-bit FIXED POINT with
//                   integer atomics: an integer sum has no order either.  |term| <= pi and a vertex has at most F faces, so with
//                   the scale 2^k, k = 61 - ceil(log2(4 max(F, 1))), |sum| < 2^61: no overflow by construction; k >= 30.
//   per vertex      the scale rule, the normalised normal and the rotation that takes +z to it, evaluated in fp64 from the fp32
//                   inputs and rounded once.
//
// Every row index and corner is range-checked BEFORE it is used: a row that is not 0 <= a < b < V, or a face with a corner outside
// [0, V), sets a bit of info[] and is skipped, never dereferenced.
#include "sg_host.h"
#include <climits>

#define SG_INIT_THREADS 256
#define SG_INIT_MAX_F 715827882                  // 3 F < 2^31 (as sg_mesh.hip)
#define SG_MSE_THREADS 256
#define SG_MSE_MAX_BLOCKS 1024
#define SG_MSE_PAIRS 6
#define SG_PLATEAU_MAX_GROUPS 64

static inline unsigned sg_init_blocks(long long n) { return (unsigned)((n + SG_INIT_THREADS - 1) / SG_INIT_THREADS); }

// ---- incident rows ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SG_INIT_THREADS)
sg_init_clear_kernel(int V, int32_t *__restrict__ first, int32_t *__restrict__ second, long long *__restrict__ acc, int32_t *__restrict__ info)
{
    const int v = blockIdx.x * SG_INIT_THREADS + threadIdx.x;
    if (v < 4 && info) info[v] = 0;
    if (v >= V) return;
    first[v] = INT_MAX; second[v] = INT_MAX;
    acc[3 * (size_t)v] = 0; acc[3 * (size_t)v + 1] = 0; acc[3 * (size_t)v + 2] = 0;
}

// pass 0: first[v] = min row with v;  pass 1: second[v] = min row with v that is not first[v]
__global__ void __launch_bounds__(SG_INIT_THREADS)
sg_init_rows_kernel(int V, int E, int pass, const int32_t *__restrict__ edges, int32_t *__restrict__ first, int32_t *__restrict__ second,
                    int32_t *__restrict__ info)
{
    const int r = blockIdx.x * SG_INIT_THREADS + threadIdx.x;
    if (r >= E) return;
    const int a = edges[2 * (size_t)r], b = edges[2 * (size_t)r + 1];
    if (!(0 <= a && a < b && b < V)) {                               // range check: the row is reported and skipped
        if (pass == 0) atomicOr(&info[0], 1);
        return;
    }
    if (pass == 0) {
        atomicMin(&first[a], r); atomicMin(&first[b], r);
    } else {
        if (first[a] != r) atomicMin(&second[a], r);
        if (first[b] != r) atomicMin(&second[b], r);
    }
}

// ---- angle-weighted face normals, fixed point ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SG_INIT_THREADS)
sg_init_face_normals_kernel(int V, int F, double fixed, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                            long long *__restrict__ acc, int32_t *__restrict__ info)
{
    const int f = blockIdx.x * SG_INIT_THREADS + threadIdx.x;
    if (f >= F) return;
    int c[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) { c[k] = faces[3 * (size_t)f + k]; ok = ok && c[k] >= 0 && c[k] < V; }
    if (!ok) { atomicOr(&info[2], 1); return; }                      // range check: the face is reported and skipped
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int d = 0; d < 3; d++) p[k][d] = (double)verts[3 * (size_t)c[k] + d];
    const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
    double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double nn = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(nn > 0.0) || !(nn < INFINITY)) return;                     // a degenerate (or non-finite) face has no normal: no term
    nx /= nn; ny /= nn; nz /= nn;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const double ax = p[i][0] - p[k][0], ay = p[i][1] - p[k][1], az = p[i][2] - p[k][2];
        const double bx = p[j][0] - p[k][0], by = p[j][1] - p[k][1], bz = p[j][2] - p[k][2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double angle = atan2(sqrt(cx * cx + cy * cy + cz * cz), ax * bx + ay * by + az * bz);      // in [0, pi]
        unsigned long long *dst = (unsigned long long *)(acc + 3 * (size_t)c[k]);
        atomicAdd(dst, (unsigned long long)llrint(nx * angle * fixed));
        atomicAdd(dst + 1, (unsigned long long)llrint(ny * angle * fixed));
        atomicAdd(dst + 2, (unsigned long long)llrint(nz * angle * fixed));
    }
}

// ---- per vertex: scales, normal, rotation ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SG_INIT_THREADS)
sg_init_vertex_kernel(int V, float scale_multiplier, float thickness, const float *__restrict__ verts, const int32_t *__restrict__ edges,
                      const int32_t *__restrict__ first, const int32_t *__restrict__ second, const long long *__restrict__ acc,
                      float *__restrict__ scales, float *__restrict__ scales_aux, float *__restrict__ normals, float *__restrict__ rotmat,
                      int32_t *__restrict__ info)
{
    const int v = blockIdx.x * SG_INIT_THREADS + threadIdx.x;
    if (v >= V) return;
    // scales: the first two rows that contain v, (a0, b0) and (a1, b1); len = multiplier * max(|x[a0] - x[a1]|, |x[b0] - x[b1]|)
    const int r0 = first[v], r1 = second[v];
    float s[3] = {0.f, 0.f, 0.f}, sa[3] = {0.f, 0.f, 0.f};
    if (r1 == INT_MAX) {                                             // fewer than two incident rows (r0 <= r1): reported, zeros
        atomicOr(&info[1], 1);
    } else {                                                         // (only rows that passed the range check are in first / second)
        const int a0 = edges[2 * (size_t)r0], b0 = edges[2 * (size_t)r0 + 1], a1 = edges[2 * (size_t)r1], b1 = edges[2 * (size_t)r1 + 1];
        double la = 0.0, lb = 0.0;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double da = (double)verts[3 * (size_t)a0 + d] - (double)verts[3 * (size_t)a1 + d];
            const double db = (double)verts[3 * (size_t)b0 + d] - (double)verts[3 * (size_t)b1 + d];
            la += da * da; lb += db * db;
        }
        const double len = (double)scale_multiplier * sqrt(fmax(la, lb));
        const double l = log(len);
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double sd = exp(d == 2 ? l * (double)thickness : l);        // the thickness factor acts on the logarithm (:699)
            s[d] = (float)sd;
            sa[d] = (float)log(expm1(sd));                                     // log(exp(scales) - 1)
        }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) { scales[3 * (size_t)v + d] = s[d]; scales_aux[3 * (size_t)v + d] = sa[d]; }
    // normal: the accumulated sum, normalised (the fixed-point scale cancels); no face: zero
    double nx = (double)acc[3 * (size_t)v], ny = (double)acc[3 * (size_t)v + 1], nz = (double)acc[3 * (size_t)v + 2];
    const double nn = sqrt(nx * nx + ny * ny + nz * nz);
    if (nn > 0.0) { nx /= nn; ny /= nn; nz /= nn; } else { nx = ny = 0.0; nz = 0.0; }
    normals[3 * (size_t)v] = (float)nx; normals[3 * (size_t)v + 1] = (float)ny; normals[3 * (size_t)v + 2] = (float)nz;
    // rotation of +z onto n: I + K + K^2 / (1 + c), c = n.z, K the cross-product matrix of (0,0,1) x n = (-n.y, n.x, 0).  A vertex
    // without a normal: identity.  1 + c <= 0 (n = -z): the half-turn about x.
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (nn > 0.0) {
        const double d1 = 1.0 + nz;
        if (d1 > 0.0) {
            const double f = 1.0 / d1;
            R[0] = 1.0 - f * nx * nx; R[1] = -f * nx * ny;       R[2] = nx;
            R[3] = -f * nx * ny;      R[4] = 1.0 - f * ny * ny;  R[5] = ny;
            R[6] = -nx;               R[7] = -ny;                R[8] = 1.0 - f * (nx * nx + ny * ny);
        } else {
            R[4] = -1.0; R[8] = -1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) rotmat[9 * (size_t)v + k] = (float)R[k];
}

extern "C" size_t sg_init_ws_bytes(int V)
{
    if (V < 0 || V > (1 << 30)) return 0;
    return sg_align((size_t)(V > 0 ? V : 1) * 3 * sizeof(long long));
}

extern "C" int sg_init_attributes(int V, int F, int E, float init_scale_multiplier, float thickness_factor, const float *verts,
                                  const int32_t *faces, const int32_t *edges, void *ws, int32_t *first, int32_t *second, float *scales,
                                  float *scales_aux, float *normals, float *rotmat, int32_t *info, void *stream)
{
    if (V < 1 || V > (1 << 30) || F < 0 || F > SG_INIT_MAX_F || E < 0)
        return sg_set_error("sg_init_attributes: 1 <= V <= 2^30, 0 <= F <= (2^31 - 1) / 3, E >= 0", hipSuccess);
    if (!verts || (F > 0 && !faces) || (E > 0 && !edges) || !ws || !first || !second || !scales || !scales_aux || !normals || !rotmat || !info)
        return sg_set_error("sg_init_attributes: null pointer", hipSuccess);
    if (((uintptr_t)ws & 7) != 0)
        return sg_set_error("sg_init_attributes: ws must be 8-byte aligned", hipSuccess);
    hipStream_t st = (hipStream_t)stream;
    long long *acc = (long long *)ws;
    // the fixed-point scale: |sum| <= F * pi * 2^k < 4 F * 2^k <= 2^61
    int bits = 0;
    while ((1ll << bits) < 4ll * (F > 0 ? F : 1)) bits++;
    const double fixed = ldexp(1.0, 61 - bits);
    hipLaunchKernelGGL(sg_init_clear_kernel, dim3(sg_init_blocks(V)), dim3(SG_INIT_THREADS), 0, st, V, first, second, acc, info);
    if (E > 0) {
        hipLaunchKernelGGL(sg_init_rows_kernel, dim3(sg_init_blocks(E)), dim3(SG_INIT_THREADS), 0, st, V, E, 0, edges, first, second, info);
        hipLaunchKernelGGL(sg_init_rows_kernel, dim3(sg_init_blocks(E)), dim3(SG_INIT_THREADS), 0, st, V, E, 1, edges, first, second, info);
    }
    if (F > 0)
        hipLaunchKernelGGL(sg_init_face_normals_kernel, dim3(sg_init_blocks(F)), dim3(SG_INIT_THREADS), 0, st, V, F, fixed, verts, faces, acc,
                           info);
    hipLaunchKernelGGL(sg_init_vertex_kernel, dim3(sg_init_blocks(V)), dim3(SG_INIT_THREADS), 0, st, V, init_scale_multiplier,
                       thickness_factor, verts, edges, first, second, acc, scales, scales_aux, normals, rotmat, info);
    return sg_launched("sg_init_attributes");
}

// ---- the pre-fit's loss: up to six MSE terms, value and gradient in one march -------------------------------------------------------
struct SgMsePairs {
    const float *out[SG_MSE_PAIRS], *tgt[SG_MSE_PAIRS];
    float *grad[SG_MSE_PAIRS];
    long long numel[SG_MSE_PAIRS];               // 0: the pair is absent
};

__global__ void __launch_bounds__(SG_MSE_THREADS)
sg_attr_mse_kernel(SgMsePairs P, float *__restrict__ partials)
{
    __shared__ float sW[SG_MSE_THREADS / SG_WAVE][SG_MSE_PAIRS];
    const long long stride = (long long)gridDim.x * SG_MSE_THREADS;
    const long long t0 = (long long)blockIdx.x * SG_MSE_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SG_MSE_PAIRS; k++) {
        const long long n = P.numel[k];
        float a = 0.f;
        if (n > 0) {
            const float *__restrict__ o = P.out[k], *__restrict__ t = P.tgt[k];
            float *__restrict__ g = P.grad[k];
            const float fn = (float)n;
            for (long long i = t0; i < n; i += stride) {
                const float d = o[i] - t[i];
                a += d * d;
                if (g) g[i] = (2.0f * d) / fn;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s, 64);          // (a fixed tree: the same bits on every run)
        if (lane == 0) sW[wave][k] = a;
    }
    __syncthreads();
    if (threadIdx.x < SG_MSE_PAIRS) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < SG_MSE_THREADS / SG_WAVE; w++) a += sW[w][threadIdx.x];
        partials[(size_t)blockIdx.x * 8 + threadIdx.x] = a;
    }
}

// one wave: the partials of a term are summed in a fixed order, in double; terms[k] = sum / numel, terms[6] = their fp32 sum in order
__global__ void __launch_bounds__(SG_WAVE)
sg_attr_mse_final_kernel(SgMsePairs P, int blocks, const float *__restrict__ partials, float *__restrict__ terms)
{
    __shared__ float sT[SG_MSE_PAIRS];
    const int lane = threadIdx.x;
    for (int k = 0; k < SG_MSE_PAIRS; k++) {
        double a = 0.0;
        for (int b = lane; b < blocks; b += SG_WAVE) a += (double)partials[(size_t)b * 8 + k];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s, 64);
        if (lane == 0) sT[k] = P.numel[k] > 0 ? (float)(a / (double)P.numel[k]) : 0.f;
    }
    __syncthreads();
    if (lane == 0) {
        float total = 0.f;
        for (int k = 0; k < SG_MSE_PAIRS; k++) { terms[k] = sT[k]; if (P.numel[k] > 0) total += sT[k]; }
        terms[6] = total; terms[7] = 0.f;
    }
}

static const int sg_mse_width[SG_MSE_PAIRS] = {3, 3, 3, 6, 48, 1};

extern "C" size_t sg_attr_mse_ws_bytes(void) { return sg_align((size_t)SG_MSE_MAX_BLOCKS * 8 * sizeof(float)); }

extern "C" int sg_attr_mse(int N, const float *const *outputs, const float *const *targets, float *const *grads, void *ws, float *terms,
                           void *stream)
{
    if (N < 1 || N > (1 << 30))
        return sg_set_error("sg_attr_mse: 1 <= N <= 2^30", hipSuccess);
    if (!outputs || !targets || !ws || !terms)
        return sg_set_error("sg_attr_mse: null pointer", hipSuccess);
    SgMsePairs P;
    long long most = 0;
    for (int k = 0; k < SG_MSE_PAIRS; k++) {
        if ((outputs[k] == nullptr) != (targets[k] == nullptr))
            return sg_set_error("sg_attr_mse: a pair needs both its output and its target (or neither)", hipSuccess);
        P.out[k] = outputs[k]; P.tgt[k] = targets[k];
        P.grad[k] = outputs[k] && grads ? grads[k] : nullptr;
        P.numel[k] = outputs[k] ? (long long)N * sg_mse_width[k] : 0;
        if (P.numel[k] > most) most = P.numel[k];
    }
    if (most == 0)
        return sg_set_error("sg_attr_mse: no pair", hipSuccess);
    long long blocks = (most + SG_MSE_THREADS * 4 - 1) / (SG_MSE_THREADS * 4);
    if (blocks > SG_MSE_MAX_BLOCKS) blocks = SG_MSE_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_attr_mse_kernel, dim3((unsigned)blocks), dim3(SG_MSE_THREADS), 0, st, P, (float *)ws);
    hipLaunchKernelGGL(sg_attr_mse_final_kernel, dim3(1), dim3(SG_WAVE), 0, st, P, (int)blocks, (const float *)ws, terms);
    return sg_launched("sg_attr_mse");
}

// ---- ReduceLROnPlateau (mode min, relative threshold, cooldown 0, min_lr 0) in device memory ------------------------------------------
// state (double): [0] best, [1] bad steps, [2] losses digested, [3] steps begun, [4 .. 4 + G) multiplier per group,
// [4 + G .. 4 + 2 G) base learning rate per group.  One launch per step, lane 0 runs the state machine:
//   if steps begun > losses digested: the loss at *loss belongs to the previous step -- digest it (row `losses digested` of log takes
//   n_copy floats of `terms` and the G multipliers that step ran with, as doubles);  then, with begin != 0, count this step as begun
//   and multiply column 5 of every group's row of `hyper` by its multiplier.
__global__ void __launch_bounds__(SG_WAVE)
sg_plateau_kernel(int G, int begin, double factor, int patience, double threshold, double eps, const float *__restrict__ loss,
                  double *__restrict__ state, float *__restrict__ hyper, const float *__restrict__ terms, int n_copy,
                  double *__restrict__ log, int log_rows)
{
    __shared__ int sDigest;
    __shared__ int sRow;
    const int lane = threadIdx.x;
    if (lane == 0) {
        const int digested = (int)state[2], begun = (int)state[3];
        sDigest = begun > digested; sRow = digested;
        if (sDigest) {
            const double cur = (double)loss[0];
            double best = state[0], bad = state[1];
            if (log && digested < log_rows)                          // the multipliers that step ran with: before this digest
                for (int g = 0; g < G; g++) log[(size_t)digested * (n_copy + G) + n_copy + g] = state[4 + g];
            if (cur < best * (1.0 - threshold)) { best = cur; bad = 0.0; } else bad += 1.0;
            if (bad > (double)patience) {
                for (int g = 0; g < G; g++) {
                    const double old_lr = state[4 + G + g] * state[4 + g], new_lr = old_lr * factor;      // (min_lr 0)
                    if (old_lr - new_lr > eps) state[4 + g] *= factor;
                }
                bad = 0.0;
            }
            state[0] = best; state[1] = bad; state[2] = (double)(digested + 1);
        }
        if (begin) state[3] = (double)(begun + 1);
    }
    __syncthreads();
    if (sDigest && log && sRow < log_rows && lane < n_copy) log[(size_t)sRow * (n_copy + G) + lane] = (double)terms[lane];
    if (begin && hyper)
        for (int g = lane; g < G; g += SG_WAVE) hyper[8 * (size_t)g + 5] *= (float)state[4 + g];
}

extern "C" int sg_plateau_step(int n_groups, int begin, int patience, const double *settings, const float *loss, double *state,
                               float *hyper, const float *terms, int n_copy, double *log, int log_rows, void *stream)
{
    if (n_groups < 1 || n_groups > SG_PLATEAU_MAX_GROUPS || patience < 0 || n_copy < 0 || n_copy > SG_WAVE || log_rows < 0)
        return sg_set_error("sg_plateau_step: 1 <= n_groups <= 64, patience >= 0, 0 <= n_copy <= 64, log_rows >= 0", hipSuccess);
    if (!settings || !loss || !state || (begin && !hyper) || (log && n_copy > 0 && !terms))
        return sg_set_error("sg_plateau_step: null pointer", hipSuccess);
    const double factor = settings[0], threshold = settings[1], eps = settings[2];
    if (!(factor > 0.0 && factor < 1.0) || !(threshold >= 0.0) || !(eps >= 0.0))
        return sg_set_error("sg_plateau_step: 0 < factor < 1, threshold >= 0, eps >= 0", hipSuccess);
    hipLaunchKernelGGL(sg_plateau_kernel, dim3(1), dim3(SG_WAVE), 0, (hipStream_t)stream, n_groups, begin, factor, patience, threshold, eps,
                       loss, state, hyper, terms, n_copy, log, log_rows);
    return sg_launched("sg_plateau_step");
}
