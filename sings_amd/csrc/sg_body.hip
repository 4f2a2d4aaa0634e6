// The body model on the device (include/sings_body.h): what the reference's SMPL / SMPLH layer does once per run on the host -- the
// regressor of a subdivided template (smpl_layer.py:349-350), the rest joints of a betas vector, blend shapes and pose correctives
// (body_model/lbs.py:129-165) and the smoothing filter of its subdivision loop (smpl_layer.py:322-331).
//
// Not throughput kernels: they run once per template or once per betas vector.  What they are held to is reproducibility and accuracy:
//   sums        fp64, in a fixed order: a thread walks its elements in index order, a workgroup adds its 256 values in a fixed tree, one
//               workgroup adds the workgroups' partials the same way.  No floating-point atomics anywhere.
//   normals     the unit face normals are added to their corners in 64-bit FIXED POINT with integer atomics (as sg_init.hip): an
//               integer sum has no order.  |term| <= 1 and a vertex has at most F faces, so with the scale 2^k,
//               k = 61 - ceil(log2(4 max(F, 1))), |sum| < 2^61: no overflow by construction; k >= 30.
//   the filter  x lives in fp64 in the workspace across the iterations; its fp32 rounding is written once, at the end, and only when
//               no error bit is set.
//
// Every face corner is range-checked BEFORE it is used (a bad face sets a bit of info[] and is skipped); the CSR comes from
// sg_mesh_terms_build, which skips bad edge rows the same way, so its columns lie in [0, V).
#include "sg_host.h"
#include "../../include/sings_body.h"

#define SGB_THREADS 256
#define SGB_MAX_F 715827882                      // 3 F < 2^31 (as sg_mesh.hip)
// scal[]: the scalars of the filter, in device memory
#define SGB_VOL0 0
#define SGB_EPS 1
#define SGB_MEAN_A 2
#define SGB_SLOPE 3
#define SGB_STEP 4
#define SGB_SCALARS 8

static inline unsigned sgb_blocks(long long n) { return (unsigned)((n + SGB_THREADS - 1) / SGB_THREADS); }

// the 256 values of a workgroup added in a fixed tree -> every thread gets the sum
__device__ __forceinline__ double sgb_block_sum(double v, double *s)
{
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = SGB_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double sgb_block_max(double v, double *s)
{
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = SGB_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
// n partials added by ONE workgroup: thread t takes t, t + 256, ... in order, then the tree
__device__ __forceinline__ double sgb_final_sum(const double *__restrict__ partial, int n, double *s)
{
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += SGB_THREADS) v += partial[i];
    return sgb_block_sum(v, s);
}

// ---- the regressor of a subdivided template ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_renorm_kernel(int J, int V, const float *__restrict__ Jt, float *__restrict__ Jreg)
{
    __shared__ double s[SGB_THREADS];
    const int j = blockIdx.x;
    double v = 0.0;
    for (int i = threadIdx.x; i < V; i += SGB_THREADS) v += (double)Jt[(size_t)i * J + j];
    const float sum = (float)sgb_block_sum(v, s);
    for (int i = threadIdx.x; i < V; i += SGB_THREADS) Jreg[(size_t)j * V + i] = Jt[(size_t)i * J + j] / sum;
}

// ---- the regressor folded through [v_template | shapedirs] ----------------------------------------------------------------------------
// a workgroup per (joint, axis); a thread keeps the B + 1 sums of its vertices.  A zero weight adds nothing and is skipped: the
// regressor of a body model is sparse.
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_joint_basis_kernel(int V, int B, const float *__restrict__ vt, const float *__restrict__ shapedirs, const float *__restrict__ Jreg,
                           float *__restrict__ J0, float *__restrict__ JS)
{
    __shared__ double s[SGB_THREADS];
    const int j = blockIdx.x / 3, c = blockIdx.x % 3;
    double acc[SG_BODY_MAX_BETAS + 1];
#pragma unroll
    for (int q = 0; q <= SG_BODY_MAX_BETAS; q++) acc[q] = 0.0;
    for (int v = threadIdx.x; v < V; v += SGB_THREADS) {
        const double w = (double)Jreg[(size_t)j * V + v];
        if (w == 0.0) continue;
        acc[0] += w * (double)vt[3 * (size_t)v + c];
        const float *sd = shapedirs + (3 * (size_t)v + c) * B;
#pragma unroll
        for (int b = 0; b < SG_BODY_MAX_BETAS; b++)
            if (b < B) acc[1 + b] += w * (double)sd[b];
    }
#pragma unroll
    for (int q = 0; q <= SG_BODY_MAX_BETAS; q++) {
        if (q <= B) {                                                // (uniform: every thread of the workgroup takes the same q)
            const double r = sgb_block_sum(acc[q], s);
            if (threadIdx.x == 0) {
                if (q == 0) J0[blockIdx.x] = (float)r;
                else JS[(size_t)blockIdx.x * B + (q - 1)] = (float)r;
            }
        }
    }
}

// ---- blend shapes and pose correctives ------------------------------------------------------------------------------------------------
// a thread per (row k, coordinate i of the 3 V); posedirs [P, 3V] is read along i
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_shaped_kernel(int V, int B, int P, const float *__restrict__ vt, const float *__restrict__ shapedirs, const float *__restrict__ betas,
                      const float *__restrict__ posedirs, const float *__restrict__ feat, float *__restrict__ v_shaped,
                      float *__restrict__ shape_off, float *__restrict__ pose_off, float *__restrict__ v_posed)
{
    const size_t n = 3 * (size_t)V, i = (size_t)blockIdx.x * SGB_THREADS + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= n) return;
    double so = 0.0, po = 0.0;
    for (int b = 0; b < B; b++) so += (double)shapedirs[i * B + b] * (double)betas[(size_t)k * B + b];
    for (int p = 0; p < P; p++) po += (double)feat[(size_t)k * P + p] * (double)posedirs[(size_t)p * n + i];
    const double vs = (double)vt[i] + so;
    const size_t o = (size_t)k * n + i;
    if (shape_off) shape_off[o] = (float)so;
    if (pose_off) pose_off[o] = (float)po;
    if (v_shaped) v_shaped[o] = (float)vs;
    if (v_posed) v_posed[o] = (float)(vs + po);
}

// ---- the smoothing filter -------------------------------------------------------------------------------------------------------------
struct SgbWs { double *x, *nrm, *delta, *a, *partial, *scal; long long *acc; int pitch; };

static SgbWs sgb_carve(void *ws, int V, int F)
{
    SgbWs w;
    const size_t v3 = 3 * (size_t)V;
    const unsigned nbv = sgb_blocks(V), nbf = sgb_blocks(F);
    w.pitch = (int)(nbv > nbf ? nbv : nbf);
    w.x = (double *)ws; w.nrm = w.x + v3; w.delta = w.nrm + v3; w.a = w.delta + v3;
    w.partial = w.a + V; w.scal = w.partial + 2 * (size_t)w.pitch;
    w.acc = (long long *)(w.scal + SGB_SCALARS);
    return w;
}

__global__ void __launch_bounds__(SGB_THREADS)
sg_body_prep_kernel(int V, const float *__restrict__ x0, const int32_t *__restrict__ row_ptr, double *__restrict__ x, long long *__restrict__ acc,
                    int32_t *__restrict__ info)
{
    const int v = blockIdx.x * SGB_THREADS + threadIdx.x;
    if (v >= V) return;
    int bad = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const float f = x0[3 * (size_t)v + d];
        if (!isfinite(f)) bad |= SG_BODY_NOT_FINITE;
        x[3 * (size_t)v + d] = (double)f;
        acc[3 * (size_t)v + d] = 0;
    }
    if (row_ptr[v + 1] <= row_ptr[v]) bad |= SG_BODY_ISOLATED;
    if (bad) atomicOr(&info[0], bad);
}

// the corners of face f, range-checked
__device__ __forceinline__ bool sgb_corners(int V, const int32_t *__restrict__ faces, int f, int c[3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) { c[k] = faces[3 * (size_t)f + k]; ok = ok && c[k] >= 0 && c[k] < V; }
    return ok;
}
// x_a . (x_b x x_c) of three points
__device__ __forceinline__ double sgb_triple(const double p[3][3])
{
    const double cx = p[1][1] * p[2][2] - p[1][2] * p[2][1], cy = p[1][2] * p[2][0] - p[1][0] * p[2][2],
                 cz = p[1][0] * p[2][1] - p[1][1] * p[2][0];
    return (p[0][0] * cx + p[0][1] * cy) + p[0][2] * cz;
}

// of x0: the unit face normals into their corners' accumulators, the largest face area and the volume
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_faces0_kernel(int V, int F, double fixed, const double *__restrict__ x, const int32_t *__restrict__ faces, long long *__restrict__ acc,
                      double *__restrict__ partial, int pitch, int32_t *__restrict__ info)
{
    __shared__ double s[SGB_THREADS];
    const int f = blockIdx.x * SGB_THREADS + threadIdx.x;
    double vol = 0.0, area = 0.0;
    int c[3];
    if (f < F) {
        if (!sgb_corners(V, faces, f, c)) atomicOr(&info[0], SG_BODY_BAD_FACE);
        else {
            double p[3][3];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int d = 0; d < 3; d++) p[k][d] = x[3 * (size_t)c[k] + d];
            vol = sgb_triple(p);
            const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
            const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
            if (nn > 0.0 && nn < INFINITY) {                         // a degenerate (or non-finite) face has no normal and no area
                area = 0.5 * nn;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    unsigned long long *dst = (unsigned long long *)(acc + 3 * (size_t)c[k]);
                    atomicAdd(dst, (unsigned long long)llrint(nx / nn * fixed));
                    atomicAdd(dst + 1, (unsigned long long)llrint(ny / nn * fixed));
                    atomicAdd(dst + 2, (unsigned long long)llrint(nz / nn * fixed));
                }
            }
        }
    }
    const double bv = sgb_block_sum(vol, s), ba = sgb_block_max(area, s);
    if (threadIdx.x == 0) { partial[blockIdx.x] = bv; partial[pitch + blockIdx.x] = ba; }
}
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_final0_kernel(int nb, const double *__restrict__ partial, int pitch, double *__restrict__ scal)
{
    __shared__ double s[SGB_THREADS];
    const double vol = sgb_final_sum(partial, nb, s);
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += SGB_THREADS) a = fmax(a, partial[pitch + i]);
    a = sgb_block_max(a, s);
    if (threadIdx.x == 0) {
        scal[SGB_VOL0] = vol / 6.0; scal[SGB_EPS] = 0.01 * sqrt(a);
        scal[SGB_MEAN_A] = 0.0; scal[SGB_SLOPE] = 0.0; scal[SGB_STEP] = 0.0;
    }
}
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_normals_kernel(int V, const long long *__restrict__ acc, double *__restrict__ nrm)
{
    const int v = blockIdx.x * SGB_THREADS + threadIdx.x;
    if (v >= V) return;
    double nx = (double)acc[3 * (size_t)v], ny = (double)acc[3 * (size_t)v + 1], nz = (double)acc[3 * (size_t)v + 2];
    const double nn = sqrt((nx * nx + ny * ny) + nz * nz);           // (the fixed-point scale cancels)
    if (nn > 0.0) { nx /= nn; ny /= nn; nz /= nn; } else { nx = ny = nz = 0.0; }
    nrm[3 * (size_t)v] = nx; nrm[3 * (size_t)v + 1] = ny; nrm[3 * (size_t)v + 2] = nz;
}

// delta = L x - x (the neighbours in the CSR's order: columns ascending), a = 1 / max(1e-12, |n . (x - L x)|), the workgroup's sum of a
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_lap_kernel(int V, const double *__restrict__ x, const double *__restrict__ nrm, const int32_t *__restrict__ row_ptr,
                   const int32_t *__restrict__ col, double *__restrict__ delta, double *__restrict__ a, double *__restrict__ partial)
{
    __shared__ double s[SGB_THREADS];
    const int v = blockIdx.x * SGB_THREADS + threadIdx.x;
    double av = 0.0;
    if (v < V) {
        const int r0 = row_ptr[v], r1 = row_ptr[v + 1];
        double d[3] = { 0.0, 0.0, 0.0 };
        if (r1 > r0) {
            double q[3] = { 0.0, 0.0, 0.0 };
            for (int e = r0; e < r1; e++) {
                const size_t o = 3 * (size_t)col[e];
                q[0] += x[o]; q[1] += x[o + 1]; q[2] += x[o + 2];
            }
            const double n = (double)(r1 - r0);
#pragma unroll
            for (int k = 0; k < 3; k++) d[k] = q[k] / n - x[3 * (size_t)v + k];
        }
        const size_t o = 3 * (size_t)v;
        delta[o] = d[0]; delta[o + 1] = d[1]; delta[o + 2] = d[2];
        const double dil = fabs((nrm[o] * -d[0] + nrm[o + 1] * -d[1]) + nrm[o + 2] * -d[2]);
        av = 1.0 / fmax(1e-12, dil);
        a[v] = av;
    }
    const double b = sgb_block_sum(av, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_mean_kernel(int nb, int V, const double *__restrict__ partial, double *__restrict__ scal)
{
    __shared__ double s[SGB_THREADS];
    const double sum = sgb_final_sum(partial, nb, s);
    if (threadIdx.x == 0) scal[SGB_MEAN_A] = sum / (double)V;
}
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_move_kernel(int V, double lamb, double *__restrict__ x, const double *__restrict__ delta, const double *__restrict__ a,
                    const double *__restrict__ scal)
{
    const int v = blockIdx.x * SGB_THREADS + threadIdx.x;
    if (v >= V) return;
    const double l = fmax(0.2 * lamb, fmin(1.0, lamb * a[v] / scal[SGB_MEAN_A]));
#pragma unroll
    for (int k = 0; k < 3; k++) x[3 * (size_t)v + k] += l * delta[3 * (size_t)v + k];
}
// vol(x) and, in the first iteration, vol(x + eps n): the workgroups' sums
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_vol_kernel(int V, int F, int first, const double *__restrict__ x, const double *__restrict__ nrm, const int32_t *__restrict__ faces,
                   const double *__restrict__ scal, double *__restrict__ partial, int pitch)
{
    __shared__ double s[SGB_THREADS];
    const int f = blockIdx.x * SGB_THREADS + threadIdx.x;
    double vol = 0.0, vole = 0.0;
    int c[3];
    if (f < F && sgb_corners(V, faces, f, c)) {
        double p[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int d = 0; d < 3; d++) p[k][d] = x[3 * (size_t)c[k] + d];
        vol = sgb_triple(p);
        if (first) {
            const double eps = scal[SGB_EPS];
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int d = 0; d < 3; d++) p[k][d] += eps * nrm[3 * (size_t)c[k] + d];
            vole = sgb_triple(p);
        }
    }
    const double bv = sgb_block_sum(vol, s);
    const double be = first ? sgb_block_sum(vole, s) : 0.0;          // (first is uniform)
    if (threadIdx.x == 0) { partial[blockIdx.x] = bv; if (first) partial[pitch + blockIdx.x] = be; }
}
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_vol_final_kernel(int nb, int first, const double *__restrict__ partial, int pitch, double *__restrict__ scal, int32_t *__restrict__ info)
{
    __shared__ double s[SGB_THREADS];
    const double vol = sgb_final_sum(partial, nb, s) / 6.0;
    const double vole = first ? sgb_final_sum(partial + pitch, nb, s) / 6.0 : 0.0;
    if (threadIdx.x != 0) return;
    if (first) {
        const double dv = vole - vol;
        const bool ok = dv != 0.0 && isfinite(dv);
        if (!ok) atomicOr(&info[0], SG_BODY_BAD_SLOPE);
        scal[SGB_SLOPE] = ok ? scal[SGB_EPS] / dv : 0.0;
    }
    scal[SGB_STEP] = scal[SGB_SLOPE] * (scal[SGB_VOL0] - vol);
}
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_push_kernel(int V, double *__restrict__ x, const double *__restrict__ nrm, const double *__restrict__ scal)
{
    const int v = blockIdx.x * SGB_THREADS + threadIdx.x;
    if (v >= V) return;
    const double step = scal[SGB_STEP];
#pragma unroll
    for (int k = 0; k < 3; k++) x[3 * (size_t)v + k] += nrm[3 * (size_t)v + k] * step;
}
__global__ void __launch_bounds__(SGB_THREADS)
sg_body_out_kernel(int V, const double *__restrict__ x, float *__restrict__ x_out, const int32_t *__restrict__ info)
{
    const size_t i = (size_t)blockIdx.x * SGB_THREADS + threadIdx.x;
    if (i >= 3 * (size_t)V || info[0] != 0) return;
    x_out[i] = (float)x[i];
}

// ---- entry points (include/sings_body.h) --------------------------------------------------------------------------------------------
static bool sgb_count_ok(int n, int hi) { return n >= 1 && n <= hi; }

extern "C" int sg_body_renorm(int J, int V, const float *Jt, float *J_regressor, void *stream)
{
    if (!sgb_count_ok(J, SG_BODY_MAX_JOINTS) || !sgb_count_ok(V, SG_BODY_MAX_VERTS))
        return sg_failf("sg_body_renorm: J = %d / V = %d outside 1..%d / 1..%d", J, V, SG_BODY_MAX_JOINTS, SG_BODY_MAX_VERTS);
    if (!Jt || !J_regressor) return sg_set_error("sg_body_renorm: null pointer", hipSuccess);
    hipLaunchKernelGGL(sg_body_renorm_kernel, dim3(J), dim3(SGB_THREADS), 0, (hipStream_t)stream, J, V, Jt, J_regressor);
    return sg_launched("sg_body_renorm");
}

extern "C" int sg_body_joint_basis(int V, int J, int B, const float *v_template, const float *shapedirs, const float *J_regressor,
                                   float *J0, float *JS, void *stream)
{
    if (!sgb_count_ok(J, SG_BODY_MAX_JOINTS) || !sgb_count_ok(V, SG_BODY_MAX_VERTS) || !sgb_count_ok(B, SG_BODY_MAX_BETAS))
        return sg_failf("sg_body_joint_basis: J = %d / V = %d / B = %d outside 1..%d / 1..%d / 1..%d", J, V, B, SG_BODY_MAX_JOINTS,
                        SG_BODY_MAX_VERTS, SG_BODY_MAX_BETAS);
    if (!v_template || !shapedirs || !J_regressor || !J0 || !JS) return sg_set_error("sg_body_joint_basis: null pointer", hipSuccess);
    hipLaunchKernelGGL(sg_body_joint_basis_kernel, dim3(3 * J), dim3(SGB_THREADS), 0, (hipStream_t)stream, V, B, v_template, shapedirs,
                       J_regressor, J0, JS);
    return sg_launched("sg_body_joint_basis");
}

extern "C" int sg_body_shaped(int V, int B, int K, int P, const float *v_template, const float *shapedirs, const float *betas,
                              const float *posedirs, const float *pose_feature, float *v_shaped, float *shape_offsets,
                              float *pose_offsets, float *v_posed, void *stream)
{
    if (!sgb_count_ok(V, SG_BODY_MAX_VERTS) || !sgb_count_ok(B, SG_BODY_MAX_BETAS) || !sgb_count_ok(K, SG_BODY_MAX_ROWS))
        return sg_failf("sg_body_shaped: V = %d / B = %d / K = %d outside 1..%d / 1..%d / 1..%d", V, B, K, SG_BODY_MAX_VERTS,
                        SG_BODY_MAX_BETAS, SG_BODY_MAX_ROWS);
    if (P < 0) return sg_failf("sg_body_shaped: P = %d pose features", P);
    if (!v_template || !shapedirs || !betas || (P > 0 && (!posedirs || !pose_feature)))
        return sg_set_error("sg_body_shaped: null pointer", hipSuccess);
    hipLaunchKernelGGL(sg_body_shaped_kernel, dim3(sgb_blocks(3LL * V), K), dim3(SGB_THREADS), 0, (hipStream_t)stream, V, B, P, v_template,
                       shapedirs, betas, posedirs, pose_feature, v_shaped, shape_offsets, pose_offsets, v_posed);
    return sg_launched("sg_body_shaped");
}

extern "C" size_t sg_body_smooth_ws_bytes(int V, int F)
{
    if (!sgb_count_ok(V, SG_BODY_MAX_VERTS) || !sgb_count_ok(F, SGB_MAX_F)) return 0;
    const unsigned nbv = sgb_blocks(V), nbf = sgb_blocks(F);
    const size_t pitch = nbv > nbf ? nbv : nbf;
    // x, nrm, delta [3V] and a [V] fp64; two rows of partials; the scalars; the normals' accumulators [3V] int64
    return (9 * (size_t)V + V + 2 * pitch + SGB_SCALARS + 3 * (size_t)V) * 8;
}

extern "C" int sg_body_smooth(int V, int F, int iterations, float lamb, const float *x0, const int32_t *faces, const int32_t *row_ptr,
                              const int32_t *col, void *ws, float *x_out, int32_t *info, void *stream)
{
    if (!sgb_count_ok(V, SG_BODY_MAX_VERTS) || !sgb_count_ok(F, SGB_MAX_F))
        return sg_failf("sg_body_smooth: V = %d / F = %d outside 1..%d / 1..%d", V, F, SG_BODY_MAX_VERTS, SGB_MAX_F);
    if (iterations < 0 || iterations > SG_BODY_MAX_ITERATIONS)
        return sg_failf("sg_body_smooth: %d iterations outside 0..%d", iterations, SG_BODY_MAX_ITERATIONS);
    if (!isfinite(lamb)) return sg_set_error("sg_body_smooth: lamb is not finite", hipSuccess);
    if (!x0 || !faces || !row_ptr || !col || !ws || !x_out || !info) return sg_set_error("sg_body_smooth: null pointer", hipSuccess);
    if (x_out == x0) return sg_set_error("sg_body_smooth: x_out may not alias x0", hipSuccess);
    const hipStream_t st = (hipStream_t)stream;
    const SgbWs w = sgb_carve(ws, V, F);
    const unsigned nbv = sgb_blocks(V), nbf = sgb_blocks(F);
    int bits = 2;                                                    // ceil(log2(4 max(F, 1)))
    while ((1LL << bits) < 4LL * F) bits++;
    const double fixed = ldexp(1.0, 61 - bits);
    const hipError_t e = hipMemsetAsync(info, 0, SG_BODY_INFO_INTS * sizeof(int32_t), st);
    if (e != hipSuccess) return sg_set_error("sg_body_smooth (info)", e);
    hipLaunchKernelGGL(sg_body_prep_kernel, dim3(nbv), dim3(SGB_THREADS), 0, st, V, x0, row_ptr, w.x, w.acc, info);
    hipLaunchKernelGGL(sg_body_faces0_kernel, dim3(nbf), dim3(SGB_THREADS), 0, st, V, F, fixed, w.x, faces, w.acc, w.partial, w.pitch, info);
    hipLaunchKernelGGL(sg_body_final0_kernel, dim3(1), dim3(SGB_THREADS), 0, st, (int)nbf, w.partial, w.pitch, w.scal);
    hipLaunchKernelGGL(sg_body_normals_kernel, dim3(nbv), dim3(SGB_THREADS), 0, st, V, w.acc, w.nrm);
    for (int i = 0; i < iterations; i++) {
        const int first = i == 0;
        hipLaunchKernelGGL(sg_body_lap_kernel, dim3(nbv), dim3(SGB_THREADS), 0, st, V, w.x, w.nrm, row_ptr, col, w.delta, w.a, w.partial);
        hipLaunchKernelGGL(sg_body_mean_kernel, dim3(1), dim3(SGB_THREADS), 0, st, (int)nbv, V, w.partial, w.scal);
        hipLaunchKernelGGL(sg_body_move_kernel, dim3(nbv), dim3(SGB_THREADS), 0, st, V, (double)lamb, w.x, w.delta, w.a, w.scal);
        hipLaunchKernelGGL(sg_body_vol_kernel, dim3(nbf), dim3(SGB_THREADS), 0, st, V, F, first, w.x, w.nrm, faces, w.scal, w.partial, w.pitch);
        hipLaunchKernelGGL(sg_body_vol_final_kernel, dim3(1), dim3(SGB_THREADS), 0, st, (int)nbf, first, w.partial, w.pitch, w.scal, info);
        hipLaunchKernelGGL(sg_body_push_kernel, dim3(nbv), dim3(SGB_THREADS), 0, st, V, w.x, w.nrm, w.scal);
    }
    hipLaunchKernelGGL(sg_body_out_kernel, dim3(sgb_blocks(3LL * V)), dim3(SGB_THREADS), 0, st, V, w.x, x_out, info);
    return sg_launched("sg_body_smooth");
}
