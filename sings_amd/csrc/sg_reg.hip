// Geometry-preserving regularisers of the SinGS trainer, forward value + gradient.
//
// Replaces (sings/rec/losses/loss_items.py, called from gs_trainer.py:355-399):
//   L2Norm                   :15-54    norms of xyz_offsets, scales - mean, large scales, low opacities
//   RegionLaplacianLoss_v2   :93-192   sum_r w_r mean((L_r x_r)^2), L_r = D^-1 A - I over same-label edges
//                                      (pytorch3d.ops.laplacian), + forward_hands
//   pytorch3d.loss.mesh_edge_loss(mesh, target_length = 0)  (gs_trainer.py:366)  mean_e |v0 - v1|^2
// All HBM / latency-bound graph work over a CSR that the caller built: gathers (no scatter, no float atomics -> deterministic),
// fixed-order two-stage reductions (sg_reduce.h).  GaussiansEdgeLoss (:57-90) and its k-NN search are in sg_knn.hip, the fused
// Laplacians of the training step in sg_mesh_terms.hip.
#include "sg_reduce.h"

// ---------------------------------------------------------------------------------------------------------
// Region Laplacian.  CSR over same-label edges (both directions), deg_inv[i] = 1/deg(i) (0 if isolated),
// vscale[i] = w_region(i) / (V_region * C) (0 for vertices outside every weighted region).
__global__ void __launch_bounds__(256)
sg_lap_fwd_kernel(int V, int C, const float *__restrict__ x, const int *__restrict__ row_ptr, const int *__restrict__ col,
                  const float *__restrict__ deg_inv, const float *__restrict__ vscale, float *__restrict__ g,
                  float *__restrict__ partial)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc[1] = { 0.0f };
    if (i < V) {
        const int r0 = row_ptr[i], r1 = row_ptr[i + 1];
        const float di = deg_inv[i], sc = vscale[i];
        for (int c = 0; c < C; c++) {
            float s = 0.0f;
            for (int e = r0; e < r1; e++) s += x[(size_t)col[e] * C + c];
            const float y = s * di - x[(size_t)i * C + c];
            acc[0] += sc * y * y;
            g[(size_t)i * C + c] = 2.0f * sc * y;                 // dLoss / dy
        }
    }
    sg_block_partials<1>(acc, partial);
}

// dL/dx = L^T g:  (L^T g)_j = sum_{i in N(j)} g_i / deg(i) - g_j   (symmetric adjacency)
__global__ void __launch_bounds__(256)
sg_lap_bwd_kernel(int V, int C, const float *__restrict__ g, const int *__restrict__ row_ptr, const int *__restrict__ col,
                  const float *__restrict__ deg_inv, const float *__restrict__ upstream, float *__restrict__ dx)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= V) return;
    const float u = upstream ? upstream[0] : 1.0f;
    const int r0 = row_ptr[j], r1 = row_ptr[j + 1];
    for (int c = 0; c < C; c++) {
        float s = 0.0f;
        for (int e = r0; e < r1; e++) { const int i = col[e]; s += g[(size_t)i * C + c] * deg_inv[i]; }
        dx[(size_t)j * C + c] = u * (s - g[(size_t)j * C + c]);
    }
}

// Cotangent variant (loss_items.py:150-165 with pytorch3d.ops.cot_laplacian): the regions OVERLAP (a region takes every face that
// touches one of its vertices), so the operator is a STACK of weighted rows -- one row per (region, vertex of that region) -- over the
// global vertex array: y_r = sum_e val_e x[col_e] (no diagonal term: cot_laplacian returns the off-diagonal weights only, and the
// reference multiplies by exactly that), loss = sum_r rscale_r |y_r|^2 with rscale_r = weight(region) / (rows of the region * C).
__global__ void __launch_bounds__(256)
sg_rows_fwd_kernel(int R, int C, const float *__restrict__ x, const int *__restrict__ row_ptr, const int *__restrict__ col,
                   const float *__restrict__ val, const float *__restrict__ rscale, float *__restrict__ g, float *__restrict__ partial)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    float acc[1] = { 0.0f };
    if (r < R) {
        const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
        const float sc = rscale[r];
        for (int c = 0; c < C; c++) {
            float y = 0.0f;
            for (int e = e0; e < e1; e++) y += val[e] * x[(size_t)col[e] * C + c];
            acc[0] += sc * y * y;
            g[(size_t)r * C + c] = 2.0f * sc * y;
        }
    }
    sg_block_partials<1>(acc, partial);
}
// dL/dx_j = sum over the entries of column j (the transposed CSR: t_row_ptr [V+1], t_row = stacked row, t_val) of val g_row
__global__ void __launch_bounds__(256)
sg_rows_bwd_kernel(int V, int C, const float *__restrict__ g, const int *__restrict__ t_row_ptr, const int *__restrict__ t_row,
                   const float *__restrict__ t_val, const float *__restrict__ upstream, float *__restrict__ dx)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= V) return;
    const float u = upstream ? upstream[0] : 1.0f;
    const int e0 = t_row_ptr[j], e1 = t_row_ptr[j + 1];
    for (int c = 0; c < C; c++) {
        float s = 0.0f;
        for (int e = e0; e < e1; e++) s += t_val[e] * g[(size_t)t_row[e] * C + c];
        dx[(size_t)j * C + c] = u * s;
    }
}

__global__ void __launch_bounds__(256)
sg_scalar_reduce_kernel(const float *__restrict__ partial, int nblocks, float scale, float *__restrict__ out)
{
    __shared__ double sums[SG_RED_MAXQ];
    sg_final_sums(partial, nblocks, 1, sums);
    if (threadIdx.x == 0) out[0] = (float)(sums[0] * (double)scale);
}

// ---------------------------------------------------------------------------------------------------------
// mesh_edge_loss(target_length = 0) = (1/E) sum_e |v0 - v1|^2 over the E unique undirected edges.
// CSR holds every edge in both directions: loss = (1/2E) sum_i sum_{j in N(i)} |v_i - v_j|^2.
__global__ void __launch_bounds__(256)
sg_mesh_edge_kernel(int V, int E, const float *__restrict__ x, const int *__restrict__ row_ptr, const int *__restrict__ col,
                    const float *__restrict__ upstream, float *__restrict__ dx, float *__restrict__ partial)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc[1] = { 0.0f };
    if (i < V) {
        const float u = upstream ? upstream[0] : 1.0f;
        const float xi = x[3 * (size_t)i], yi = x[3 * (size_t)i + 1], zi = x[3 * (size_t)i + 2];
        float gx = 0, gy = 0, gz = 0;
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++) {
            const int j = col[e];
            const float ddx = xi - x[3 * (size_t)j], ddy = yi - x[3 * (size_t)j + 1], ddz = zi - x[3 * (size_t)j + 2];
            acc[0] += ddx * ddx + ddy * ddy + ddz * ddz;
            gx += ddx; gy += ddy; gz += ddz;
        }
        const float k = 2.0f * u / (float)E;
        if (dx) { dx[3 * (size_t)i] = k * gx; dx[3 * (size_t)i + 1] = k * gy; dx[3 * (size_t)i + 2] = k * gz; }
    }
    sg_block_partials<1>(acc, partial);
}

// ---------------------------------------------------------------------------------------------------------
// L2Norm.  phase 1 partials: q0 sum s, q1 sum s^2, q2 sum |off|^2, q3 sum_{s > thr} s^2, q4 sum_{o < thr} (0.5 - o)^2
struct SgL2Args {
    int N, has_offsets, has_scales, has_opacity;
    float l_off, l_diff, l_max, max_thr, l_op, op_thr;
};
__global__ void __launch_bounds__(256)
sg_l2norm_stats_kernel(SgL2Args a, const float *__restrict__ off, const float *__restrict__ scales,
                       const float *__restrict__ opacity, float *__restrict__ partial)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    float v[5] = { 0, 0, 0, 0, 0 };
    if (i < a.N) {
        if (a.has_scales) {
            const float s = scales[3 * (size_t)i];
            v[0] = s; v[1] = s * s; v[3] = s > a.max_thr ? s * s : 0.0f;
        }
        if (a.has_offsets) {
            const float ox = off[3 * (size_t)i], oy = off[3 * (size_t)i + 1], oz = off[3 * (size_t)i + 2];
            v[2] = ox * ox + oy * oy + oz * oz;
        }
        if (a.has_opacity) {
            const float o = opacity[i];
            v[4] = o < a.op_thr ? (0.5f - o) * (0.5f - o) : 0.0f;
        }
    }
    sg_block_partials<5>(v, partial);
}
// scal: [0] loss, [1] mean s, [2..5] 1/norm of (offsets, diff, max-scale, opacity) times lambda (0 if norm == 0)
__global__ void __launch_bounds__(256)
sg_l2norm_reduce_kernel(SgL2Args a, const float *__restrict__ partial, int nblocks, float *__restrict__ scal,
                        float *__restrict__ loss_out)
{
    __shared__ double sums[SG_RED_MAXQ];
    sg_final_sums(partial, nblocks, 5, sums);
    if (threadIdx.x == 0) {
        const double n = (double)a.N, mean = sums[0] / n;
        double d2 = sums[1] - n * mean * mean;
        if (d2 < 0) d2 = 0;
        const double n_off = sqrt(sums[2]), n_diff = sqrt(d2), n_max = sqrt(sums[3]), n_op = sqrt(sums[4]);
        double loss = 0;
        if (a.has_offsets) loss += a.l_off * n_off;
        if (a.has_scales) loss += a.l_diff * n_diff + a.l_max * n_max;
        if (a.has_opacity) loss += a.l_op * n_op;
        scal[0] = (float)loss; scal[1] = (float)mean;
        scal[2] = n_off > 0 ? (float)(a.l_off / n_off) : 0.0f;
        scal[3] = n_diff > 0 ? (float)(a.l_diff / n_diff) : 0.0f;
        scal[4] = n_max > 0 ? (float)(a.l_max / n_max) : 0.0f;
        scal[5] = n_op > 0 ? (float)(a.l_op / n_op) : 0.0f;
        if (loss_out) loss_out[0] = (float)loss;
    }
}
__global__ void __launch_bounds__(256)
sg_l2norm_grad_kernel(SgL2Args a, const float *__restrict__ off, const float *__restrict__ scales,
                      const float *__restrict__ opacity, const float *__restrict__ scal,
                      const float *__restrict__ upstream, float *__restrict__ d_off, float *__restrict__ d_scales,
                      float *__restrict__ d_opacity)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const float u = upstream ? upstream[0] : 1.0f;
    if (a.has_offsets && d_off) {
        const float k = u * scal[2];
        d_off[3 * (size_t)i] = k * off[3 * (size_t)i]; d_off[3 * (size_t)i + 1] = k * off[3 * (size_t)i + 1];
        d_off[3 * (size_t)i + 2] = k * off[3 * (size_t)i + 2];
    }
    if (a.has_scales && d_scales) {
        const float s = scales[3 * (size_t)i];
        // d|s - mean| / ds_i = (d_i - mean(d)) / |d| = d_i / |d|  (sum d = 0);  + thresholded norm
        float g = scal[3] * (s - scal[1]) + (s > a.max_thr ? scal[4] * s : 0.0f);
        d_scales[3 * (size_t)i] = u * g; d_scales[3 * (size_t)i + 1] = 0.0f; d_scales[3 * (size_t)i + 2] = 0.0f;
    }
    if (a.has_opacity && d_opacity) {
        const float o = opacity[i];
        d_opacity[i] = o < a.op_thr ? -u * scal[5] * (0.5f - o) : 0.0f;
    }
}

// ---- launchers --------------------------------------------------------------------------------------------
void sg_launch_scalar_reduce(const float *partial, int nblocks, float scale, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(sg_scalar_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nblocks, scale, out);
}

size_t sg_reg_ws_bytes_impl(int n) { return sg_align((size_t)sg_nb(n) * SG_RED_MAXQ * 4) + 256; }

void sg_launch_region_laplacian(int V, int C, const float *x, const int *row_ptr, const int *col, const float *deg_inv,
                                const float *vscale, void *ws, float *g_ws, float *loss, const float *upstream,
                                float *dL_dx, hipStream_t st)
{
    float *partial = (float *)ws;
    const int nb = sg_nb(V);
    hipLaunchKernelGGL(sg_lap_fwd_kernel, dim3(nb), dim3(256), 0, st, V, C, x, row_ptr, col, deg_inv, vscale, g_ws, partial);
    if (loss) sg_launch_scalar_reduce(partial, nb, 1.0f, loss, st);
    if (dL_dx) hipLaunchKernelGGL(sg_lap_bwd_kernel, dim3(nb), dim3(256), 0, st, V, C, g_ws, row_ptr, col, deg_inv, upstream, dL_dx);
}

void sg_launch_rows_laplacian(int R, int V, int C, const float *x, const int *row_ptr, const int *col, const float *val,
                              const float *rscale, const int *t_row_ptr, const int *t_row, const float *t_val, void *ws, float *g_ws,
                              float *loss, const float *upstream, float *dL_dx, hipStream_t st)
{
    float *partial = (float *)ws;
    const int nb = sg_nb(R);
    hipLaunchKernelGGL(sg_rows_fwd_kernel, dim3(nb), dim3(256), 0, st, R, C, x, row_ptr, col, val, rscale, g_ws, partial);
    if (loss) sg_launch_scalar_reduce(partial, nb, 1.0f, loss, st);
    if (dL_dx) hipLaunchKernelGGL(sg_rows_bwd_kernel, dim3(sg_nb(V)), dim3(256), 0, st, V, C, g_ws, t_row_ptr, t_row, t_val, upstream, dL_dx);
}

void sg_launch_mesh_edge(int V, int E, const float *x, const int *row_ptr, const int *col, void *ws, float *loss,
                         const float *upstream, float *dL_dx, hipStream_t st)
{
    float *partial = (float *)ws;
    const int nb = sg_nb(V);
    hipLaunchKernelGGL(sg_mesh_edge_kernel, dim3(nb), dim3(256), 0, st, V, E, x, row_ptr, col, upstream, dL_dx, partial);
    if (loss) sg_launch_scalar_reduce(partial, nb, 0.5f / (float)E, loss, st);
}

void sg_launch_l2norm(int N, const float *off, const float *scales, const float *opacity, const float *lambdas6, void *ws,
                      float *loss, const float *upstream, float *d_off, float *d_scales, float *d_opacity, hipStream_t st)
{
    SgL2Args a;
    a.N = N; a.has_offsets = off != nullptr; a.has_scales = scales != nullptr; a.has_opacity = opacity != nullptr;
    a.l_off = lambdas6[0]; a.l_diff = lambdas6[1]; a.l_max = lambdas6[2]; a.max_thr = lambdas6[3]; a.l_op = lambdas6[4];
    a.op_thr = lambdas6[5];
    float *partial = (float *)ws;
    const int nb = sg_nb(N);
    float *scal = (float *)((char *)ws + sg_align((size_t)nb * SG_RED_MAXQ * 4));
    hipLaunchKernelGGL(sg_l2norm_stats_kernel, dim3(nb), dim3(256), 0, st, a, off, scales, opacity, partial);
    hipLaunchKernelGGL(sg_l2norm_reduce_kernel, dim3(1), dim3(256), 0, st, a, partial, nb, scal, loss);
    if (d_off || d_scales || d_opacity)
        hipLaunchKernelGGL(sg_l2norm_grad_kernel, dim3(nb), dim3(256), 0, st, a, off, scales, opacity, scal, upstream, d_off,
                           d_scales, d_opacity);
}
