// Geometry-preserving regularisers of the SinGS trainer, forward value + gradient.
//
// Replaces (sings/rec/losses/loss_items.py, called from gs_trainer.py:355-399):
//   L2Norm                   :15-54    norms of xyz_offsets, scales - mean, large scales, low opacities
//   GaussiansEdgeLoss        :57-90    ((scale_i - mean_{K-1 nearest} |x_i - x_j|)^2).mean(), K = 9 incl. self
//                                      (pytorch3d.ops.knn_points, brute force, in the reference)
//   RegionLaplacianLoss_v2   :93-192   sum_r w_r mean((L_r x_r)^2), L_r = D^-1 A - I over same-label edges
//                                      (pytorch3d.ops.laplacian), + forward_hands
//   pytorch3d.loss.mesh_edge_loss(mesh, target_length = 0)  (gs_trainer.py:366)  mean_e |v0 - v1|^2
// All HBM / latency-bound graph work: CSR gathers (no scatter, no float atomics -> deterministic), a uniform-grid
// exact k-nearest-neighbour search instead of the O(N^2) brute force, fixed-order two-stage reductions.
#include "sg_common.h"
#include "sg_knn_grid.h"

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

// ---------------------------------------------------------------------------------------------------------
// Exact k nearest neighbours on a uniform grid.  grid params live in device memory (computed on the device):
__global__ void __launch_bounds__(256)
sg_bbox_partial_kernel(int N, const float *__restrict__ xyz, float *__restrict__ partial /* [nb][8]: min xyz, max xyz */)
{
    __shared__ float sMn[4][3], sMx[4][3];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mn[3] = { 3e38f, 3e38f, 3e38f }, mx[3] = { -3e38f, -3e38f, -3e38f };
    if (i < N) {
#pragma unroll
        for (int c = 0; c < 3; c++) mn[c] = mx[c] = xyz[3 * (size_t)i + c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64)); mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64)); }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { sMn[wave][c] = mn[c]; sMx[wave][c] = mx[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        partial[(size_t)blockIdx.x * 8 + c] = fminf(fminf(sMn[0][c], sMn[1][c]), fminf(sMn[2][c], sMn[3][c]));
        partial[(size_t)blockIdx.x * 8 + 3 + c] = fmaxf(fmaxf(sMx[0][c], sMx[1][c]), fmaxf(sMx[2][c], sMx[3][c]));
    }
}
// one workgroup: bounding box -> grid (sg_knn_grid.h: cell edge h with ~max_cells cells in the box, never more)
__device__ __forceinline__ void sg_grid_setup_body(const float *__restrict__ partial, int nblocks, int N, int max_cells, SgGrid *__restrict__ grid)
{
    __shared__ float sMn[256][3], sMx[256][3];
    float mn[3] = { 3e38f, 3e38f, 3e38f }, mx[3] = { -3e38f, -3e38f, -3e38f };
    for (int b = threadIdx.x; b < nblocks; b += 256)
        for (int c = 0; c < 3; c++) { mn[c] = fminf(mn[c], partial[(size_t)b * 8 + c]); mx[c] = fmaxf(mx[c], partial[(size_t)b * 8 + 3 + c]); }
    for (int c = 0; c < 3; c++) { sMn[threadIdx.x][c] = mn[c]; sMx[threadIdx.x][c] = mx[c]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < 3; c++) {
                sMn[threadIdx.x][c] = fminf(sMn[threadIdx.x][c], sMn[threadIdx.x + s][c]);
                sMx[threadIdx.x][c] = fmaxf(sMx[threadIdx.x][c], sMx[threadIdx.x + s][c]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) sg_knn_grid_size(sMn[0], sMx[0], max_cells, grid);
}
__device__ __forceinline__ void sg_cell_of(const SgGrid &g, float x, float y, float z, int c[3])
{
    c[0] = min(max((int)((x - g.lo[0]) * g.inv_h), 0), g.dim[0] - 1);
    c[1] = min(max((int)((y - g.lo[1]) * g.inv_h), 0), g.dim[1] - 1);
    c[2] = min(max((int)((z - g.lo[2]) * g.inv_h), 0), g.dim[2] - 1);
}
__device__ __forceinline__ void sg_cell_count_body(int N, const float *__restrict__ xyz, const SgGrid *__restrict__ grid, uint32_t *__restrict__ cell_of,
                     uint32_t *__restrict__ rank_in_cell, uint32_t *__restrict__ count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const SgGrid g = *grid;
    int c[3];
    sg_cell_of(g, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], c);
    const uint32_t id = (uint32_t)((c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0]);
    cell_of[i] = id;
    rank_in_cell[i] = atomicAdd(&count[id], 1u);
}
// exclusive scan of count[0, ncells) in three steps (block sums, scan of block sums, add back); 1024 cells per block
__device__ __forceinline__ void sg_cells_scan1_body(const SgGrid *__restrict__ grid, const uint32_t *__restrict__ count, uint32_t *__restrict__ start,
                      uint32_t *__restrict__ block_sum)
{
    __shared__ uint32_t sW[4];
    const int ncells = grid->ncells;
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    if (blockIdx.x * 1024 >= ncells) return;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = base + k < ncells ? count[base + k] : 0u; s += v[k]; }
    uint32_t incl = s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) sW[wave] = incl;
    __syncthreads();
    uint32_t off = 0;
    for (int w = 0; w < wave; w++) off += sW[w];
    uint32_t ex = off + incl - s;
#pragma unroll
    for (int k = 0; k < 4; k++) { if (base + k < ncells) start[base + k] = ex; ex += v[k]; }
    if (threadIdx.x == 255) block_sum[blockIdx.x] = ex;
}
__device__ __forceinline__ void sg_cells_scan2_body(const SgGrid *__restrict__ grid, uint32_t *__restrict__ block_sum)
{
    // single workgroup, serial over chunks of 1024 block sums
    __shared__ uint32_t sW[16];
    __shared__ uint32_t carry;
    const int nb = (grid->ncells + 1023) / 1024;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const uint32_t v = i < nb ? block_sum[i] : 0u;
        uint32_t incl = v;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        if (lane == 63) sW[wave] = incl;
        __syncthreads();
        uint32_t off = carry;
        for (int w = 0; w < wave; w++) off += sW[w];
        if (i < nb) block_sum[i] = off + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = off + incl;
        __syncthreads();
    }
}
__device__ __forceinline__ void sg_cell_scatter_body(int N, const float *__restrict__ xyz, const uint32_t *__restrict__ cell_of,
                       const uint32_t *__restrict__ rank_in_cell, const uint32_t *__restrict__ start,
                       const uint32_t *__restrict__ block_sum, float4 *__restrict__ sorted /* xyz + original index */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t id = cell_of[i];
    const uint32_t slot = start[id] + block_sum[id >> 10] + rank_in_cell[i];
    sorted[slot] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float((uint32_t)i));
}

// cells[id] = (first sorted slot, count): one 8-B load per visited cell in the query
__device__ __forceinline__ void sg_cells_finalize_body(const SgGrid *__restrict__ grid, const uint32_t *__restrict__ count,
                         const uint32_t *__restrict__ start, const uint32_t *__restrict__ block_sum, uint2 *__restrict__ cells)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < grid->ncells) cells[id] = make_uint2(start[id] + block_sum[id >> 10], count[id]);
}

// The coarse and the fine grid are built by the SAME launches (blockIdx.y = level): seven launches instead of fourteen -- on a side
// stream beside the raster kernels every small launch waits for dispatch slots (5-us kernels took 12-55 us each in the training
// step's trace), so the number of launches is what the build costs.
struct SgKnnLv { SgGrid *grid; float4 *sorted; uint2 *cells; uint32_t *cell_of, *rank_in, *count, *start, *bsum; int mc; };
struct SgKnnLv2 { SgKnnLv l[2]; };
__global__ void __launch_bounds__(256)
sg_grid_setup2_kernel(const float *__restrict__ partial, int nblocks, int N, SgKnnLv2 L)
{
    const SgKnnLv &g = L.l[blockIdx.y];
    sg_grid_setup_body(partial, nblocks, N, g.mc, g.grid);
}
__global__ void __launch_bounds__(256)
sg_zero2_kernel(SgKnnLv2 L)
{
    const SgKnnLv &g = L.l[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)g.mc; i += (size_t)gridDim.x * 256) g.count[i] = 0u;
}
__global__ void __launch_bounds__(256)
sg_cell_count2_kernel(int N, const float *__restrict__ xyz, SgKnnLv2 L)
{
    const SgKnnLv &g = L.l[blockIdx.y];
    sg_cell_count_body(N, xyz, g.grid, g.cell_of, g.rank_in, g.count);
}
__global__ void __launch_bounds__(256)
sg_cells_scan1_2_kernel(SgKnnLv2 L)
{
    const SgKnnLv &g = L.l[blockIdx.y];
    sg_cells_scan1_body(g.grid, g.count, g.start, g.bsum);
}
__global__ void __launch_bounds__(1024)
sg_cells_scan2_2_kernel(SgKnnLv2 L)
{
    const SgKnnLv &g = L.l[blockIdx.y];
    sg_cells_scan2_body(g.grid, g.bsum);
}
__global__ void __launch_bounds__(256)
sg_cell_scatter2_kernel(int N, const float *__restrict__ xyz, SgKnnLv2 L)
{
    const SgKnnLv &g = L.l[blockIdx.y];
    sg_cell_scatter_body(N, xyz, g.cell_of, g.rank_in, g.start, g.bsum, g.sorted);
}
__global__ void __launch_bounds__(256)
sg_cells_finalize2_kernel(SgKnnLv2 L)
{
    const SgKnnLv &g = L.l[blockIdx.y];
    sg_cells_finalize_body(g.grid, g.count, g.start, g.bsum, g.cells);
}

// One lane per (cell-sorted) point: grow a cube of cells around the point's cell ring by ring; the K best squared
// distances sit in registers (sorted insertion).  The search is complete when the K-th best distance is no larger than
// the distance from the point to the faces of the searched cube.  Lanes of a wave are neighbours in space, so their
// candidate loads hit the same lines; candidates are fetched four at a time to keep several loads in flight.  Inside a
// ring, rows and cells farther from the point than its current K-th best are skipped (a dense point finds its K
// neighbours in its own cell and then touches 2-3 of the 26 cells around it instead of all of them).
// (Two wave-cooperative variants -- union box per wave, shared (y,z) row groups -- were slower on avatar-like clouds
//  whose density varies 100x: every sparse lane drags its whole wave through wide boxes.)
template <int K>
__device__ __forceinline__ void sg_knn_insert(float d, float best[K])
{
    if (d < best[K - 1]) {
#pragma unroll
        for (int k = 0; k < K; k++) { const float lo = fminf(best[k], d); d = fmaxf(best[k], d); best[k] = lo; }
    }
}
__device__ __forceinline__ float sg_d2(float4 q, float4 p)
{
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return dx * dx + dy * dy + dz * dz;
}

// Two grids over the same cloud: the coarse one (~4N cells) and a fine one (~32N cells, 2x smaller cells).  A point
// whose coarse cell holds more than SG_KNN_DENSE points searches the fine grid: an avatar's density varies 100x (the
// median coarse cell holds 4 points, 10 % of the points sit in cells of 300+), and a dense point otherwise compares
// itself with the ~2 500 points of its 27 coarse cells.  Either search is exact -- the level only changes the cost
// (threshold / fine-grid size swept: 24 / 64N 353 us, 16 / 32N 330 us at 150k avatar points; 128N and 16N lose).
#define SG_KNN_DENSE 16
#define SG_KNN_SUB 4                   // lanes that search for one point: the ROWS of a ring are dealt to them
template <int K>
__device__ __forceinline__ void sg_knn_merge_group(float best[K])
{
#pragma unroll
    for (int o = 1; o < SG_KNN_SUB; o <<= 1) {
        float other[K];
#pragma unroll
        for (int k = 0; k < K; k++) other[k] = __shfl_xor(best[k], o, 64);
#pragma unroll
        for (int k = 0; k < K; k++) sg_knn_insert<K>(other[k], best);
    }
}
#ifdef SG_KNN_ACCOUNT
// accounting build (tools/knn_account.sh): per point (rows iterated, rows searched, cell look-ups, candidates, inserts, rings,
// fine grid used, candidates of the busiest of its lanes)
__device__ uint32_t *sg_knn_acct;
extern "C" int sg_debug_knn_account(uint32_t *dev_buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(sg_knn_acct), &dev_buf, sizeof(dev_buf)); }
#define SG_ACCT(q, n) acct[q] += (n)
#else
#define SG_ACCT(q, n) do { } while (0)
#endif
template <int K>
__global__ void __launch_bounds__(256)
sg_knn_query_kernel(int N, const float4 *__restrict__ sorted_c, const SgGrid *__restrict__ grid_c,
                    const uint2 *__restrict__ cells_c, const float4 *__restrict__ sorted_f,
                    const SgGrid *__restrict__ grid_f, const uint2 *__restrict__ cells_f, float *__restrict__ mean_edge)
{
    // SG_KNN_SUB lanes per point.  What a lane spends its time on is the chain row -> cell look-up -> candidates ->
    // next row (ring 1 alone: 9 rows, 210 of the kernel's 320 us with one lane per point and 2.3 waves per SIMD); the
    // rows of a ring are therefore dealt round-robin to the lanes of the point, each keeps the K best of ITS rows of
    // the current ring (`mine`), the lists are merged at the end of the ring into `best` (identical in the group).
    // 150k / 500k avatar points, whole k-NN: 1 lane 450 / 1 465 us, 4 lanes 353 / 1 048, 8 lanes 394 / 1 057, 16 lanes
    // 461 / 1 376.  (Dealing the CANDIDATES of a row to 8 lanes instead left the chain as long as it was: no gain.  Cell
    // look-ups of three rows issued together + the next four candidates in flight during the inserts: 15 % slower.
    // Round 3, tools/knn_account.py: a point costs 131 distance evaluations, 21 cell look-ups and 52 inserts in 2.2 rings --
    // 2.3 KB gathered for 128 B of neighbours -- and the busiest lane of a point evaluates 60 candidates (its share would be
    // 33; 1 359 for the worst point).  Searching the runs of a round of four rows with ALL four lanes, candidates
    // interleaved, evened that out (busiest lane 37 on average, 562 at worst) and was SLOWER, 366 vs 335 us at 150k and
    // 1 204 vs 999 us at 500k: every run became its own load round-trip in every lane.  The kernel's time is the number
    // of dependent round-trips a wave makes, not the candidates of its busiest lane.)
    const int gid = blockIdx.x * 256 + threadIdx.x, j = gid & (SG_KNN_SUB - 1);
    const int s = min(gid / SG_KNN_SUB, N - 1);                  // (the tail group repeats the last point: harmless)
    const float4 p = sorted_c[s];
    SgGrid g = *grid_c;
    const uint2 *__restrict__ cells = cells_c;
    const float4 *__restrict__ sorted = sorted_c;
    int c0[3];
    sg_cell_of(g, p.x, p.y, p.z, c0);
    if (cells_c[(c0[2] * g.dim[1] + c0[1]) * g.dim[0] + c0[0]].y > SG_KNN_DENSE) {
        g = *grid_f; cells = cells_f; sorted = sorted_f;
        sg_cell_of(g, p.x, p.y, p.z, c0);
    }
    const float cx = (p.x - g.lo[0]) * g.inv_h, cy = (p.y - g.lo[1]) * g.inv_h, cz = (p.z - g.lo[2]) * g.inv_h;
    float best[K], mine[K];
#ifdef SG_KNN_ACCOUNT
    uint32_t acct[8] = { 0, 0, 0, 0, 0, 0, sorted == sorted_f ? 1u : 0u, 0 };
#endif
#pragma unroll
    for (int k = 0; k < K; k++) { best[k] = 3e38f; mine[k] = 3e38f; }
    const int rmax = max(max(g.dim[0], g.dim[1]), g.dim[2]);
    const float inv_h2 = g.inv_h * g.inv_h;
    for (int r = 0; r <= rmax; r++) {
        const int x0 = max(c0[0] - r, 0), x1 = min(c0[0] + r, g.dim[0] - 1);
        const int y0 = max(c0[1] - r, 0), y1 = min(c0[1] + r, g.dim[1] - 1);
        const int z0 = max(c0[2] - r, 0), z1 = min(c0[2] + r, g.dim[2] - 1);
        const int ny = y1 - y0 + 1, nrows = ny * (z1 - z0 + 1);
        for (int i = j; i < nrows; i += SG_KNN_SUB) {
            const int z = z0 + i / ny, y = y0 + i % ny;
            // squared distance (in cell units) from p to the row of cells (y, z): rows and cells farther than the K-th best
            // so far (finished rings and this lane's rows of the current one; inf until K points are known) cannot improve
            // the result and are skipped (0.999 / 1.001: rounding of the cell maths)
            const float ez = fmaxf(fmaxf((float)z - cz, cz - (float)(z + 1)), 0.0f);
            const float ey = fmaxf(fmaxf((float)y - cy, cy - (float)(y + 1)), 0.0f);
            const float lim = fminf(best[K - 1], mine[K - 1]) * inv_h2;
            const float dyz = (ey * ey + ez * ez) * 0.999f;
            SG_ACCT(0, 1);
            if (dyz >= lim) continue;
            SG_ACCT(1, 1);
            const bool shell_row = (abs(z - c0[2]) == r) || (abs(y - c0[1]) == r);
            const uint32_t row = (uint32_t)((z * g.dim[1] + y) * g.dim[0]);
            if (shell_row) {
                // the x range of the ring, cut to the cells within the K-th best distance, is ONE contiguous run of the
                // sorted array
                int xa = x0, xb = x1;
                if (lim < 1e30f) {
                    const float rad = sqrtf(lim - dyz) * 1.001f + 1e-3f;
                    xa = max(xa, (int)floorf(cx - rad)); xb = min(xb, (int)floorf(cx + rad));
                    if (xa > xb) continue;
                }
                const uint2 ca = cells[row + xa], cb = cells[row + xb];
                uint32_t t = ca.x;
                const uint32_t e = cb.x + cb.y;
                SG_ACCT(2, 2); SG_ACCT(3, e - t);
                for (; t + 4 <= e; t += 4) {
                    const float4 q0 = sorted[t], q1 = sorted[t + 1], q2 = sorted[t + 2], q3 = sorted[t + 3];
                    const float d0 = sg_d2(q0, p), d1 = sg_d2(q1, p), d2 = sg_d2(q2, p), d3 = sg_d2(q3, p);
                    if (d0 < best[K - 1]) { SG_ACCT(4, d0 < mine[K - 1]); sg_knn_insert<K>(d0, mine); }
                    if (d1 < best[K - 1]) { SG_ACCT(4, d1 < mine[K - 1]); sg_knn_insert<K>(d1, mine); }
                    if (d2 < best[K - 1]) { SG_ACCT(4, d2 < mine[K - 1]); sg_knn_insert<K>(d2, mine); }
                    if (d3 < best[K - 1]) { SG_ACCT(4, d3 < mine[K - 1]); sg_knn_insert<K>(d3, mine); }
                }
                for (; t < e; t++) { const float d = sg_d2(sorted[t], p); if (d < best[K - 1]) { SG_ACCT(4, d < mine[K - 1]); sg_knn_insert<K>(d, mine); } }
            } else {
                // interior row: only the two end cells (if they are at distance r in x)
                for (int side = 0; side < 2; side++) {
                    const int x = side ? c0[0] + r : c0[0] - r;
                    if (x < 0 || x >= g.dim[0]) continue;
                    const float ex = fmaxf(fmaxf((float)x - cx, cx - (float)(x + 1)), 0.0f);
                    if (dyz + ex * ex * 0.999f >= fminf(best[K - 1], mine[K - 1]) * inv_h2) continue;
                    const uint2 cc = cells[row + x];
                    SG_ACCT(2, 1); SG_ACCT(3, cc.y);
                    for (uint32_t t = cc.x; t < cc.x + cc.y; t++) {
                        const float d = sg_d2(sorted[t], p);
                        if (d < best[K - 1]) { SG_ACCT(4, d < mine[K - 1]); sg_knn_insert<K>(d, mine); }
                    }
                }
            }
        }
        // this ring's candidates: K best of the group's lists, then into the running list; the lanes' lists start empty again
        SG_ACCT(5, j == 0);
        sg_knn_merge_group<K>(mine);
#pragma unroll
        for (int k = 0; k < K; k++) { sg_knn_insert<K>(mine[k], best); mine[k] = 3e38f; }
        // distance from p to the nearest face of the searched cube that is not the grid boundary
        float reach = 3e38f;
        if (c0[0] - r > 0) reach = fminf(reach, cx - (float)(c0[0] - r));
        if (c0[0] + r < g.dim[0] - 1) reach = fminf(reach, (float)(c0[0] + r + 1) - cx);
        if (c0[1] - r > 0) reach = fminf(reach, cy - (float)(c0[1] - r));
        if (c0[1] + r < g.dim[1] - 1) reach = fminf(reach, (float)(c0[1] + r + 1) - cy);
        if (c0[2] - r > 0) reach = fminf(reach, cz - (float)(c0[2] - r));
        if (c0[2] + r < g.dim[2] - 1) reach = fminf(reach, (float)(c0[2] + r + 1) - cz);
        if (reach > 1e37f) break;                               // the cube covers the whole grid
        reach = fmaxf(reach, 0.0f) * g.h * 0.9999f;             // (conservative against the rounding of the cell maths)
        if (best[K - 1] <= reach * reach) break;
    }
    // mean Euclidean distance to the K-1 nearest OTHER points (best[0] is the point itself, distance 0)
    float m = 0.0f;
#pragma unroll
    for (int k = 1; k < K; k++) m += sqrtf(best[k]);
    if (j == 0 && gid / SG_KNN_SUB < N) mean_edge[__float_as_uint(p.w)] = m / (float)(K - 1);
#ifdef SG_KNN_ACCOUNT
    if (sg_knn_acct && gid / SG_KNN_SUB < N) {
        uint32_t *o = sg_knn_acct + 8 * (size_t)__float_as_uint(p.w);
        for (int q = 0; q < 6; q++) atomicAdd(&o[q], acct[q]);
        if (j == 0) o[6] = acct[6];
        atomicMax(&o[7], acct[3]);
    }
#endif
}

// loss = mean((s_i - l_i)^2), dL/ds_i = 2 (s_i - l_i) / N   (edge lengths are detached in the reference)
__global__ void __launch_bounds__(256)
sg_edge_loss_kernel(int N, const float *__restrict__ scales, const float *__restrict__ mean_edge,
                    const float *__restrict__ upstream, float *__restrict__ d_scales, float *__restrict__ partial)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc[1] = { 0.0f };
    if (i < N) {
        const float u = upstream ? upstream[0] : 1.0f;
        const float d = scales[3 * (size_t)i] - mean_edge[i];
        acc[0] = d * d;
        if (d_scales) { d_scales[3 * (size_t)i] = u * 2.0f * d / (float)N; d_scales[3 * (size_t)i + 1] = 0.0f; d_scales[3 * (size_t)i + 2] = 0.0f; }
    }
    sg_block_partials<1>(acc, partial);
}

// ---- launchers --------------------------------------------------------------------------------------------
static inline int sg_nb(int n) { return (n + 255) / 256 > 0 ? (n + 255) / 256 : 1; }

size_t sg_reg_ws_bytes_impl(int n) { return sg_align((size_t)sg_nb(n) * SG_RED_MAXQ * 4) + 256; }

void sg_launch_region_laplacian(int V, int C, const float *x, const int *row_ptr, const int *col, const float *deg_inv,
                                const float *vscale, void *ws, float *g_ws, float *loss, const float *upstream,
                                float *dL_dx, hipStream_t st)
{
    float *partial = (float *)ws;
    const int nb = sg_nb(V);
    hipLaunchKernelGGL(sg_lap_fwd_kernel, dim3(nb), dim3(256), 0, st, V, C, x, row_ptr, col, deg_inv, vscale, g_ws, partial);
    if (loss) hipLaunchKernelGGL(sg_scalar_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nb, 1.0f, loss);
    if (dL_dx) hipLaunchKernelGGL(sg_lap_bwd_kernel, dim3(nb), dim3(256), 0, st, V, C, g_ws, row_ptr, col, deg_inv, upstream, dL_dx);
}

void sg_launch_rows_laplacian(int R, int V, int C, const float *x, const int *row_ptr, const int *col, const float *val,
                              const float *rscale, const int *t_row_ptr, const int *t_row, const float *t_val, void *ws, float *g_ws,
                              float *loss, const float *upstream, float *dL_dx, hipStream_t st)
{
    float *partial = (float *)ws;
    const int nb = sg_nb(R);
    hipLaunchKernelGGL(sg_rows_fwd_kernel, dim3(nb), dim3(256), 0, st, R, C, x, row_ptr, col, val, rscale, g_ws, partial);
    if (loss) hipLaunchKernelGGL(sg_scalar_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nb, 1.0f, loss);
    if (dL_dx) hipLaunchKernelGGL(sg_rows_bwd_kernel, dim3(sg_nb(V)), dim3(256), 0, st, V, C, g_ws, t_row_ptr, t_row, t_val, upstream, dL_dx);
}

void sg_launch_mesh_edge(int V, int E, const float *x, const int *row_ptr, const int *col, void *ws, float *loss,
                         const float *upstream, float *dL_dx, hipStream_t st)
{
    float *partial = (float *)ws;
    const int nb = sg_nb(V);
    hipLaunchKernelGGL(sg_mesh_edge_kernel, dim3(nb), dim3(256), 0, st, V, E, x, row_ptr, col, upstream, dL_dx, partial);
    if (loss) hipLaunchKernelGGL(sg_scalar_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nb, 0.5f / (float)E, loss);
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

// workspace of the k-NN search: partials, then per grid (coarse, fine): grid struct, per-point cell / rank, sorted points,
// cell counters + starts + block sums + (start, count) pairs
static size_t sg_knn_grid_bytes(size_t n, size_t mc)
{
    return 256 + 2 * sg_align(n * 4) + sg_align(n * 16) + 2 * sg_align(mc * 4) + sg_align(((mc + 1023) / 1024) * 4) + sg_align(mc * 8);
}
size_t sg_knn_ws_bytes_impl(int N)
{
    const size_t n = N > 0 ? N : 1;
    return sg_align((size_t)sg_nb(N) * 32) + sg_align((size_t)sg_nb(N) * SG_RED_MAXQ * 4) + sg_align(n * 4) +
           sg_knn_grid_bytes(n, sg_knn_max_cells(N)) + sg_knn_grid_bytes(n, sg_knn_max_cells_fine(N));
}
struct SgKnnGrid { SgGrid *grid; float4 *sorted; uint2 *cells; uint32_t *cell_of, *rank_in, *count, *start, *bsum; size_t mc; };
// where one grid's arrays live in the workspace (no launches)
static void sg_knn_grid_at(int N, size_t mc, char *&b, SgKnnGrid *g)
{
    const size_t n = N;
    g->mc = mc;
    g->grid = (SgGrid *)b; b += 256;
    g->cell_of = (uint32_t *)b; b += sg_align(n * 4);
    g->rank_in = (uint32_t *)b; b += sg_align(n * 4);
    g->sorted = (float4 *)b; b += sg_align(n * 16);
    g->count = (uint32_t *)b; b += sg_align(mc * 4);
    g->start = (uint32_t *)b; b += sg_align(mc * 4);
    g->bsum = (uint32_t *)b; b += sg_align(((mc + 1023) / 1024) * 4);
    g->cells = (uint2 *)b; b += sg_align(mc * 8);
}
struct SgKnnWs { float *bpart, *partial, *medge; SgKnnGrid gc, gf; };
static SgKnnWs sg_knn_ws_at(int N, void *ws)
{
    const size_t n = N;
    SgKnnWs w;
    char *b = (char *)ws;
    w.bpart = (float *)b; b += sg_align((size_t)sg_nb(N) * 32);
    w.partial = (float *)b; b += sg_align((size_t)sg_nb(N) * SG_RED_MAXQ * 4);
    w.medge = (float *)b; b += sg_align(n * 4);
    sg_knn_grid_at(N, sg_knn_max_cells(N), b, &w.gc);
    sg_knn_grid_at(N, sg_knn_max_cells_fine(N), b, &w.gf);
    return w;
}
// bounding box partials -> grid -> counting sort of the points by cell
// bounding box partials -> both grids -> counting sort of the points by cell, both levels per launch
static void sg_knn_build2(int N, const float *xyz, const float *bpart, const SgKnnGrid &gc, const SgKnnGrid &gf, hipStream_t st)
{
    SgKnnLv2 L;
    const SgKnnGrid *gs[2] = { &gc, &gf };
    size_t mcmax = 0;
    for (int k = 0; k < 2; k++) {
        const SgKnnGrid &g = *gs[k];
        L.l[k] = SgKnnLv{ g.grid, g.sorted, g.cells, g.cell_of, g.rank_in, g.count, g.start, g.bsum, (int)g.mc };
        mcmax = g.mc > mcmax ? g.mc : mcmax;
    }
    const int nb = sg_nb(N), ncb = (int)((mcmax + 1023) / 1024);
    hipLaunchKernelGGL(sg_grid_setup2_kernel, dim3(1, 2), dim3(256), 0, st, bpart, nb, N, L);
    hipLaunchKernelGGL(sg_zero2_kernel, dim3(1024, 2), dim3(256), 0, st, L);
    hipLaunchKernelGGL(sg_cell_count2_kernel, dim3(nb, 2), dim3(256), 0, st, N, xyz, L);
    hipLaunchKernelGGL(sg_cells_scan1_2_kernel, dim3(ncb, 2), dim3(256), 0, st, L);
    hipLaunchKernelGGL(sg_cells_scan2_2_kernel, dim3(1, 2), dim3(1024), 0, st, L);
    hipLaunchKernelGGL(sg_cell_scatter2_kernel, dim3(nb, 2), dim3(256), 0, st, N, xyz, L);
    hipLaunchKernelGGL(sg_cells_finalize2_kernel, dim3((unsigned)((mcmax + 255) / 256), 2), dim3(256), 0, st, L);
}

// first half: the two grids over the cloud (eight small launches: both levels per launch); second half: the query + the loss.  One call does both
// (sg_gaussian_edge_loss); a caller that wants the latency-bound grid builds early and the GPU-filling query later -- beside
// kernels with idle issue slots instead of beside a chain of small ones -- makes the two calls itself on the same workspace.
void sg_launch_knn_prepare(int N, const float *xyz, void *ws, hipStream_t st)
{
    const SgKnnWs w = sg_knn_ws_at(N, ws);
    hipLaunchKernelGGL(sg_bbox_partial_kernel, dim3(sg_nb(N)), dim3(256), 0, st, N, xyz, w.bpart);
    sg_knn_build2(N, xyz, w.bpart, w.gc, w.gf, st);
}
int sg_launch_knn_finish(int N, int K, const float *scales, void *ws, float *mean_edge_out, float *loss, const float *upstream,
                         float *d_scales, hipStream_t st)
{
    if (K != 9 && K != 5 && K != 17) return 1;
    const SgKnnWs w = sg_knn_ws_at(N, ws);
    const SgKnnGrid &gc = w.gc, &gf = w.gf;
    float *medge = mean_edge_out ? mean_edge_out : w.medge;
    float *partial = w.partial;
    const int nb = sg_nb(N);
    const int nbq = (int)(((size_t)N * SG_KNN_SUB + 255) / 256);
    if (K == 9) hipLaunchKernelGGL(sg_knn_query_kernel<9>, dim3(nbq), dim3(256), 0, st, N, gc.sorted, gc.grid, gc.cells, gf.sorted, gf.grid, gf.cells, medge);
    else if (K == 5) hipLaunchKernelGGL(sg_knn_query_kernel<5>, dim3(nbq), dim3(256), 0, st, N, gc.sorted, gc.grid, gc.cells, gf.sorted, gf.grid, gf.cells, medge);
    else hipLaunchKernelGGL(sg_knn_query_kernel<17>, dim3(nbq), dim3(256), 0, st, N, gc.sorted, gc.grid, gc.cells, gf.sorted, gf.grid, gf.cells, medge);
    if (scales && (loss || d_scales)) {
        hipLaunchKernelGGL(sg_edge_loss_kernel, dim3(nb), dim3(256), 0, st, N, scales, medge, upstream, d_scales, partial);
        if (loss) hipLaunchKernelGGL(sg_scalar_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nb, 1.0f / (float)N, loss);
    }
    return 0;
}
int sg_launch_knn_edge(int N, int K, const float *xyz, const float *scales, void *ws, float *mean_edge_out, float *loss,
                       const float *upstream, float *d_scales, hipStream_t st)
{
    if (K != 9 && K != 5 && K != 17) return 1;
    sg_launch_knn_prepare(N, xyz, ws, st);
    return sg_launch_knn_finish(N, K, scales, ws, mean_edge_out, loss, upstream, d_scales, st);
}

// =============================================================================================================
// Mesh terms of the training step (include/sings_mesh_terms.h): the region Laplacian of the anchor positions, the region Laplacian of
// the DC colours and the hand Laplacian (loss_items.py:93-192 as gs_trainer.py:366-399 calls them) in ONE forward and ONE backward
// launch over one CSR, and that CSR -- with its degrees, label counts and per-vertex scales -- built on the device.
#include "sg_host.h"
#include "../../include/sings_mesh_terms.h"

// ---- the build.  Integer atomics for counts and slots only; the slots of a row are sorted afterwards, so every output is a pure
// function of the inputs (two builds: the same bits).
__global__ void __launch_bounds__(256)
sg_mt_zero_kernel(int V, int L, int *__restrict__ deg, int *__restrict__ count, int *__restrict__ info)
{
    const size_t n = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)V; i += n) deg[i] = 0;
    if (count) for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)L; i += n) count[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < SG_MESH_TERMS_INFO_INTS) info[threadIdx.x] = 0;
}
// an edge row that may be dereferenced: 0 <= a < b < V; it counts when both labels agree (and are labels at all)
__device__ __forceinline__ bool sg_mt_edge(int V, int L, const int *__restrict__ edges, const int *__restrict__ label, int e, int &a, int &b,
                                           bool &bad)
{
    a = edges[2 * (size_t)e]; b = edges[2 * (size_t)e + 1];
    bad = !(a >= 0 && a < b && b < V);
    if (bad) return false;
    if (!label) return true;
    const int la = label[a];
    return la == label[b] && (unsigned)la < (unsigned)L;
}
__global__ void __launch_bounds__(256)
sg_mt_count_kernel(int V, int E, int L, const int *__restrict__ edges, const int *__restrict__ label, int *__restrict__ deg,
                   int *__restrict__ count, int *__restrict__ info)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (label && t < V) {
        const int l = label[t];
        if ((unsigned)l >= (unsigned)L) atomicOr(&info[0], SG_MESH_TERMS_BAD_LABEL);
        else atomicAdd(&count[l], 1);
    }
    if (t < E) {
        int a, b; bool bad;
        if (sg_mt_edge(V, L, edges, label, t, a, b, bad)) { atomicAdd(&deg[a], 1); atomicAdd(&deg[b], 1); }
        else if (bad) atomicOr(&info[0], SG_MESH_TERMS_BAD_EDGE);
    }
}
// row_ptr = exclusive scan of deg, one workgroup of 1024: thread t owns the rows [t chunk, (t + 1) chunk)
__global__ void __launch_bounds__(1024)
sg_mt_scan_kernel(int V, const int *__restrict__ deg, int *__restrict__ row_ptr, int *__restrict__ info)
{
    __shared__ int sW[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (V + 1023) / 1024;
    const int lo = min(tid * chunk, V), hi = min(lo + chunk, V);
    int s = 0;
    for (int i = lo; i < hi; i++) s += deg[i];
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) sW[wave] = incl;
    __syncthreads();
    int run = incl - s;
    for (int w = 0; w < wave; w++) run += sW[w];
    for (int i = lo; i < hi; i++) { row_ptr[i] = run; run += deg[i]; }
    if (tid == 1023) { row_ptr[V] = run; info[1] = run; }
}
__global__ void __launch_bounds__(256)
sg_mt_fill_kernel(int V, int E, int L, const int *__restrict__ edges, const int *__restrict__ label, const int *__restrict__ row_ptr,
                  int *__restrict__ deg, int *__restrict__ col)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= E) return;
    int a, b; bool bad;
    if (!sg_mt_edge(V, L, edges, label, t, a, b, bad)) return;
    // (deg counts down to zero: a slot in [0, deg) per entry, any order -- the rows are sorted next)
    col[row_ptr[a] + atomicSub(&deg[a], 1) - 1] = b;
    col[row_ptr[b] + atomicSub(&deg[b], 1) - 1] = a;
}
__device__ __forceinline__ void sg_mt_sift(int *__restrict__ h, int root, int n)
{
    const int v = h[root];
    for (;;) {
        int c = 2 * root + 1;
        if (c >= n) break;
        if (c + 1 < n && h[c + 1] > h[c]) c++;
        if (h[c] <= v) break;
        h[root] = h[c]; root = c;
    }
    h[root] = v;
}
// per vertex: its columns ascending (heap sort in place: the pole of a sphere has a valence beyond any fixed register array),
// 1 / degree, and the three scales  w[label] / (count[label] * 3)  (position, colour, hand; C = 3 channels each)
__global__ void __launch_bounds__(256)
sg_mt_rows_kernel(int V, int L, const int *__restrict__ label, const float *__restrict__ w_pos, const float *__restrict__ w_col,
                  const float *__restrict__ w_hand, const int *__restrict__ row_ptr, int *__restrict__ col, const int *__restrict__ count,
                  float *__restrict__ deg_inv, float *__restrict__ vscale)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const int r0 = row_ptr[i], n = row_ptr[i + 1] - r0;
    int *h = col + r0;
    for (int k = n / 2 - 1; k >= 0; k--) sg_mt_sift(h, k, n);
    for (int m = n - 1; m > 0; m--) { const int t = h[0]; h[0] = h[m]; h[m] = t; sg_mt_sift(h, 0, m); }
    deg_inv[i] = n > 0 ? 1.0f / (float)n : 0.0f;
    if (!label) return;
    const int l = label[i];
    float s[3] = { 0.0f, 0.0f, 0.0f };
    if ((unsigned)l < (unsigned)L) {
        const float d = (float)count[l] * 3.0f;
        s[0] = w_pos[l] / d; s[1] = w_col[l] / d; s[2] = w_hand[l] / d;
    }
    vscale[3 * (size_t)i] = s[0]; vscale[3 * (size_t)i + 1] = s[1]; vscale[3 * (size_t)i + 2] = s[2];
}

// ---- the fused terms.  Slab q of g [3][V][3] holds dLoss_q / dy of term q (0 position, 1 colour, 2 hand), weighted by term_w[q].
struct SgMtIn { const float *xyz, *scales, *normals, *colour; int cstride; };
// xyz_canon of vertex j and its anchor  xyz + mean(scales) n / 2  (sings_hybrid.py:441-443), formed where it is read
__device__ __forceinline__ void sg_mt_point(const SgMtIn &in, int j, float p[3], float an[3], float c[3])
{
    const size_t o = 3 * (size_t)j;
    const float m = ((in.scales[o] + in.scales[o + 1]) + in.scales[o + 2]) / 3.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p[k] = in.xyz[o + k];
        an[k] = p[k] + m * in.normals[o + k] * 0.5f;
        c[k] = in.colour[(size_t)j * in.cstride + k];
    }
}
__global__ void __launch_bounds__(256)
sg_mesh_terms_fwd_kernel(int V, SgMtIn in, const int *__restrict__ row_ptr, const int *__restrict__ col, const float *__restrict__ deg_inv,
                         const float *__restrict__ vscale, const float *__restrict__ term_w, float *__restrict__ g,
                         float *__restrict__ partial)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc[3] = { 0.0f, 0.0f, 0.0f };
    if (i < V) {
        const int r0 = row_ptr[i], r1 = row_ptr[i + 1];
        float sp[3] = { 0, 0, 0 }, sa[3] = { 0, 0, 0 }, sc[3] = { 0, 0, 0 }, p[3], an[3], c[3];
        for (int e = r0; e < r1; e++) {
            sg_mt_point(in, col[e], p, an, c);
#pragma unroll
            for (int k = 0; k < 3; k++) { sp[k] += p[k]; sa[k] += an[k]; sc[k] += c[k]; }
        }
        sg_mt_point(in, i, p, an, c);
        const float di = deg_inv[i];
        float k2[3];
#pragma unroll
        for (int q = 0; q < 3; q++) k2[q] = 2.0f * (term_w[q] * vscale[3 * (size_t)i + q]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float y[3] = { sa[k] * di - an[k], sc[k] * di - c[k], sp[k] * di - p[k] };
#pragma unroll
            for (int q = 0; q < 3; q++) {
                acc[q] += vscale[3 * (size_t)i + q] * y[q] * y[q];
                g[((size_t)q * V + i) * 3 + k] = k2[q] * y[q];
            }
        }
    }
    sg_block_partials<3>(acc, partial);
}
__global__ void __launch_bounds__(256)
sg_mesh_terms_reduce_kernel(const float *__restrict__ partial, int nblocks, const float *__restrict__ term_w, float *__restrict__ terms)
{
    __shared__ double sums[SG_RED_MAXQ];
    sg_final_sums(partial, nblocks, 3, sums);
    if (threadIdx.x < 3) terms[threadIdx.x] = (float)(sums[threadIdx.x] * (double)term_w[threadIdx.x]);
}
// L^T g of the three slabs in one gather; d anchor / d scales_k = n / 6 for each of the three columns
__global__ void __launch_bounds__(256)
sg_mesh_terms_bwd_kernel(int V, const float *__restrict__ g, const float *__restrict__ normals, const int *__restrict__ row_ptr,
                         const int *__restrict__ col, const float *__restrict__ deg_inv, const float *__restrict__ upstream,
                         float *__restrict__ d_xyz, float *__restrict__ d_scales, float *__restrict__ d_colour)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= V) return;
    const float u = upstream ? upstream[0] : 1.0f;
    float s[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int e = row_ptr[j]; e < row_ptr[j + 1]; e++) {
        const int i = col[e];
        const float d = deg_inv[i];
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int k = 0; k < 3; k++) s[3 * q + k] += g[((size_t)q * V + i) * 3 + k] * d;
    }
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int k = 0; k < 3; k++) s[3 * q + k] -= g[((size_t)q * V + j) * 3 + k];
    const size_t o = 3 * (size_t)j;
    if (d_xyz) { d_xyz[o] = u * (s[0] + s[6]); d_xyz[o + 1] = u * (s[1] + s[7]); d_xyz[o + 2] = u * (s[2] + s[8]); }
    if (d_colour) { d_colour[o] = u * s[3]; d_colour[o + 1] = u * s[4]; d_colour[o + 2] = u * s[5]; }
    if (d_scales) {
        const float ds = u * (((normals[o] * s[0] + normals[o + 1] * s[1]) + normals[o + 2] * s[2]) / 6.0f);
        d_scales[o] = ds; d_scales[o + 1] = ds; d_scales[o + 2] = ds;
    }
}

// ---- entry points (include/sings_mesh_terms.h)
extern "C" int sg_mesh_terms_build(int V, int E, int L, const int32_t *edges, const int32_t *vertex_label, const float *w_pos,
                                   const float *w_col, const float *w_hand, int32_t *row_ptr, int32_t *col, float *deg_inv,
                                   int32_t *count, float *vscale, int32_t *deg_ws, int32_t *info, void *stream)
{
    if (V < 1 || V > (1 << 30)) return sg_set_error("sg_mesh_terms_build: V must be 1..2^30", hipSuccess);
    if (E < 0 || E >= (1 << 30)) return sg_set_error("sg_mesh_terms_build: E must be 0..2^30 - 1", hipSuccess);
    if (vertex_label && L < 1) return sg_set_error("sg_mesh_terms_build: L must be >= 1", hipSuccess);
    if ((E > 0 && (!edges || !col)) || !row_ptr || !deg_inv || !deg_ws || !info ||
        (vertex_label && (!w_pos || !w_col || !w_hand || !count || !vscale)))
        return sg_set_error("sg_mesh_terms_build: null pointer", hipSuccess);
    const hipStream_t st = (hipStream_t)stream;
    const int nbv = sg_nb(V), nbe = sg_nb(V > E ? V : E);
    int *cnt = vertex_label ? count : nullptr;
    hipLaunchKernelGGL(sg_mt_zero_kernel, dim3(nbv < 1024 ? nbv : 1024), dim3(256), 0, st, V, L, deg_ws, cnt, info);
    hipLaunchKernelGGL(sg_mt_count_kernel, dim3(nbe), dim3(256), 0, st, V, E, L, edges, vertex_label, deg_ws, cnt, info);
    hipLaunchKernelGGL(sg_mt_scan_kernel, dim3(1), dim3(1024), 0, st, V, deg_ws, row_ptr, info);
    if (E > 0) hipLaunchKernelGGL(sg_mt_fill_kernel, dim3(sg_nb(E)), dim3(256), 0, st, V, E, L, edges, vertex_label, row_ptr, deg_ws, col);
    hipLaunchKernelGGL(sg_mt_rows_kernel, dim3(nbv), dim3(256), 0, st, V, L, vertex_label, w_pos, w_col, w_hand, row_ptr, col, cnt, deg_inv,
                       vscale);
    return sg_launched("sg_mesh_terms_build");
}

extern "C" int sg_mesh_terms(int V, const float *xyz_canon, const float *scales, const float *normals, const float *colour,
                             int colour_stride, const int32_t *row_ptr, const int32_t *col, const float *deg_inv, const float *vscale,
                             const float *term_w, void *ws, float *g_ws, float *terms, const float *upstream, float *d_xyz_canon,
                             float *d_scales, float *d_colour, void *stream)
{
    if (V < 1 || V > (1 << 30)) return sg_set_error("sg_mesh_terms: V must be 1..2^30", hipSuccess);
    if (colour_stride < 3) return sg_set_error("sg_mesh_terms: the colour rows are at least 3 floats apart", hipSuccess);
    if (!xyz_canon || !scales || !normals || !colour || !row_ptr || !col || !deg_inv || !vscale || !term_w || !ws || !g_ws || !terms)
        return sg_set_error("sg_mesh_terms: null pointer", hipSuccess);
    const hipStream_t st = (hipStream_t)stream;
    const int nb = sg_nb(V);
    const SgMtIn in = { xyz_canon, scales, normals, colour, colour_stride };
    float *partial = (float *)ws;
    hipLaunchKernelGGL(sg_mesh_terms_fwd_kernel, dim3(nb), dim3(256), 0, st, V, in, row_ptr, col, deg_inv, vscale, term_w, g_ws, partial);
    hipLaunchKernelGGL(sg_mesh_terms_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nb, term_w, terms);
    if (d_xyz_canon || d_scales || d_colour)
        hipLaunchKernelGGL(sg_mesh_terms_bwd_kernel, dim3(nb), dim3(256), 0, st, V, g_ws, normals, row_ptr, col, deg_inv, upstream,
                           d_xyz_canon, d_scales, d_colour);
    return sg_launched("sg_mesh_terms");
}
