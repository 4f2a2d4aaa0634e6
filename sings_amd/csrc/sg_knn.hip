// GaussiansEdgeLoss of the SinGS trainer (sings/rec/losses/loss_items.py:57-90, called from gs_trainer.py:355-399), forward value +
// gradient:  ((scale_i - mean_{K-1 nearest} |x_i - x_j|)^2).mean(), K = 9 incl. self (pytorch3d.ops.knn_points, brute force, in the
// reference).  Here: an exact k-nearest-neighbour search on two uniform grids built on the device -- bounding box, grid sizing
// (sg_knn_grid.h), counting sort of the points by cell (the scan of sg_scan.h), query -- and the fixed-order sum of sg_reduce.h.
// No float atomics: deterministic.
#include "sg_reduce.h"
#include "sg_scan.h"
#include "sg_knn_grid.h"

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
__device__ __forceinline__ void sg_cell_of(const SgGrid &g, float x, float y, float z, int c[3])
{
    c[0] = min(max((int)((x - g.lo[0]) * g.inv_h), 0), g.dim[0] - 1);
    c[1] = min(max((int)((y - g.lo[1]) * g.inv_h), 0), g.dim[1] - 1);
    c[2] = min(max((int)((z - g.lo[2]) * g.inv_h), 0), g.dim[2] - 1);
}

// One grid's arrays in the workspace: the grid struct, per-point cell / rank, the points sorted by cell (xyz + original index), cell
// counters + starts + block sums + (first sorted slot, count) pairs; mc = the cell budget the arrays are sized for.
// The coarse and the fine grid are built by the SAME launches (blockIdx.y = level): seven launches instead of fourteen -- on a side
// stream beside the raster kernels every small launch waits for dispatch slots (5-us kernels took 12-55 us each in the training
// step's trace), so the number of launches is what the build costs.
struct SgKnnGrid { SgGrid *grid; float4 *sorted; uint2 *cells; uint32_t *cell_of, *rank_in, *count, *start, *bsum; size_t mc; };
struct SgKnnGrids { SgKnnGrid l[2]; };

// one workgroup: bounding box -> grid (sg_knn_grid.h: cell edge h with ~max_cells cells in the box, never more)
__global__ void __launch_bounds__(256)
sg_grid_setup2_kernel(const float *__restrict__ partial, int nblocks, int N, SgKnnGrids L)
{
    const SgKnnGrid &g = L.l[blockIdx.y];
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
    if (threadIdx.x == 0) sg_knn_grid_size(sMn[0], sMx[0], (int)g.mc, g.grid);
}
__global__ void __launch_bounds__(256)
sg_zero2_kernel(SgKnnGrids L)
{
    const SgKnnGrid &g = L.l[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < g.mc; i += (size_t)gridDim.x * 256) g.count[i] = 0u;
}
__global__ void __launch_bounds__(256)
sg_cell_count2_kernel(int N, const float *__restrict__ xyz, SgKnnGrids L)
{
    const SgKnnGrid &g = L.l[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const SgGrid gr = *g.grid;
    int c[3];
    sg_cell_of(gr, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], c);
    const uint32_t id = (uint32_t)((c[2] * gr.dim[1] + c[1]) * gr.dim[0] + c[0]);
    g.cell_of[i] = id;
    g.rank_in[i] = atomicAdd(&g.count[id], 1u);
}
// exclusive scan of count[0, ncells) (sg_scan.h): start[id] + bsum[id >> 10] is the first sorted slot of cell id
__global__ void __launch_bounds__(256)
sg_cells_scan1_2_kernel(SgKnnGrids L)
{
    const SgKnnGrid &g = L.l[blockIdx.y];
    sg_scan_block(g.grid->ncells, [&](int i) { return g.count[i]; }, g.start, g.bsum);
}
__global__ void __launch_bounds__(1024)
sg_cells_scan2_2_kernel(SgKnnGrids L)
{
    const SgKnnGrid &g = L.l[blockIdx.y];
    sg_scan_block_sums(g.grid->ncells, g.bsum);
}
__global__ void __launch_bounds__(256)
sg_cell_scatter2_kernel(int N, const float *__restrict__ xyz, SgKnnGrids L)
{
    const SgKnnGrid &g = L.l[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t id = g.cell_of[i];
    const uint32_t slot = g.start[id] + g.bsum[id >> 10] + g.rank_in[i];
    g.sorted[slot] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float((uint32_t)i));
}
// cells[id] = (first sorted slot, count): one 8-B load per visited cell in the query
__global__ void __launch_bounds__(256)
sg_cells_finalize2_kernel(SgKnnGrids L)
{
    const SgKnnGrid &g = L.l[blockIdx.y];
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < g.grid->ncells) g.cells[id] = make_uint2(g.start[id] + g.bsum[id >> 10], g.count[id]);
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
struct SgKnnWs { float *bpart, *partial, *medge; SgKnnGrids g; /* l[0] coarse, l[1] fine */ };
static SgKnnWs sg_knn_ws_at(int N, void *ws)
{
    const size_t n = N;
    SgKnnWs w;
    char *b = (char *)ws;
    w.bpart = (float *)b; b += sg_align((size_t)sg_nb(N) * 32);
    w.partial = (float *)b; b += sg_align((size_t)sg_nb(N) * SG_RED_MAXQ * 4);
    w.medge = (float *)b; b += sg_align(n * 4);
    sg_knn_grid_at(N, sg_knn_max_cells(N), b, &w.g.l[0]);
    sg_knn_grid_at(N, sg_knn_max_cells_fine(N), b, &w.g.l[1]);
    return w;
}

// first half: the two grids over the cloud (eight small launches, both levels per launch: bounding box partials -> both grids ->
// counting sort of the points by cell); second half: the query + the loss.  One call does both (sg_gaussian_edge_loss); a caller
// that wants the latency-bound grid builds early and the GPU-filling query later -- beside kernels with idle issue slots instead
// of beside a chain of small ones -- makes the two calls itself on the same workspace.
void sg_launch_knn_prepare(int N, const float *xyz, void *ws, hipStream_t st)
{
    const SgKnnWs w = sg_knn_ws_at(N, ws);
    const SgKnnGrids &L = w.g;
    const size_t mcmax = L.l[0].mc > L.l[1].mc ? L.l[0].mc : L.l[1].mc;
    const int nb = sg_nb(N), ncb = (int)((mcmax + 1023) / 1024);
    hipLaunchKernelGGL(sg_bbox_partial_kernel, dim3(nb), dim3(256), 0, st, N, xyz, w.bpart);
    hipLaunchKernelGGL(sg_grid_setup2_kernel, dim3(1, 2), dim3(256), 0, st, w.bpart, nb, N, L);
    hipLaunchKernelGGL(sg_zero2_kernel, dim3(1024, 2), dim3(256), 0, st, L);
    hipLaunchKernelGGL(sg_cell_count2_kernel, dim3(nb, 2), dim3(256), 0, st, N, xyz, L);
    hipLaunchKernelGGL(sg_cells_scan1_2_kernel, dim3(ncb, 2), dim3(256), 0, st, L);
    hipLaunchKernelGGL(sg_cells_scan2_2_kernel, dim3(1, 2), dim3(1024), 0, st, L);
    hipLaunchKernelGGL(sg_cell_scatter2_kernel, dim3(nb, 2), dim3(256), 0, st, N, xyz, L);
    hipLaunchKernelGGL(sg_cells_finalize2_kernel, dim3((unsigned)((mcmax + 255) / 256), 2), dim3(256), 0, st, L);
}

// the query for one K; sg_knn_query_for is the one place that says which K exist (NULL for any other)
typedef void (*SgKnnQueryFn)(int N, const SgKnnGrids &g, float *medge, hipStream_t st);
template <int K>
static void sg_knn_query_launch(int N, const SgKnnGrids &g, float *medge, hipStream_t st)
{
    const SgKnnGrid &gc = g.l[0], &gf = g.l[1];
    const int nbq = (int)(((size_t)N * SG_KNN_SUB + 255) / 256);
    hipLaunchKernelGGL(sg_knn_query_kernel<K>, dim3(nbq), dim3(256), 0, st, N, gc.sorted, gc.grid, gc.cells, gf.sorted, gf.grid, gf.cells, medge);
}
static SgKnnQueryFn sg_knn_query_for(int K)
{
    switch (K) {
    case 5: return sg_knn_query_launch<5>;
    case 9: return sg_knn_query_launch<9>;
    case 17: return sg_knn_query_launch<17>;
    default: return nullptr;
    }
}
// the second half with the query already chosen
static void sg_knn_finish(int N, SgKnnQueryFn query, const float *scales, void *ws, float *mean_edge_out, float *loss,
                          const float *upstream, float *d_scales, hipStream_t st)
{
    const SgKnnWs w = sg_knn_ws_at(N, ws);
    float *medge = mean_edge_out ? mean_edge_out : w.medge;
    const int nb = sg_nb(N);
    query(N, w.g, medge, st);
    if (scales && (loss || d_scales)) {
        hipLaunchKernelGGL(sg_edge_loss_kernel, dim3(nb), dim3(256), 0, st, N, scales, medge, upstream, d_scales, w.partial);
        if (loss) sg_launch_scalar_reduce(w.partial, nb, 1.0f / (float)N, loss, st);
    }
}
// (both return 1 for a K without a query, before anything is launched)
int sg_launch_knn_finish(int N, int K, const float *scales, void *ws, float *mean_edge_out, float *loss, const float *upstream,
                         float *d_scales, hipStream_t st)
{
    const SgKnnQueryFn query = sg_knn_query_for(K);
    if (!query) return 1;
    sg_knn_finish(N, query, scales, ws, mean_edge_out, loss, upstream, d_scales, st);
    return 0;
}
int sg_launch_knn_edge(int N, int K, const float *xyz, const float *scales, void *ws, float *mean_edge_out, float *loss,
                       const float *upstream, float *d_scales, hipStream_t st)
{
    const SgKnnQueryFn query = sg_knn_query_for(K);
    if (!query) return 1;
    sg_launch_knn_prepare(N, xyz, ws, st);
    sg_knn_finish(N, query, scales, ws, mean_edge_out, loss, upstream, d_scales, st);
    return 0;
}
