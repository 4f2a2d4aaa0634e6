// Mesh terms of the training step (include/sings_mesh_terms.h): the region Laplacian of the anchor positions, the region Laplacian of
// the DC colours and the hand Laplacian (loss_items.py:93-192 as gs_trainer.py:366-399 calls them) in ONE forward and ONE backward
// launch over one CSR, and that CSR -- with its degrees, label counts and per-vertex scales -- built on the device.
#include "sg_host.h"
#include "sg_reduce.h"
#include "sg_scan.h"
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
    const int incl = sg_wave_incl_scan(s, lane);
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
