// The soft silhouette of a posed triangle mesh and its backward (include/sings_silhouette.h): the device path of the pose refinement,
// held to `silhouette_host` of sings_amd/pose_refine.py.
//
//   setup      a thread per (frame, face): project the three corners, decide validity as the definition does, grow the screen bounding
//              box by the band radius sqrt(LOGIT sigma) / s pixels, count the face into the 16 x 16 tiles the box meets
//   binning    the exclusive scan of sg_scan.h over the tile counts; a thread per (frame, face) takes a slot in each of its tiles by an
//              INTEGER atomic (which slot is a matter of scheduling); then a workgroup per tile brings its list into ascending face
//              index -- an all-ascending bitonic network, in LDS up to SG_SIL_SORT_LDS entries and in place in global memory beyond,
//              n log^2 n at any length -- so nothing downstream depends on scheduling
//   composite  a workgroup per tile, a pixel per lane; the list goes through LDS SG_SIL_CHUNK faces at a time, any length
//   backward   the same traversal with dL/dx_f = -dL/dalpha Q prob_f: no product over the other faces, no division.  The six screen
//              sums of a pair are reduced over the wave (DPP within a row of 16, two swaps across the rows), over the four waves through
//              LDS in wave order, and written as ONE partial per (tile, face) pair.  A thread per face then adds its pairs in tile
//              order (it finds itself in a sorted list by bisection), a thread per vertex its corners in CSR order, and applies the
//              projection's chain rule
//
// No floating-point atomics, no waiting between workgroups; every loop runs to a count read before it; every __syncthreads() is
// reached by the whole workgroup.  A pair beyond the capacity is dropped (the index is tested before every write) and info[0] says so.
#include "sg_host.h"
#include "sg_scan.h"
#include "sg_sil_pair.h"
#include "../../include/sings_silhouette.h"

#define SIL_ZNEAR 1e-3f
#define SIL_MIN_AREA 1e-8f
static_assert(SG_SIL_TILE * SG_SIL_TILE == 256 && SG_SIL_CHUNK == 256, "a workgroup stages one face per thread and owns one pixel per thread");

struct SilDims {
    int K, V, F, H, W, gx, gy, T;
    uint32_t cap;
    float fx, fy, cx, cy, rad_px;
    SgSilScalars c;
};
struct SilWs {
    int32_t *info; float *rec; int32_t *rect; uint32_t *tile_count, *tile_start, *bsum, *cursor; float *Q, *face_grad;
    uint32_t *list; float *partial;
};

// where tile i's list starts, and how much of it lies within the capacity
__device__ __forceinline__ uint32_t sil_start(const SilWs &w, int i) { return w.tile_start[i] + w.bsum[i >> 10]; }
__device__ __forceinline__ uint32_t sil_length(const SilWs &w, int i, uint32_t start, uint32_t cap)
{
    const uint32_t n = w.tile_count[i], room = start < cap ? cap - start : 0u;
    return n < room ? n : room;
}

// ---- setup ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sg_sil_setup_kernel(SilDims d, const float *__restrict__ verts, const int32_t *__restrict__ faces, SilWs w)
{
    const int f = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (f >= d.F) return;
    const size_t kf = (size_t)k * d.F + f;
    int idx[3];
    float u[3] = {0.0f, 1.0f, 0.0f}, v[3] = {0.0f, 0.0f, 1.0f};
    bool valid = true;
#pragma unroll
    for (int c = 0; c < 3; c++) { idx[c] = faces[3 * f + c]; valid = valid && (unsigned)idx[c] < (unsigned)d.V; }
    if (valid) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float *p = verts + ((size_t)k * d.V + idx[c]) * 3;
            const float x = p[0], y = p[1], z = p[2];
            valid = valid && isfinite(x) && isfinite(y) && isfinite(z) && z > SIL_ZNEAR;
            u[c] = d.fx * x / z + d.cx;
            v[c] = d.fy * y / z + d.cy;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) valid = valid && isfinite(u[c]) && isfinite(v[c]);
        const float e1x = u[1] - u[0], e1y = v[1] - v[0], e2x = u[2] - u[0], e2y = v[2] - v[0];
        valid = valid && fabsf(e1x * e2y - e1y * e2x) * d.c.s2 > SIL_MIN_AREA;
    }
    int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
    if (valid) {
        // tiles [floor((min - rad) / 16), floor((max + rad) / 16)], clamped as floats first: a coordinate may be anything finite
        const float ulo = fminf(u[0], fminf(u[1], u[2])) - d.rad_px, uhi = fmaxf(u[0], fmaxf(u[1], u[2])) + d.rad_px;
        const float vlo = fminf(v[0], fminf(v[1], v[2])) - d.rad_px, vhi = fmaxf(v[0], fmaxf(v[1], v[2])) + d.rad_px;
        x0 = max((int)floorf(fminf(fmaxf(ulo * 0.0625f, -1.0f), (float)d.gx)), 0);
        x1 = min((int)floorf(fminf(fmaxf(uhi * 0.0625f, -1.0f), (float)d.gx)), d.gx - 1);
        y0 = max((int)floorf(fminf(fmaxf(vlo * 0.0625f, -1.0f), (float)d.gy)), 0);
        y1 = min((int)floorf(fminf(fmaxf(vhi * 0.0625f, -1.0f), (float)d.gy)), d.gy - 1);
        if (x1 < x0 || y1 < y0) { x0 = 0; y0 = 0; x1 = -1; y1 = -1; }
    }
    float4 *rec = (float4 *)w.rec + kf * 2;
    rec[0] = make_float4(u[0], v[0], u[1], v[1]);
    rec[1] = make_float4(u[2], v[2], 0.0f, 0.0f);
    ((int4 *)w.rect)[kf] = make_int4(x0, y0, x1, y1);
    uint32_t *count = w.tile_count + (size_t)k * d.T;
    for (int ty = y0; ty <= y1; ty++)
        for (int tx = x0; tx <= x1; tx++) atomicAdd(count + ty * d.gx + tx, 1u);
}

// ---- binning -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sg_sil_scan_kernel(int n, const uint32_t *__restrict__ count, uint32_t *__restrict__ out, uint32_t *__restrict__ bsum)
{
    sg_scan_block(n, [&](int i) { return count[i]; }, out, bsum);
}

__global__ void __launch_bounds__(1024)
sg_sil_scan_sums_kernel(SilDims d, SilWs w)
{
    const uint32_t total = sg_scan_block_sums(d.K * d.T, w.bsum);
    if ((int)threadIdx.x < d.K) {
        const int k = threadIdx.x;
        const uint32_t lo = sil_start(w, k * d.T), hi = k + 1 < d.K ? sil_start(w, (k + 1) * d.T) : total;
        w.info[SG_SIL_INFO_WORDS + k] = (int32_t)(hi - lo);
    }
    if (threadIdx.x == 0) {
        // [0], [1]: this launch; [2], [3]: over every launch since the owner of the workspace last zeroed them
        w.info[0] = total > d.cap ? 1 : 0; w.info[1] = (int32_t)total;
        if (total > d.cap) w.info[2] = 1;
        if ((int32_t)total > w.info[3]) w.info[3] = (int32_t)total;
    }
}

__global__ void __launch_bounds__(256)
sg_sil_fill_kernel(SilDims d, SilWs w)
{
    const int f = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (f >= d.F) return;
    const int4 r = ((const int4 *)w.rect)[(size_t)k * d.F + f];
    for (int ty = r.y; ty <= r.w; ty++)
        for (int tx = r.x; tx <= r.z; tx++) {
            const int i = k * d.T + ty * d.gx + tx;
            const uint64_t at = (uint64_t)sil_start(w, i) + atomicAdd(w.cursor + i, 1u);
            if (at < d.cap) w.list[at] = (uint32_t)f;
        }
}

// a[0, n) ascending, by the whole workgroup: the bitonic network with every comparator pointing up, so that a list of any length sorts as
// if padded with +inf (an entry beyond n would never move: its comparators are left out)
template <typename P>
__device__ __forceinline__ void sil_sort_network(P a, int n, int tid)
{
    for (int k = 2; (k >> 1) < n; k <<= 1) {
        for (int i = tid; i < n; i += 256) {
            const int l = i ^ (k - 1);
            if (l > i && l < n) { const uint32_t p = a[i], q = a[l]; if (p > q) { a[i] = q; a[l] = p; } }
        }
        __syncthreads();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int i = tid; i < n; i += 256) {
                const int l = i ^ j;
                if (l > i && l < n) { const uint32_t p = a[i], q = a[l]; if (p > q) { a[i] = q; a[l] = p; } }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256)
sg_sil_sort_kernel(SilDims d, SilWs w)
{
    __shared__ uint32_t s[SG_SIL_SORT_LDS];
    const int i = blockIdx.y * d.T + blockIdx.x, tid = threadIdx.x;
    const uint32_t start = sil_start(w, i);
    const int n = (int)sil_length(w, i, start, d.cap);
    if (n < 2) return;                                               // (uniform: the whole workgroup)
    uint32_t *g = w.list + start;
    if (n <= SG_SIL_SORT_LDS) {
        for (int e = tid; e < n; e += 256) s[e] = g[e];
        __syncthreads();
        sil_sort_network(s, n, tid);
        for (int e = tid; e < n; e += 256) g[e] = s[e];
    } else
        sil_sort_network(g, n, tid);
}

// ---- the composites ------------------------------------------------------------------------------------------------------------------
// a tile's faces [base, base + m) into LDS, a thread each; barriers before (the previous chunk is read out) and after
__device__ __forceinline__ void sil_stage(const SilDims &d, const SilWs &w, int k, uint32_t at, int m, float4 *sRec, int tid)
{
    __syncthreads();
    if (tid < m) {
        const uint32_t f = min(w.list[at + tid], (uint32_t)(d.F - 1));
        const float4 *rec = (const float4 *)w.rec + ((size_t)k * d.F + f) * 2;
        sRec[2 * tid] = rec[0];
        sRec[2 * tid + 1] = rec[1];
    }
    __syncthreads();
}

template <bool COUNT>
__global__ void __launch_bounds__(256)
sg_sil_forward_kernel(SilDims d, SilWs w, float *__restrict__ alpha, int32_t *__restrict__ counts)
{
    __shared__ float4 sRec[2 * SG_SIL_CHUNK];
    __shared__ int sMax[4];
    const int tid = threadIdx.x, k = blockIdx.z, i = k * d.T + blockIdx.y * d.gx + blockIdx.x;
    const int ix = blockIdx.x * SG_SIL_TILE + (tid & 15), iy = blockIdx.y * SG_SIL_TILE + (tid >> 4);
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const bool in_image = ix < d.W && iy < d.H;
    const uint32_t start = sil_start(w, i);
    const int n = (int)sil_length(w, i, start, d.cap);
    float Q = 1.0f;
    int cnt = 0;
    bool done = false;                                               // this wave's Q is 0.0f on every lane: nothing can change it
    for (int base = 0; base < n; base += SG_SIL_CHUNK) {
        const int m = min(SG_SIL_CHUNK, n - base);
        sil_stage(d, w, k, start + base, m, sRec, tid);
        if (COUNT || !done) {
            for (int j = 0; j < m; j++) {
                const SgSilPair p = sg_sil_pair(px, py, sRec[2 * j], sRec[2 * j + 1], d.c);
                if (p.on) { Q *= 1.0f - sg_sil_prob(p.x); cnt++; }
            }
            if (!COUNT) done = __ballot(Q != 0.0f) == 0ull;
        }
    }
    if (in_image) {
        const size_t at = ((size_t)k * d.H + iy) * d.W + ix;
        alpha[at] = 1.0f - Q;
        w.Q[at] = Q;
    }
    if (COUNT) {
        int c = in_image ? cnt : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c = max(c, __shfl_xor(c, o, 64));
        if ((tid & 63) == 0) sMax[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) atomicMax(counts + k, max(max(sMax[0], sMax[1]), max(sMax[2], sMax[3])));     // (an integer maximum has no order)
    }
}

#define SIL_DPP(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false))
// the sum of v over the 64 lanes, to every lane, in a fixed tree: within a row of 16 by DPP, then across the four rows
__device__ __forceinline__ float sil_wave_sum(float v)
{
    v += SIL_DPP(v, 0xB1);                       // quad_perm [1,0,3,2]
    v += SIL_DPP(v, 0x4E);                       // quad_perm [2,3,0,1]
    v += SIL_DPP(v, 0x141);                      // row_half_mirror
    v += SIL_DPP(v, 0x140);                      // row_mirror
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__global__ void __launch_bounds__(256)
sg_sil_backward_kernel(SilDims d, SilWs w, const float *__restrict__ dalpha)
{
    __shared__ float4 sRec[2 * SG_SIL_CHUNK];
    __shared__ float sPart[4][SG_SIL_CHUNK * 6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = blockIdx.z, i = k * d.T + blockIdx.y * d.gx + blockIdx.x;
    const int ix = blockIdx.x * SG_SIL_TILE + (tid & 15), iy = blockIdx.y * SG_SIL_TILE + (tid >> 4);
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const uint32_t start = sil_start(w, i);
    const int n = (int)sil_length(w, i, start, d.cap);
    float gQ = 0.0f;                                                 // dL/dx_f = gQ prob_f
    if (ix < d.W && iy < d.H) {
        const size_t at = ((size_t)k * d.H + iy) * d.W + ix;
        gQ = -(dalpha[at] * w.Q[at]);
    }
    const bool wave_live = __ballot(gQ != 0.0f) != 0ull;
    const float scale = -2.0f * (d.c.s2 / d.c.sigma);               // d x / d (pixel distance^2) = sign s^2 / sigma; d d2 = -2 (...) below
    for (int base = 0; base < n; base += SG_SIL_CHUNK) {
        const int m = min(SG_SIL_CHUNK, n - base);
        sil_stage(d, w, k, start + base, m, sRec, tid);
        if (!wave_live) {
            for (int e = lane; e < m * 6; e += 64) sPart[wave][e] = 0.0f;
        } else {
            for (int j = 0; j < m; j++) {
                const SgSilPair p = sg_sil_pair(px, py, sRec[2 * j], sRec[2 * j + 1], d.c);
                const bool act = p.on && gQ != 0.0f;
                if (__ballot(act) == 0ull) {                         // (wave-uniform)
                    if (lane < 6) sPart[wave][j * 6 + lane] = 0.0f;
                    continue;
                }
                // d2 = |pixel - a - t (b - a)|^2 with t clamped: d d2 / d a = -2 (1 - t) (dx, dy), d d2 / d b = -2 t (dx, dy)
                const float g = act ? gQ * sg_sil_prob(p.x) * p.sign * scale : 0.0f;
                const float ga = g * (1.0f - p.t), gb = g * p.t;
                const float ax = ga * p.dx, ay = ga * p.dy, bx = gb * p.dx, by = gb * p.dy;
                float s[6];
                s[0] = p.edge == 0 ? ax : p.edge == 2 ? bx : 0.0f;  s[1] = p.edge == 0 ? ay : p.edge == 2 ? by : 0.0f;
                s[2] = p.edge == 1 ? ax : p.edge == 0 ? bx : 0.0f;  s[3] = p.edge == 1 ? ay : p.edge == 0 ? by : 0.0f;
                s[4] = p.edge == 2 ? ax : p.edge == 1 ? bx : 0.0f;  s[5] = p.edge == 2 ? ay : p.edge == 1 ? by : 0.0f;
#pragma unroll
                for (int q = 0; q < 6; q++) s[q] = sil_wave_sum(s[q]);
                const float mine = lane == 0 ? s[0] : lane == 1 ? s[1] : lane == 2 ? s[2] : lane == 3 ? s[3] : lane == 4 ? s[4] : s[5];
                if (lane < 6) sPart[wave][j * 6 + lane] = mine;
            }
        }
        __syncthreads();
        float *out = w.partial + (size_t)(start + base) * 6;        // (start + base + m <= capacity)
        for (int e = tid; e < m * 6; e += 256) out[e] = ((sPart[0][e] + sPart[1][e]) + sPart[2][e]) + sPart[3][e];
    }
}

// a thread per (frame, face): its pairs in tile order (row-major over its rectangle); it finds itself in a tile's ascending list by
// bisection.  A face without a tile, or whose pair was dropped, adds nothing: face_grad is written for every face.
__global__ void __launch_bounds__(256)
sg_sil_face_gather_kernel(SilDims d, SilWs w)
{
    const int f = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (f >= d.F) return;
    const size_t kf = (size_t)k * d.F + f;
    const int4 r = ((const int4 *)w.rect)[kf];
    float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int ty = r.y; ty <= r.w; ty++)
        for (int tx = r.x; tx <= r.z; tx++) {
            const int i = k * d.T + ty * d.gx + tx;
            const uint32_t start = sil_start(w, i);
            const uint32_t n = sil_length(w, i, start, d.cap);
            uint32_t lo = 0, hi = n;
            for (int step = 0; step < 32 && lo < hi; step++) {       // the first entry >= f
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (w.list[start + mid] < (uint32_t)f) lo = mid + 1; else hi = mid;
            }
            if (lo < n && w.list[start + lo] == (uint32_t)f) {
                const float *p = w.partial + (size_t)(start + lo) * 6;
#pragma unroll
                for (int q = 0; q < 6; q++) s[q] += p[q];
            }
        }
#pragma unroll
    for (int q = 0; q < 6; q++) w.face_grad[kf * 6 + q] = s[q];
}

// a thread per (frame, vertex): its corners in CSR order, then u = fx x / z + cx, v = fy y / z + cy
__global__ void __launch_bounds__(256)
sg_sil_vertex_gather_kernel(SilDims d, SilWs w, const float *__restrict__ verts, const int32_t *__restrict__ row_ptr,
                            const int32_t *__restrict__ corner, float *__restrict__ dverts)
{
    const int vi = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (vi >= d.V) return;
    const int e0 = row_ptr[vi], e1 = row_ptr[vi + 1];
    float gu = 0.0f, gv = 0.0f;
    for (int e = e0; e < e1; e++) {
        const int fc = corner[e];
        if ((unsigned)fc >= (unsigned)(3 * d.F)) continue;
        const float *p = w.face_grad + ((size_t)k * d.F + fc / 3) * 6 + 2 * (fc % 3);
        gu += p[0]; gv += p[1];
    }
    const size_t at = ((size_t)k * d.V + vi) * 3;
    const float x = verts[at], y = verts[at + 1], z = verts[at + 2];
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (isfinite(x) && isfinite(y) && isfinite(z) && z > SIL_ZNEAR && (gu != 0.0f || gv != 0.0f)) {
        gx = gu * d.fx / z;
        gy = gv * d.fy / z;
        gz = -(gu * (d.fx * x) + gv * (d.fy * y)) / (z * z);
    }
    dverts[at] = gx; dverts[at + 1] = gy; dverts[at + 2] = gz;
}

// ---- the update launch of the pose refinement ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
sg_sil_pose_update_kernel(int K, float lr, float *__restrict__ pose, const float *__restrict__ grad, float *__restrict__ m,
                          float *__restrict__ v, const float *__restrict__ grad_mask, const float *__restrict__ lo,
                          const float *__restrict__ hi, int32_t *step, const float *__restrict__ terms, float *__restrict__ table,
                          int max_iterations)
{
    const int it = step[0] + 1;
    const float b1 = 0.9f, b2 = 0.999f, c1 = 0.1f, c2 = 0.001f;      // (1 - 0.9 and 1 - 0.999 of fp64, rounded to fp32 as torch rounds them)
    const float step_size = (float)((double)lr / (1.0 - pow(0.9, (double)it)));
    const float root2 = (float)sqrt(1.0 - pow(0.999, (double)it));
    for (int e = threadIdx.x; e < K * SG_SIL_POSE; e += 256) {
        const int c = e % SG_SIL_POSE;
        const float p = pose[e];
        const float g = grad[e] * (grad_mask[c] * ((p < hi[c] && p > lo[c]) ? 1.0f : 0.0f));
        const float mm = b1 * m[e] + c1 * g;
        const float vv = b2 * v[e] + c2 * g * g;
        m[e] = mm; v[e] = vv;
        pose[e] = p - step_size * mm / (sqrtf(vv) / root2 + 1e-8f);
    }
    if (terms && it <= max_iterations)
        for (int e = threadIdx.x; e < K * 2; e += 256) table[(size_t)(it - 1) * K * 2 + e] = terms[e];
    __syncthreads();                                                 // (every thread has read step[0])
    if (threadIdx.x == 0) step[0] = it;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int sil_layout(const char *who, int K, int V, int F, int H, int W, size_t capacity, size_t *L)
{
    if (K < 1 || K > SG_SIL_MAX_FRAMES) return sg_failf("%s: K = %d outside 1..%d", who, K, SG_SIL_MAX_FRAMES);
    if (V < 1 || F < 1 || H < 1 || W < 1) return sg_failf("%s: V = %d, F = %d, H = %d, W = %d must be positive", who, V, F, H, W);
    if (capacity < 1) return sg_failf("%s: capacity 0", who);
    if (!L) return sg_failf("%s: null pointer", who);
    const long long lim = 2147483647LL, gx = (W + 15) / 16, gy = (H + 15) / 16, KT = (long long)K * gx * gy;
    if ((long long)K * H * W > lim || 8LL * K * F > lim || 3LL * K * V > lim || KT + 1024 > lim ||
        capacity > (size_t)((lim - SG_SIL_GUARD_WORDS) / 6))
        return sg_failf("%s: K = %d, V = %d, F = %d, %d x %d, capacity %zu: an offset does not fit int32", who, K, V, F, W, H, capacity);
    const size_t words[SG_SIL_L_BYTES] = {
        (size_t)SG_SIL_INFO_WORDS + (size_t)K, 8 * (size_t)K * F, 4 * (size_t)K * F, (size_t)KT, (size_t)KT + (size_t)(KT + 1023) / 1024,
        (size_t)KT, (size_t)K * H * W, 6 * (size_t)K * F, capacity + SG_SIL_GUARD_WORDS, 6 * capacity + SG_SIL_GUARD_WORDS};
    size_t at = 0;
    for (int p = 0; p < SG_SIL_L_BYTES; p++) { L[p] = at; at += (words[p] * 4 + 255) / 256 * 256; }
    L[SG_SIL_L_BYTES] = at;
    return 0;
}

extern "C" int sg_sil_layout(int K, int V, int F, int H, int W, size_t capacity, size_t *layout)
{
    return sil_layout("sg_sil_layout", K, V, F, H, W, capacity, layout);
}

static int sil_prepare(const char *who, int K, int V, int F, int H, int W, float fx, float fy, float cx, float cy, float sigma,
                       size_t capacity, void *ws, SilDims *d, SilWs *w)
{
    size_t L[SG_SIL_LAYOUT_WORDS];
    if (sil_layout(who, K, V, F, H, W, capacity, L)) return 1;
    if (!(sigma > 0.0f) || !isfinite(sigma) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy))
        return sg_failf("%s: sigma = %g must be positive and the intrinsics finite", who, (double)sigma);
    if (!ws || ((uintptr_t)ws & 15)) return sg_failf("%s: the workspace is null or not 16-byte aligned", who);
    const double logit = log(1.0 / 1e-4 - 1.0);
    const float s = 2.0f / (float)(H < W ? H : W);
    d->K = K; d->V = V; d->F = F; d->H = H; d->W = W; d->gx = (W + 15) / 16; d->gy = (H + 15) / 16; d->T = d->gx * d->gy;
    d->cap = (uint32_t)capacity;
    d->fx = fx; d->fy = fy; d->cx = cx; d->cy = cy;
    d->rad_px = (float)(sqrt(logit * (double)sigma) / (2.0 / (double)(H < W ? H : W)));
    d->c.s2 = s * s; d->c.r = (float)logit * sigma; d->c.sigma = sigma;
    char *b = (char *)ws;
    w->info = (int32_t *)(b + L[SG_SIL_L_INFO]); w->rec = (float *)(b + L[SG_SIL_L_REC]); w->rect = (int32_t *)(b + L[SG_SIL_L_RECT]);
    w->tile_count = (uint32_t *)(b + L[SG_SIL_L_TILE_COUNT]); w->tile_start = (uint32_t *)(b + L[SG_SIL_L_TILE_START]);
    w->bsum = w->tile_start + (size_t)K * d->T; w->cursor = (uint32_t *)(b + L[SG_SIL_L_CURSOR]);
    w->Q = (float *)(b + L[SG_SIL_L_Q]); w->face_grad = (float *)(b + L[SG_SIL_L_FACE_GRAD]);
    w->list = (uint32_t *)(b + L[SG_SIL_L_LIST]); w->partial = (float *)(b + L[SG_SIL_L_PARTIAL]);
    return 0;
}

extern "C" int sg_sil_forward(int K, int V, int F, int H, int W, float fx, float fy, float cx, float cy, float sigma, size_t capacity,
                              const float *verts, const int32_t *faces, void *ws, float *alpha, int32_t *counts, void *stream)
{
    SilDims d; SilWs w;
    if (sil_prepare("sg_sil_forward", K, V, F, H, W, fx, fy, cx, cy, sigma, capacity, ws, &d, &w)) return 1;
    if (!verts || !faces || !alpha) return sg_failf("sg_sil_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int KT = K * d.T;
    const dim3 per_face((F + 255) / 256, K), per_tile(d.gx, d.gy, K);
    // tile_count, tile_start + block sums and cursor lie one behind the other
    hipError_t e = hipMemsetAsync(w.tile_count, 0, (size_t)((char *)w.Q - (char *)w.tile_count), st);
    if (e == hipSuccess && counts) e = hipMemsetAsync(counts, 0, sizeof(int32_t) * K, st);
    if (e != hipSuccess) return sg_set_error("sg_sil_forward: memset", e);
    hipLaunchKernelGGL(sg_sil_setup_kernel, per_face, dim3(256), 0, st, d, verts, faces, w);
    hipLaunchKernelGGL(sg_sil_scan_kernel, dim3((KT + 1023) / 1024), dim3(256), 0, st, KT, w.tile_count, w.tile_start, w.bsum);
    hipLaunchKernelGGL(sg_sil_scan_sums_kernel, dim3(1), dim3(1024), 0, st, d, w);
    hipLaunchKernelGGL(sg_sil_fill_kernel, per_face, dim3(256), 0, st, d, w);
    hipLaunchKernelGGL(sg_sil_sort_kernel, dim3(d.T, K), dim3(256), 0, st, d, w);
    if (counts) hipLaunchKernelGGL(sg_sil_forward_kernel<true>, per_tile, dim3(256), 0, st, d, w, alpha, counts);
    else hipLaunchKernelGGL(sg_sil_forward_kernel<false>, per_tile, dim3(256), 0, st, d, w, alpha, counts);
    return sg_launched("sg_sil_forward");
}

extern "C" int sg_sil_backward(int K, int V, int F, int H, int W, float fx, float fy, float cx, float cy, float sigma, size_t capacity,
                               const float *verts, const int32_t *faces, void *ws, const float *dalpha, const int32_t *row_ptr,
                               const int32_t *corner, float *dverts, void *stream)
{
    SilDims d; SilWs w;
    if (sil_prepare("sg_sil_backward", K, V, F, H, W, fx, fy, cx, cy, sigma, capacity, ws, &d, &w)) return 1;
    if (!verts || !faces || !dalpha || !row_ptr || !corner || !dverts) return sg_failf("sg_sil_backward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_sil_backward_kernel, dim3(d.gx, d.gy, K), dim3(256), 0, st, d, w, dalpha);
    hipLaunchKernelGGL(sg_sil_face_gather_kernel, dim3((F + 255) / 256, K), dim3(256), 0, st, d, w);
    hipLaunchKernelGGL(sg_sil_vertex_gather_kernel, dim3((V + 255) / 256, K), dim3(256), 0, st, d, w, verts, row_ptr, corner, dverts);
    return sg_launched("sg_sil_backward");
}

extern "C" int sg_sil_pose_update(int K, float lr, float *pose, const float *grad, float *m, float *v, const float *grad_mask,
                                  const float *lo, const float *hi, int32_t *step, const float *terms, float *table, int max_iterations,
                                  void *stream)
{
    if (K < 1 || K > SG_SIL_MAX_FRAMES) return sg_failf("sg_sil_pose_update: K = %d outside 1..%d", K, SG_SIL_MAX_FRAMES);
    if (!pose || !grad || !m || !v || !grad_mask || !lo || !hi || !step) return sg_failf("sg_sil_pose_update: null pointer");
    if ((terms == nullptr) != (table == nullptr)) return sg_failf("sg_sil_pose_update: terms and table come together");
    if (terms && max_iterations < 1) return sg_failf("sg_sil_pose_update: a table of %d iterations", max_iterations);
    hipLaunchKernelGGL(sg_sil_pose_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, K, lr, pose, grad, m, v, grad_mask, lo, hi,
                       step, terms, table, max_iterations);
    return sg_launched("sg_sil_pose_update");
}
