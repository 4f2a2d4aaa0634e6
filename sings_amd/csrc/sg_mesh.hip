// Mesh topology on the device for the reference's `hybrid` densification (sings_hybrid.py:1022-1150, geometry_ops.py:8-76): the
// unique undirected edges of a (flagged) face set in lexicographic order -- the order of `torch.unique(sorted_edges, dim=0)`, so a
// midpoint's index is the reference's --, the selective 1-to-4 subdivision, and the midpoint rows of per-vertex attributes.  Further
// down, for its pruning (sings_hybrid.py:1153-1257, geometry_ops.py:79-167): the sequential edge collapse as one launch, the face filter.
//
// Not a throughput kernel: at SMPL scale (110 k vertices, 220 k faces) every array is a few MB and the cost is the launches and ONE
// host read of (E, flagged faces).  What matters is that the output is a pure function of the input:
//
//   directed instances  every flagged face contributes its three edges as (a = min, b = max); an instance lives in the ROW of a.
//                       count[a] (integer atomics: a sum of ones has no order), exclusive scan -> row starts (the three-step scan
//                       of sg_scan.h, as the k-NN cells), then every instance takes a slot of its row with a returning atomic.  WHICH slot
//                       depends on arrival order; nothing that leaves this file does:
//   rank by counting    an instance's place among the unique edges is computed from the row's CONTENTS, not from its slots: it
//                       is a head if no instance at a smaller slot of the row holds the same b, its multiplicity is the number of
//                       instances with its b, and the rank of its edge is the number of heads with a smaller b.  All three are
//                       counts over a multiset, the same for every permutation of the row.  One lane per instance walks its row
//                       (6 entries on average, L2-resident): a row of ANY length takes the same path -- a hub of valence n costs
//                       O(n^2) loads, 25 k for the pole of an 80-column UV sphere, and there is no length at which another kernel
//                       takes over.
//   unique counts       heads per row (integer atomics again), scanned -> the first edge of every row; edge (a, b) = that + rank.
//
// The host reads info[] once between sg_mesh_edges_build and sg_mesh_edges_emit: E sizes the outputs.
#include "sg_host.h"
#include "sg_scan.h"

#define SG_MESH_THREADS 256
#define SG_MESH_MAX_V (1 << 30)                  // the scan's block table and the 32-bit row offsets cover this many vertices
#define SG_MESH_MAX_F 715827882                  // 3 F < 2^31: an instance index is an int

// ---- exclusive scan of n uint32 (or of n flags), the three steps of sg_scan.h: prefix(i) = out[i] + bsum[i >> 10].  Two independent
// jobs per launch (blockIdx.y).
struct SgScanJob {
    const uint32_t *in;         // values, or NULL:
    const uint8_t *in8;         // flags (!= 0 counts 1), or NULL as well: every entry counts 1
    uint32_t *out, *bsum;
    int32_t *total;             // the sum of all n entries
    int n;
};
struct SgScanJobs { SgScanJob j[2]; };

__device__ __forceinline__ uint32_t sg_scan_value(const SgScanJob &J, int i)
{
    return J.in ? J.in[i] : (J.in8 ? (J.in8[i] != 0 ? 1u : 0u) : 1u);
}
__global__ void __launch_bounds__(256)
sg_mesh_scan1_kernel(SgScanJobs JJ)
{
    const SgScanJob &J = JJ.j[blockIdx.y];
    sg_scan_block(J.n, [&](int i) { return sg_scan_value(J, i); }, J.out, J.bsum);
}
__global__ void __launch_bounds__(1024)
sg_mesh_scan2_kernel(SgScanJobs JJ)
{
    const SgScanJob &J = JJ.j[blockIdx.y];
    const uint32_t total = sg_scan_block_sums(J.n, J.bsum);
    if (threadIdx.x == 0) *J.total = (int32_t)total;
}
static void sg_mesh_scan(const SgScanJob &a, const SgScanJob *b, hipStream_t st)
{
    SgScanJobs JJ;
    JJ.j[0] = a; JJ.j[1] = b ? *b : a;
    const int nmax = b && b->n > a.n ? b->n : a.n;
    const unsigned nb = (unsigned)(((long long)nmax + 1023) / 1024);
    if (nb > 0)
        hipLaunchKernelGGL(sg_mesh_scan1_kernel, dim3(nb, b ? 2 : 1), dim3(256), 0, st, JJ);
    hipLaunchKernelGGL(sg_mesh_scan2_kernel, dim3(1, b ? 2 : 1), dim3(1024), 0, st, JJ);
}

// ---- workspace: uint32 words, every piece on a 256-byte boundary; the pieces that must start at zero come first
struct SgMeshWs {
    uint32_t *count, *cursor, *ucount;           // [V] each: instances per row, slots handed out, heads per row (zeroed per call)
    uint32_t *start, *ebase;                     // [V]: scan of count / ucount (block-local part)
    uint32_t *bsum_v, *bsum_u, *bsum_f;          // block sums of the three scans
    uint32_t *frank;                             // [F]: flagged faces in front of f (block-local part)
    uint32_t *row_b, *slot_row, *face_slot;      // [3F]: the b of a slot, its row, the slot of face edge (f, k)
    uint32_t *head;                              // [3F]: multiplicity << 1 | head, per slot
    int32_t *total;                              // [4]: totals of scans that report to nobody else
    size_t zero_words, words;
};
static inline size_t sg_mesh_pad(size_t w) { return (w + 63) & ~(size_t)63; }
static SgMeshWs sg_mesh_carve(void *ws, int V, int F)
{
    SgMeshWs w;
    uint32_t *p = (uint32_t *)ws;
    size_t o = 0;
    const size_t v = sg_mesh_pad((size_t)V), f = sg_mesh_pad((size_t)F), f3 = sg_mesh_pad(3 * (size_t)F);
    const size_t bv = sg_mesh_pad(((size_t)V + 1023) / 1024 + 1), bf = sg_mesh_pad(((size_t)F + 1023) / 1024 + 1);
    w.count = p + o; o += v;  w.cursor = p + o; o += v;  w.ucount = p + o; o += v;
    w.zero_words = o;
    w.start = p + o; o += v;  w.ebase = p + o; o += v;
    w.bsum_v = p + o; o += bv;  w.bsum_u = p + o; o += bv;  w.bsum_f = p + o; o += bf;
    w.frank = p + o; o += f;
    w.row_b = p + o; o += f3;  w.slot_row = p + o; o += f3;  w.face_slot = p + o; o += f3;  w.head = p + o; o += f3;
    w.total = (int32_t *)(p + o); o += 64;
    w.words = o;
    return w;
}
static const char *sg_mesh_bad_sizes(int V, int F)
{
    if (V < 0 || F < 0) return "V and F must be >= 0";
    if (V > SG_MESH_MAX_V) return "V beyond the scan's range (2^30 vertices)";
    if (F > SG_MESH_MAX_F) return "F beyond 2^31 / 3 faces";
    return nullptr;
}
extern "C" size_t sg_mesh_ws_bytes(int V, int F)
{
    if (sg_mesh_bad_sizes(V, F)) return 0;
    return sg_mesh_carve(nullptr, V, F).words * sizeof(uint32_t);
}

// ---- the instances
__device__ __forceinline__ bool sg_mesh_flagged(const uint8_t *__restrict__ flags, int f) { return !flags || flags[f] != 0; }
// corners of face f; false (and nothing read further) when one of them is outside [0, V)
__device__ __forceinline__ bool sg_mesh_face(const int32_t *__restrict__ faces, int f, int V, int v[3])
{
    v[0] = faces[3 * (size_t)f]; v[1] = faces[3 * (size_t)f + 1]; v[2] = faces[3 * (size_t)f + 2];
    return (uint32_t)v[0] < (uint32_t)V && (uint32_t)v[1] < (uint32_t)V && (uint32_t)v[2] < (uint32_t)V;
}
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_count_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ flags, uint32_t *__restrict__ count,
                     int32_t *__restrict__ info)
{
    const int f = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!sg_mesh_face(faces, f, V, v)) { atomicOr(&info[2], 1); return; }       // (every face is checked: subdivision copies the others)
    if (!sg_mesh_flagged(flags, f)) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int p = v[k], q = v[(k + 1) % 3];
        atomicAdd(&count[p < q ? p : q], 1u);
    }
}
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_fill_kernel(int V, int F, const int32_t *__restrict__ faces, const uint8_t *__restrict__ flags, SgMeshWs w)
{
    const int f = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!sg_mesh_face(faces, f, V, v) || !sg_mesh_flagged(flags, f)) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int p = v[k], q = v[(k + 1) % 3];
        const uint32_t a = (uint32_t)(p < q ? p : q), b = (uint32_t)(p < q ? q : p);
        const uint32_t slot = w.start[a] + w.bsum_v[a >> 10] + atomicAdd(&w.cursor[a], 1u);      // < count's total <= 3F
        w.row_b[slot] = b;
        w.slot_row[slot] = a;
        w.face_slot[3 * (size_t)f + k] = slot;
    }
}
// one lane per slot: head flag and multiplicity from the row's contents; heads counted per row
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_heads_kernel(const int32_t *__restrict__ info, SgMeshWs w)
{
    const uint32_t t = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (t >= (uint32_t)info[3]) return;
    const uint32_t a = w.slot_row[t], b = w.row_b[t];
    const uint32_t s0 = w.start[a] + w.bsum_v[a >> 10], len = w.count[a];
    uint32_t before = 0, same = 0;
    for (uint32_t j = 0; j < len; j++) {
        const bool eq = w.row_b[s0 + j] == b;
        same += eq ? 1u : 0u;
        before += (eq && s0 + j < t) ? 1u : 0u;
    }
    w.head[t] = same << 1 | (before == 0 ? 1u : 0u);
    if (before == 0) atomicAdd(&w.ucount[a], 1u);
}
// one lane per face edge: its edge's place = first edge of the row + heads of the row with a smaller b; the head writes the edge
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_emit_kernel(int V, int F, int E, const int32_t *__restrict__ faces, const uint8_t *__restrict__ flags, SgMeshWs w,
                    int32_t *__restrict__ edges, int32_t *__restrict__ edge_faces, int32_t *__restrict__ face_edges)
{
    const size_t i = (size_t)blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (i >= 3 * (size_t)F) return;
    const int f = (int)(i / 3);
    int v[3];
    if (!sg_mesh_face(faces, f, V, v) || !sg_mesh_flagged(flags, f)) { face_edges[i] = -1; return; }
    const uint32_t t = w.face_slot[i];
    const uint32_t a = w.slot_row[t], b = w.row_b[t];
    const uint32_t s0 = w.start[a] + w.bsum_v[a >> 10], len = w.count[a];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < len; j++)
        rank += ((w.head[s0 + j] & 1u) && w.row_b[s0 + j] < b) ? 1u : 0u;
    const uint32_t e = w.ebase[a] + w.bsum_u[a >> 10] + rank;
    face_edges[i] = (int32_t)e;
    const uint32_t h = w.head[t];
    if ((h & 1u) && e < (uint32_t)E) {                                   // (E is the host's copy of info[0]: never past the outputs)
        edges[2 * (size_t)e] = (int32_t)a; edges[2 * (size_t)e + 1] = (int32_t)b;
        edge_faces[e] = (int32_t)(h >> 1);
    }
}

extern "C" int sg_mesh_edges_build(int V, int F, const int32_t *faces, const uint8_t *flags, void *ws, int32_t *info, void *stream)
{
    const char *bad = sg_mesh_bad_sizes(V, F);
    if (bad) return sg_set_error(bad, hipSuccess);
    if (!info || (F > 0 && (!faces || !ws))) return sg_set_error("sg_mesh_edges_build: null pointer", hipSuccess);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(info, 0, 4 * sizeof(int32_t), st);
    if (e != hipSuccess) return sg_set_error("sg_mesh_edges_build (info)", e);
    if (F == 0) return 0;                                                // E = 0, nothing to launch
    if (V == 0) {                                                        // every index is outside an empty vertex set
        e = hipMemsetAsync(info + 2, 1, 1, st);                          // (the low byte: info[2] = 1)
        return e == hipSuccess ? 0 : sg_set_error("sg_mesh_edges_build (info)", e);
    }
    const SgMeshWs w = sg_mesh_carve(ws, V, F);
    e = hipMemsetAsync(w.count, 0, w.zero_words * sizeof(uint32_t), st);
    if (e != hipSuccess) return sg_set_error("sg_mesh_edges_build (workspace)", e);
    const unsigned fb = ((unsigned)F + SG_MESH_THREADS - 1) / SG_MESH_THREADS;
    const unsigned ib = (unsigned)((3 * (size_t)F + SG_MESH_THREADS - 1) / SG_MESH_THREADS);
    hipLaunchKernelGGL(sg_mesh_count_kernel, dim3(fb), dim3(SG_MESH_THREADS), 0, st, V, F, faces, flags, w.count, info);
    // rows (total -> info[3], the number of instances) and flagged faces (total -> info[1]) in the same two launches
    const SgScanJob rows = {w.count, nullptr, w.start, w.bsum_v, info + 3, V};
    const SgScanJob flg = {nullptr, flags, w.frank, w.bsum_f, info + 1, F};
    sg_mesh_scan(rows, &flg, st);
    hipLaunchKernelGGL(sg_mesh_fill_kernel, dim3(fb), dim3(SG_MESH_THREADS), 0, st, V, F, faces, flags, w);
    hipLaunchKernelGGL(sg_mesh_heads_kernel, dim3(ib), dim3(SG_MESH_THREADS), 0, st, info, w);
    const SgScanJob uniq = {w.ucount, nullptr, w.ebase, w.bsum_u, info, V};
    sg_mesh_scan(uniq, nullptr, st);
    return sg_launched("sg_mesh_edges_build");
}

extern "C" int sg_mesh_edges_emit(int V, int F, int E, const int32_t *faces, const uint8_t *flags, const void *ws, int32_t *edges,
                                  int32_t *edge_faces, int32_t *face_edges, void *stream)
{
    const char *bad = sg_mesh_bad_sizes(V, F);
    if (bad) return sg_set_error(bad, hipSuccess);
    if (E < 0 || (size_t)E > 3 * (size_t)F) return sg_set_error("sg_mesh_edges_emit: E must be 0 .. 3 F", hipSuccess);
    if ((long long)V + E >= (1ll << 31)) return sg_set_error("sg_mesh_edges_emit: V + E >= 2^31 (midpoint indices are int32)", hipSuccess);
    if (F == 0) return 0;
    if (V == 0) return sg_set_error("sg_mesh_edges_emit: faces without vertices", hipSuccess);
    if (!faces || !ws || !face_edges || (E > 0 && (!edges || !edge_faces)))
        return sg_set_error("sg_mesh_edges_emit: null pointer", hipSuccess);
    const SgMeshWs w = sg_mesh_carve((void *)ws, V, F);
    const unsigned ib = (unsigned)((3 * (size_t)F + SG_MESH_THREADS - 1) / SG_MESH_THREADS);
    hipLaunchKernelGGL(sg_mesh_emit_kernel, dim3(ib), dim3(SG_MESH_THREADS), 0, (hipStream_t)stream, V, F, E, faces, flags, w, edges,
                       edge_faces, face_edges);
    return sg_launched("sg_mesh_edges_emit");
}

// ---- selective subdivision (geometry_ops.py:41-58): the unflagged faces in their order, then four children per flagged face
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_subdivide_kernel(int V, int F, int Fs, const int32_t *__restrict__ faces, const uint8_t *__restrict__ flags,
                         const int32_t *__restrict__ face_edges, const uint32_t *__restrict__ frank,
                         const uint32_t *__restrict__ bsum_f, int32_t *__restrict__ out)
{
    const int f = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (f >= F) return;
    const uint32_t r = frank[f] + bsum_f[f >> 10];                       // flagged faces in front of f
    const int v0 = faces[3 * (size_t)f], v1 = faces[3 * (size_t)f + 1], v2 = faces[3 * (size_t)f + 2];
    if (!sg_mesh_flagged(flags, f)) {
        const size_t o = (size_t)f - r;
        if (o >= (size_t)(F - Fs)) return;                               // (a stale Fs: never past the output)
        out[3 * o] = v0; out[3 * o + 1] = v1; out[3 * o + 2] = v2;
        return;
    }
    if (r >= (uint32_t)Fs) return;
    const int m0 = V + face_edges[3 * (size_t)f], m1 = V + face_edges[3 * (size_t)f + 1], m2 = V + face_edges[3 * (size_t)f + 2];
    int32_t *o = out + 3 * ((size_t)(F - Fs) + 4 * (size_t)r);
    o[0] = v0; o[1] = m0; o[2] = m2;
    o[3] = m0; o[4] = v1; o[5] = m1;
    o[6] = m2; o[7] = m1; o[8] = v2;
    o[9] = m0; o[10] = m1; o[11] = m2;
}
extern "C" int sg_mesh_subdivide(int V, int F, int Fs, const int32_t *faces, const uint8_t *flags, const int32_t *face_edges, void *ws,
                                 int32_t *new_faces, void *stream)
{
    const char *bad = sg_mesh_bad_sizes(V, F);
    if (bad) return sg_set_error(bad, hipSuccess);
    if (Fs < 0 || Fs > F) return sg_set_error("sg_mesh_subdivide: Fs must be 0 .. F", hipSuccess);
    if ((size_t)(F - Fs) + 4 * (size_t)Fs > (size_t)SG_MESH_MAX_F) return sg_set_error("sg_mesh_subdivide: too many faces out", hipSuccess);
    if (F == 0) return 0;
    if (!faces || !ws || !new_faces || (Fs > 0 && !face_edges)) return sg_set_error("sg_mesh_subdivide: null pointer", hipSuccess);
    hipStream_t st = (hipStream_t)stream;
    const SgMeshWs w = sg_mesh_carve(ws, V, F);
    // (the flags are scanned again: the call does not depend on what another call left in the workspace)
    const SgScanJob flg = {nullptr, flags, w.frank, w.bsum_f, w.total, F};
    sg_mesh_scan(flg, nullptr, st);
    const unsigned fb = ((unsigned)F + SG_MESH_THREADS - 1) / SG_MESH_THREADS;
    hipLaunchKernelGGL(sg_mesh_subdivide_kernel, dim3(fb), dim3(SG_MESH_THREADS), 0, st, V, F, Fs, faces, flags, face_edges, w.frank,
                       w.bsum_f, new_faces);
    return sg_launched("sg_mesh_subdivide");
}

// ---- midpoint rows: dst[e] = (src[a] + src[b]) * 0.5f (one add, one exact scaling: the bits of `values[rows].mean(axis=1)`), or
// src[a] for labels.  Rows of a multiple of four floats on 16-byte boundaries move as float4 (sg_skin.h's weight rows); any other
// width one float per lane, lanes consecutive over the flat [E, C] output.  An endpoint outside [0, V) is never dereferenced.
template <typename T, bool MEAN>
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_midpoints_kernel(int V, size_t n, int width, const int32_t *__restrict__ edges, const T *__restrict__ src, T *__restrict__ dst)
{
    for (size_t i = (size_t)blockIdx.x * SG_MESH_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * SG_MESH_THREADS) {
        const size_t e = i / (size_t)width, c = i - e * (size_t)width;
        const int a = edges[2 * e], b = edges[2 * e + 1];
        T r = {};
        if ((uint32_t)a < (uint32_t)V && (uint32_t)b < (uint32_t)V) {
            r = src[(size_t)a * width + c];
            if constexpr (MEAN) r = (r + src[(size_t)b * width + c]) * 0.5f;
        }
        dst[i] = r;
    }
}
// S: the scalar (float: the mean; int32_t: the smaller endpoint's value), S4: its 16-byte vector
template <typename S, typename S4, bool MEAN>
static int sg_mesh_midpoints_launch(const char *what, int V, int E, int C, const int32_t *edges, const S *src, S *dst, void *stream)
{
    if (V < 0 || E < 0 || C < 1) return sg_set_error("sg_mesh_midpoints: V, E >= 0 and C >= 1", hipSuccess);
    if (E == 0) return 0;
    if (!edges || !src || !dst) return sg_set_error("sg_mesh_midpoints: null pointer", hipSuccess);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int width = vec ? C / 4 : C;
    const size_t n = (size_t)E * width;
    const size_t want = (n + SG_MESH_THREADS - 1) / SG_MESH_THREADS;
    const unsigned blocks = (unsigned)(want < 65536 ? want : 65536);
    if (vec)
        hipLaunchKernelGGL((sg_mesh_midpoints_kernel<S4, MEAN>), dim3(blocks), dim3(SG_MESH_THREADS), 0, st, V, n, width, edges,
                           (const S4 *)src, (S4 *)dst);
    else
        hipLaunchKernelGGL((sg_mesh_midpoints_kernel<S, MEAN>), dim3(blocks), dim3(SG_MESH_THREADS), 0, st, V, n, width, edges, src, dst);
    return sg_launched(what);
}
extern "C" int sg_mesh_midpoints(int V, int E, int C, const int32_t *edges, const float *src, float *dst, void *stream)
{
    return sg_mesh_midpoints_launch<float, float4, true>("sg_mesh_midpoints", V, E, C, edges, src, dst, stream);
}
extern "C" int sg_mesh_midpoints_i32(int V, int E, int C, const int32_t *edges, const int32_t *src, int32_t *dst, void *stream)
{
    return sg_mesh_midpoints_launch<int32_t, int4, false>("sg_mesh_midpoints_i32", V, E, C, edges, src, dst, stream);
}

// ---- edge collapse (geometry_ops.py:79-167, the mesh half of sings_hybrid.py's prune_and_simplify): merge the larger endpoint of the
// longest live selected edge into the smaller one, num_collapse times; then map the faces, drop the degenerate ones and all but the
// first of every set of faces on the same three vertices, prune the vertices no face is left on, renumber.
//
// The reference's loop as a quotient graph: a class is represented by its smallest vertex, which never moves (only deleted vertices
// are overwritten), so a live edge's length is always the distance of two INPUT positions and no position is ever written.  The loop
// is sequential -- a collapse changes its neighbours' lengths -- but small (the reference skips above 10 000 selected edges): ONE
// workgroup of 1 024 lanes keeps (a, b, squared length) of every edge in LDS, entry i with lane i % 1024 and touched by no other lane,
// and runs every iteration without a launch or a host read:
//
//   pick      each lane's best key (length^2 larger, then a smaller, then b smaller) -> wave reduction -> 16 partials, barrier, read by
//             all.  The list is duplicate-free, so the key names ONE edge (v1 < v2) whatever entry holds it.
//   relabel   parent[v2] = v1.  Entries with v2 take v1 (pair re-sorted, length from the input positions); the self-edge dies.
//   merge     a relabelled (v1, x) that a live untouched (v1, x) already holds dies: the untouched ones write stamp[x] = iteration,
//             barrier, the relabelled ones read it.  (Two relabelled entries cannot meet: they were (v2, x) for distinct x.)
//
// Duplicate input rows are merged at load through a hash set (WHICH copy stays is arrival order; the copies are equal).  Afterwards
// ordinary kernels: roots of `parent`, faces counted into the row of their smallest mapped corner (the unique edges' idiom: "a face
// with a smaller index in my row has my other two corners" is a predicate over the row's contents), the file's scan, compaction in
// the original order.  The host reads info[] once between _build and _emit.
#define SG_COLLAPSE_LANES 1024
#define SG_COLLAPSE_PER_LANE 10
#define SG_COLLAPSE_MAX_EDGES (SG_COLLAPSE_LANES * SG_COLLAPSE_PER_LANE)         // 10 240 >= the reference's 2 * prune_max_n_gs_once
#define SG_COLLAPSE_HASH (1 << 15)               // slots of the load's hash set: more than three per edge
#define SG_COLLAPSE_DEAD 0xffffffffu
#define SG_COLLAPSE_EMPTY (~0ull)
#define SG_COLLAPSE_LDS_BYTES (3 * SG_COLLAPSE_MAX_EDGES * sizeof(uint32_t))    // 120 KiB of the CU's 160

struct SgCollapseWs {
    int32_t *parent, *cmap;                      // [V]: the vertex a vertex was merged into (itself: none); its class' representative
    uint32_t *stamp, *seen;                      // [V]: the iteration a live (v1, x) was last seen for x; endpoint of a selected edge
    uint32_t *count, *cursor, *start, *vrank;    // [V]: faces in the row, slots handed out, row starts / used vertices in front (block-local)
    uint32_t *frank, *slot_face, *slot_mid, *slot_max;       // [F]: kept faces in front (block-local); per slot the face and its other corners
    uint32_t *bsum_c, *bsum_v, *bsum_f;          // block sums of the three scans
    uint8_t *used, *keep;                        // [V], [F] flags
    unsigned long long *hash;                    // [SG_COLLAPSE_HASH]
    size_t words;
};
static SgCollapseWs sg_collapse_carve(void *ws, int V, int F)
{
    SgCollapseWs w;
    uint32_t *p = (uint32_t *)ws;
    size_t o = 0;
    const size_t v = sg_mesh_pad((size_t)V), f = sg_mesh_pad((size_t)F);
    const size_t bv = sg_mesh_pad(((size_t)V + 1023) / 1024 + 1), bf = sg_mesh_pad(((size_t)F + 1023) / 1024 + 1);
    w.hash = (unsigned long long *)(p + o); o += 2 * (size_t)SG_COLLAPSE_HASH;
    w.parent = (int32_t *)(p + o); o += v;  w.cmap = (int32_t *)(p + o); o += v;
    w.stamp = p + o; o += v;  w.seen = p + o; o += v;
    w.count = p + o; o += v;  w.cursor = p + o; o += v;  w.start = p + o; o += v;  w.vrank = p + o; o += v;
    w.frank = p + o; o += f;  w.slot_face = p + o; o += f;  w.slot_mid = p + o; o += f;  w.slot_max = p + o; o += f;
    w.bsum_c = p + o; o += bv;  w.bsum_v = p + o; o += bv;  w.bsum_f = p + o; o += bf;
    w.used = (uint8_t *)(p + o); o += sg_mesh_pad(((size_t)V + 3) / 4);
    w.keep = (uint8_t *)(p + o); o += sg_mesh_pad(((size_t)F + 3) / 4);
    w.words = o;
    return w;
}
extern "C" int sg_mesh_collapse_max_edges(void) { return SG_COLLAPSE_MAX_EDGES; }
extern "C" size_t sg_mesh_collapse_ws_bytes(int V, int F)
{
    if (V < 1 || sg_mesh_bad_sizes(V, F)) return 0;
    return sg_collapse_carve(nullptr, V, F).words * sizeof(uint32_t);
}

__device__ __forceinline__ bool sg_collapse_finite3(const float *__restrict__ p)
{
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}
// every piece the call reads before it writes it, and info[]
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_collapse_init_kernel(int V, int F, SgCollapseWs w, int32_t *__restrict__ info)
{
    const size_t n = (size_t)(V > F ? V : F) > (size_t)SG_COLLAPSE_HASH ? (size_t)(V > F ? V : F) : (size_t)SG_COLLAPSE_HASH;
    for (size_t i = (size_t)blockIdx.x * SG_MESH_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * SG_MESH_THREADS) {
        if (i < (size_t)V) {
            w.parent[i] = (int32_t)i; w.stamp[i] = 0; w.seen[i] = 0; w.count[i] = 0; w.cursor[i] = 0; w.used[i] = 0;
        }
        if (i < (size_t)F) w.keep[i] = 0;
        if (i < (size_t)SG_COLLAPSE_HASH) w.hash[i] = SG_COLLAPSE_EMPTY;
        if (i < 8) info[i] = 0;
    }
}
__device__ __forceinline__ float sg_collapse_len2(const float *__restrict__ verts, uint32_t a, uint32_t b)
{
    const float *p = verts + 3 * (size_t)a, *q = verts + 3 * (size_t)b;
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}
// (hi, lo) of the better of two keys: hi = the bits of length^2 (>= +0: ordered as integers), lo = (2^31 - 1 - a, 2^31 - 1 - b), 0 = none
__device__ __forceinline__ void sg_collapse_better(uint32_t &hi, unsigned long long &lo, uint32_t h, unsigned long long l)
{
    if (h > hi || (h == hi && l > lo)) { hi = h; lo = l; }
}
__global__ void __launch_bounds__(SG_COLLAPSE_LANES)
sg_mesh_collapse_loop_kernel(int V, int Es, const float *__restrict__ verts, const int32_t *__restrict__ sel, double rate, SgCollapseWs w,
                             int32_t *info)
{
    extern __shared__ uint32_t sg_collapse_lds[];                     // a | b | length^2, SG_COLLAPSE_MAX_EDGES each
    uint32_t *const sA = sg_collapse_lds, *const sB = sg_collapse_lds + SG_COLLAPSE_MAX_EDGES;
    float *const sL = (float *)(sg_collapse_lds + 2 * SG_COLLAPSE_MAX_EDGES);
    __shared__ uint32_t sHi[SG_COLLAPSE_LANES / 64];
    __shared__ unsigned long long sLo[SG_COLLAPSE_LANES / 64];
    __shared__ int sBad, sDistinct;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { sBad = 0; sDistinct = 0; }
    __syncthreads();
    // load: rows outside 0 <= a < b < V and non-finite endpoints are reported and never dereferenced; duplicates merged
    int bad = 0, distinct = 0;
#pragma unroll
    for (int k = 0; k < SG_COLLAPSE_PER_LANE; k++) {
        const int i = k * SG_COLLAPSE_LANES + tid;
        if (i >= Es) continue;
        uint32_t a = SG_COLLAPSE_DEAD, b = SG_COLLAPSE_DEAD;
        float l = 0.f;
        const int ea = sel[2 * (size_t)i], eb = sel[2 * (size_t)i + 1];
        if (!(ea >= 0 && ea < eb && eb < V)) bad |= 1;
        else if (!sg_collapse_finite3(verts + 3 * (size_t)ea) || !sg_collapse_finite3(verts + 3 * (size_t)eb)) bad |= 2;
        else {
            const unsigned long long key = (unsigned long long)(uint32_t)ea << 32 | (uint32_t)eb;
            uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 49);         // 15 bits
            bool dup = false;
            for (;;) {                                               // (at most Es < SG_COLLAPSE_HASH slots are ever taken: an empty one exists)
                const unsigned long long old = atomicCAS(&w.hash[h], SG_COLLAPSE_EMPTY, key);
                if (old == SG_COLLAPSE_EMPTY) break;
                if (old == key) { dup = true; break; }
                h = (h + 1) & (SG_COLLAPSE_HASH - 1);
            }
            if (!dup) {
                a = (uint32_t)ea; b = (uint32_t)eb; l = sg_collapse_len2(verts, a, b);
                distinct += atomicExch(&w.seen[a], 1u) == 0u ? 1 : 0;            // (a sum of ones: no order)
                distinct += atomicExch(&w.seen[b], 1u) == 0u ? 1 : 0;
            }
        }
        sA[i] = a; sB[i] = b; sL[i] = l;
    }
    if (bad) atomicOr(&sBad, bad);
    if (distinct) atomicAdd(&sDistinct, distinct);
    __syncthreads();
    if (sBad != 0) {                                                 // (uniform) nothing is collapsed; the host raises
        if (tid == 0) { info[3] = sBad; info[5] = sDistinct; }
        return;
    }
    // int(n_distinct * collapse_rate) as Python forms it, in double
    double want = (double)sDistinct * rate;
    want = want < 0.0 ? 0.0 : (want > 1073741824.0 ? 1073741824.0 : want);
    const int num = (int)want;
    int done = 0;
    for (int it = 0; it < num; it++) {
        uint32_t hi = 0;
        unsigned long long lo = 0;
#pragma unroll
        for (int k = 0; k < SG_COLLAPSE_PER_LANE; k++) {
            const int i = k * SG_COLLAPSE_LANES + tid;
            if (i >= Es) continue;
            const uint32_t a = sA[i];
            if (a == SG_COLLAPSE_DEAD) continue;
            sg_collapse_better(hi, lo, __float_as_uint(sL[i]), (unsigned long long)(0x7fffffffu - a) << 32 | (0x7fffffffu - sB[i]));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t h = __shfl_xor(hi, o, 64), l1 = __shfl_xor((uint32_t)(lo >> 32), o, 64), l0 = __shfl_xor((uint32_t)lo, o, 64);
            sg_collapse_better(hi, lo, h, (unsigned long long)l1 << 32 | l0);
        }
        if (lane == 0) { sHi[wave] = hi; sLo[wave] = lo; }
        __syncthreads();
        hi = 0; lo = 0;
#pragma unroll
        for (int x = 0; x < SG_COLLAPSE_LANES / 64; x++) sg_collapse_better(hi, lo, sHi[x], sLo[x]);
        if (lo == 0) break;                                          // (uniform) "No edge could be collapsed."
        const uint32_t v1 = 0x7fffffffu - (uint32_t)(lo >> 32), v2 = 0x7fffffffu - (uint32_t)lo, tag = (uint32_t)it + 1u;
        if (tid == 0) w.parent[v2] = (int32_t)v1;
        done++;
        uint32_t pend = 0;
#pragma unroll
        for (int k = 0; k < SG_COLLAPSE_PER_LANE; k++) {
            const int i = k * SG_COLLAPSE_LANES + tid;
            if (i >= Es) continue;
            const uint32_t a = sA[i], b = sB[i];
            if (a == SG_COLLAPSE_DEAD) continue;
            if (a == v2 || b == v2) {
                const uint32_t x = a == v2 ? b : a;
                if (x == v1) { sA[i] = SG_COLLAPSE_DEAD; continue; }             // the collapsed edge itself
                sA[i] = x < v1 ? x : v1; sB[i] = x < v1 ? v1 : x;
                sL[i] = sg_collapse_len2(verts, v1, x);
                pend |= 1u << k;
            } else if (a == v1) w.stamp[b] = tag;
            else if (b == v1) w.stamp[a] = tag;
        }
        __syncthreads();                                             // (the stamps of this workgroup's other waves are visible behind it)
#pragma unroll
        for (int k = 0; k < SG_COLLAPSE_PER_LANE; k++) {
            if (!(pend >> k & 1u)) continue;
            const int i = k * SG_COLLAPSE_LANES + tid;
            const uint32_t x = sA[i] == v1 ? sB[i] : sA[i];
            if (w.stamp[x] == tag) sA[i] = SG_COLLAPSE_DEAD;
        }
    }
    if (tid == 0) { info[2] = done; info[5] = sDistinct; info[6] = num; }
}
// roots of `parent` (a chain only descends: it ends); every vertex checked for a non-finite coordinate
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_collapse_map_kernel(int V, const float *__restrict__ verts, SgCollapseWs w, int32_t *__restrict__ info)
{
    const int v = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (v >= V) return;
    if (!sg_collapse_finite3(verts + 3 * (size_t)v)) atomicOr(&info[3], 2);
    int p = v;
    for (int q = w.parent[p]; q != p; q = w.parent[p]) p = q;
    w.cmap[v] = p;
}
// mapped corners of face f in the face's own order; false: a corner outside [0, V) (-1) or two corners equal (0)
__device__ __forceinline__ int sg_collapse_face(const int32_t *__restrict__ faces, int f, int V, const int32_t *__restrict__ cmap, int m[3])
{
    int v[3];
    if (!sg_mesh_face(faces, f, V, v)) return -1;
    m[0] = cmap[v[0]]; m[1] = cmap[v[1]]; m[2] = cmap[v[2]];
    return (m[0] != m[1] && m[1] != m[2] && m[0] != m[2]) ? 1 : 0;
}
__device__ __forceinline__ void sg_collapse_sorted(const int m[3], uint32_t &lo, uint32_t &mid, uint32_t &hi)
{
    const int a = m[0] < m[1] ? m[0] : m[1], b = m[0] < m[1] ? m[1] : m[0];
    lo = (uint32_t)(a < m[2] ? a : m[2]);
    hi = (uint32_t)(b > m[2] ? b : m[2]);
    mid = ((uint32_t)m[0] + (uint32_t)m[1] + (uint32_t)m[2]) - lo - hi;          // (three indices below 2^30: no wrap)
}
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_collapse_count_kernel(int V, int F, const int32_t *__restrict__ faces, SgCollapseWs w, int32_t *__restrict__ info)
{
    const int f = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (f >= F) return;
    int m[3];
    const int s = sg_collapse_face(faces, f, V, w.cmap, m);
    if (s < 0) { atomicOr(&info[4], 1); return; }
    if (s == 0) return;
    uint32_t lo, mid, hi;
    sg_collapse_sorted(m, lo, mid, hi);
    atomicAdd(&w.count[lo], 1u);
}
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_collapse_fill_kernel(int V, int F, const int32_t *__restrict__ faces, SgCollapseWs w)
{
    const int f = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (f >= F) return;
    int m[3];
    if (sg_collapse_face(faces, f, V, w.cmap, m) <= 0) return;
    uint32_t lo, mid, hi;
    sg_collapse_sorted(m, lo, mid, hi);
    const uint32_t slot = w.start[lo] + w.bsum_c[lo >> 10] + atomicAdd(&w.cursor[lo], 1u);      // < count's total <= F
    w.slot_face[slot] = (uint32_t)f; w.slot_mid[slot] = mid; w.slot_max[slot] = hi;
}
// kept: no face with a smaller index holds the same three vertices (counted over the row's contents: any slot order gives the same)
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_collapse_keep_kernel(int V, int F, const int32_t *__restrict__ faces, SgCollapseWs w)
{
    const int f = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (f >= F) return;
    int m[3];
    if (sg_collapse_face(faces, f, V, w.cmap, m) <= 0) return;
    uint32_t lo, mid, hi;
    sg_collapse_sorted(m, lo, mid, hi);
    const uint32_t s0 = w.start[lo] + w.bsum_c[lo >> 10], len = w.count[lo];
    uint32_t before = 0;
    for (uint32_t j = 0; j < len; j++)
        before += (w.slot_mid[s0 + j] == mid && w.slot_max[s0 + j] == hi && w.slot_face[s0 + j] < (uint32_t)f) ? 1u : 0u;
    if (before != 0) return;
    w.keep[f] = 1;
    w.used[m[0]] = 1; w.used[m[1]] = 1; w.used[m[2]] = 1;            // (every writer writes 1)
}
__global__ void __launch_bounds__(SG_MESH_THREADS)
sg_mesh_collapse_emit_kernel(int V, int F, int Fn, int Vn, const int32_t *__restrict__ faces, SgCollapseWs w, int32_t *__restrict__ new_faces,
                             uint8_t *__restrict__ prune_mask, int32_t *__restrict__ survivors)
{
    const int i = blockIdx.x * SG_MESH_THREADS + threadIdx.x;
    if (i < F && w.keep[i]) {
        int m[3];
        const uint32_t o = w.frank[i] + w.bsum_f[i >> 10];
        if (o < (uint32_t)Fn && sg_collapse_face(faces, i, V, w.cmap, m) > 0) {  // (a stale Fn: never past the output)
#pragma unroll
            for (int k = 0; k < 3; k++) new_faces[3 * (size_t)o + k] = (int32_t)(w.vrank[m[k]] + w.bsum_v[m[k] >> 10]);
        }
    }
    if (i < V) {
        const bool u = w.used[i] != 0;
        prune_mask[i] = u ? 0 : 1;
        const uint32_t o = w.vrank[i] + w.bsum_v[i >> 10];
        if (u && o < (uint32_t)Vn) survivors[o] = i;
    }
}

static const char *sg_collapse_bad_sizes(int V, int F)
{
    if (V < 1) return "sg_mesh_collapse: V must be >= 1";
    return sg_mesh_bad_sizes(V, F);
}
extern "C" int sg_mesh_collapse_build(int V, int F, int Es, const float *verts, const int32_t *selected_edges, const int32_t *faces,
                                      const double *collapse_rate, void *ws, int32_t *info, void *stream)
{
    const char *bad = sg_collapse_bad_sizes(V, F);
    if (bad) return sg_set_error(bad, hipSuccess);
    if (Es < 0) return sg_set_error("sg_mesh_collapse_build: Es must be >= 0", hipSuccess);
    if (Es > SG_COLLAPSE_MAX_EDGES) return sg_set_error("sg_mesh_collapse_build: more selected edges than sg_mesh_collapse_max_edges()", hipSuccess);
    if (!verts || !ws || !info || !collapse_rate || (Es > 0 && !selected_edges) || (F > 0 && !faces))
        return sg_set_error("sg_mesh_collapse_build: null pointer", hipSuccess);
    const double rate = *collapse_rate;
    if (!(rate >= 0.0) || !(rate <= 1.0e9)) return sg_set_error("sg_mesh_collapse_build: collapse_rate must be finite and >= 0", hipSuccess);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipFuncSetAttribute((const void *)sg_mesh_collapse_loop_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)SG_COLLAPSE_LDS_BYTES);
    if (e != hipSuccess) return sg_set_error("sg_mesh_collapse_build (LDS limit)", e);
    const SgCollapseWs w = sg_collapse_carve(ws, V, F);
    const int nmax = V > F ? (V > SG_COLLAPSE_HASH ? V : SG_COLLAPSE_HASH) : (F > SG_COLLAPSE_HASH ? F : SG_COLLAPSE_HASH);
    const unsigned want = ((unsigned)nmax + SG_MESH_THREADS - 1) / SG_MESH_THREADS;
    const unsigned vb = ((unsigned)V + SG_MESH_THREADS - 1) / SG_MESH_THREADS, fb = ((unsigned)F + SG_MESH_THREADS - 1) / SG_MESH_THREADS;
    hipLaunchKernelGGL(sg_mesh_collapse_init_kernel, dim3(want < 65536 ? want : 65536), dim3(SG_MESH_THREADS), 0, st, V, F, w, info);
    hipLaunchKernelGGL(sg_mesh_collapse_loop_kernel, dim3(1), dim3(SG_COLLAPSE_LANES), SG_COLLAPSE_LDS_BYTES, st, V, Es, verts,
                       selected_edges, rate, w, info);
    hipLaunchKernelGGL(sg_mesh_collapse_map_kernel, dim3(vb), dim3(SG_MESH_THREADS), 0, st, V, verts, w, info);
    if (F > 0) {
        hipLaunchKernelGGL(sg_mesh_collapse_count_kernel, dim3(fb), dim3(SG_MESH_THREADS), 0, st, V, F, faces, w, info);
        const SgScanJob rows = {w.count, nullptr, w.start, w.bsum_c, info + 7, V};
        sg_mesh_scan(rows, nullptr, st);
        hipLaunchKernelGGL(sg_mesh_collapse_fill_kernel, dim3(fb), dim3(SG_MESH_THREADS), 0, st, V, F, faces, w);
        hipLaunchKernelGGL(sg_mesh_collapse_keep_kernel, dim3(fb), dim3(SG_MESH_THREADS), 0, st, V, F, faces, w);
        // kept faces (total -> info[0]) and used vertices (total -> info[1]) in the same two launches
        const SgScanJob kept = {nullptr, w.keep, w.frank, w.bsum_f, info, F};
        const SgScanJob used = {nullptr, w.used, w.vrank, w.bsum_v, info + 1, V};
        sg_mesh_scan(kept, &used, st);
    }
    return sg_launched("sg_mesh_collapse_build");
}

extern "C" int sg_mesh_collapse_emit(int V, int F, int Fn, int Vn, const int32_t *faces, const void *ws, int32_t *new_faces,
                                     uint8_t *prune_mask, int32_t *survivors, void *stream)
{
    const char *bad = sg_collapse_bad_sizes(V, F);
    if (bad) return sg_set_error(bad, hipSuccess);
    if (Fn < 0 || Fn > F || Vn < 0 || Vn > V) return sg_set_error("sg_mesh_collapse_emit: Fn must be 0 .. F and Vn 0 .. V", hipSuccess);
    if (!ws || !prune_mask || (F > 0 && !faces) || (Fn > 0 && !new_faces) || (Vn > 0 && !survivors))
        return sg_set_error("sg_mesh_collapse_emit: null pointer", hipSuccess);
    const SgCollapseWs w = sg_collapse_carve((void *)ws, V, F);
    const unsigned n = (unsigned)(V > F ? V : F);
    hipLaunchKernelGGL(sg_mesh_collapse_emit_kernel, dim3((n + SG_MESH_THREADS - 1) / SG_MESH_THREADS), dim3(SG_MESH_THREADS), 0,
                       (hipStream_t)stream, V, F, Fn, Vn, faces, w, new_faces, prune_mask, survivors);
    return sg_launched("sg_mesh_collapse_emit");
}
