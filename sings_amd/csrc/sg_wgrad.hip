// Weight / bias gradient of a decoder layer: dW [Cout,Cin] = dz^T x, db [Cout] = column sums of dz.
// A GEMM whose reduction dimension is the N ~ 10^5 points and whose output is at most 128 x 128: the library kernels
// chosen for this shape ran at 330-430 us per layer (150 k points).  Here a workgroup owns a slice of rows and the whole
// output: wave w accumulates the 32 output rows [32w, 32w+32) x all Cin columns on the matrix cores
// (v_mfma_f32_32x32x2_f32, exact fp32 products, k-ordered accumulation).  The MFMA operand layout IS the memory layout
// of two consecutive rows (lane l: A = dz[n + l/32][32w + l%32], B = x[n + l/32][32t + l%32]), so operands are loaded
// straight from global memory with 128-B coalesced half-wave reads -- no LDS, 1 + Cin/32 loads per Cin/32 MFMAs.
// Per-workgroup partials are summed in a fixed order by sg_wgrad_reduce_kernel (deterministic).
#include "sg_common.h"

#define SG_WG_ROWS 256

// RR = rows of x / dz per round (one barrier per round): 32 for <= 96 input columns, 16 for 128 (64 rows lose again).
// Nine decoder layers at 150k points: 604 us (16-row rounds, one round of look-ahead, 256-row slices dealt round-robin)
// -> 550 (round size) -> 484 (two rounds of look-ahead) -> 423 us (one equally long row range per workgroup).
// Round 2: every load is a BUFFER load on a descriptor of the workgroup's own row range -- rows beyond it read as zero, so the
// loop has no bounds branches at all and the compiler can count its s_waitcnt vmcnt(n) (with a branch per load it fell back to
// vmcnt(0) right behind the look-ahead loads, which therefore never overlapped anything).
// SPLIT (cout_pad <= 64: the 64- and 48-output layers): only two waves own output rows, so the four waves form two PAIRS that share a
// round's RR rows -- pair g multiplies rows [g RR/2, (g + 1) RR/2) -- and leave TWO partial slabs per workgroup (the reduce kernel
// sums 2 x as many): 43.5 -> ~25 us for dW [64 x 96] at 150 k points, where two of the four matrix cores of a CU used to idle.
template <int TI, int RR, bool SPLIT>
__global__ void __launch_bounds__(256)
sg_wgrad_kernel(int N, int Cout, int Cin, const float *__restrict__ dz, const float *__restrict__ x,
                float *__restrict__ partial, float *__restrict__ bpartial, int cout_pad, int chunk)
{
    // the four waves need the same RR rows of x per round: they go through LDS once (double-buffered, one barrier per
    // round) instead of being read from L2/HBM by every wave (4x the traffic made the direct version bandwidth-bound)
    __shared__ float sX[2][RR][TI * 32 + 4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wv = SPLIT ? (wave & 1) : wave, grp = SPLIT ? (wave >> 1) : 0;           // output-row block, row group of the round
    constexpr int NU = SPLIT ? RR / 4 : RR / 2;                                        // row pairs per wave and round
    const int u0 = grp * NU;
    const bool active = 32 * wv < cout_pad;
    const int o = 32 * wv + (lane & 31), half = lane >> 5;
    constexpr int CIN = TI * 32;
    constexpr int F4 = RR * CIN / 4;          // float4 elements of one slab
    static_assert(F4 % 256 == 0, "a slab is a whole number of float4 per thread");
    constexpr int PER = F4 / 256;
    sg_v16f acc[TI];
#pragma unroll
    for (int t = 0; t < TI; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.0f;
    float bsum = 0.0f;
    // every workgroup takes ONE contiguous range of `chunk` rows (the last one may be short)
    const int r0 = blockIdx.x * chunk, len = min(chunk, N - r0);
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void *)(x + (size_t)r0 * CIN), 0, len * CIN * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsz = __builtin_amdgcn_make_buffer_rsrc((void *)(dz + (size_t)r0 * Cout), 0, len * Cout * 4, 0x00020000);
    const int zoff = (active && o < Cout) ? (half * Cout + o) * 4 : 0x7ffffff0;   // columns beyond Cout: out of range = 0
    int xoff[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int f = threadIdx.x + 256 * q, row = f / (CIN / 4), c4 = f - row * (CIN / 4);
        xoff[q] = (row * CIN + 4 * c4) * 4;
    }
    // two register sets (E, O): while round n computes out of LDS, the operands of round n + 1 sit in one set (stashed
    // to the other LDS buffer at the end of the round) and the loads of round n + 2 are in flight into the other --
    // a round's MFMAs (0.85 us) are shorter than a memory round trip, one round of look-ahead left the waves waiting
    float4 xrE[PER], xrO[PER];
    float anE[NU], anO[NU];
    auto fetch = [&](float4 (&xr)[PER], float (&an)[NU], int n) {
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsx, xoff[q] + n * (CIN * 4), 0, 0);
            xr[q] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
        }
#pragma unroll
        for (int u = 0; u < NU; u++)
            an[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsz, zoff + (n + 2 * (u0 + u)) * (Cout * 4), 0, 0));
    };
    auto stash = [&](const float4 (&xr)[PER], int buf) {
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int f = threadIdx.x + 256 * q, row = f / (CIN / 4), c4 = f - row * (CIN / 4);
            *(float4 *)&sX[buf][row][4 * c4] = xr[q];
        }
    };
    // round n: a-values from `cur` (its x rows are in sX[buf]); `oth` holds round n + 1
    auto round = [&](float4 (&xc)[PER], float (&ac)[NU], const float4 (&xo)[PER], int n, int buf) {
        float a[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) a[u] = ac[u];
        fetch(xc, ac, n + 2 * RR);
        if (active) {
#pragma unroll
            for (int u = 0; u < NU; u++) {
                bsum += a[u];
#pragma unroll
                for (int t = 0; t < TI; t++)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], sX[buf][2 * (u0 + u) + half][32 * t + (lane & 31)], acc[t], 0, 0, 0);
            }
        }
        stash(xo, buf ^ 1);
        __syncthreads();
    };
    if (len > 0) {
        fetch(xrE, anE, 0);
        fetch(xrO, anO, RR);
        stash(xrE, 0);
        __syncthreads();
        for (int n = 0; n < len; n += 2 * RR) {
            round(xrE, anE, xrO, n, 0);
            if (n + RR >= len) break;                  // (a break, not an `if` around the second round: the back edge keeps its static load count)
            round(xrO, anO, xrE, n + RR, 1);
        }
    }
    if (!active) return;
    // D layout of the 32x32 tile: lane l, register r -> row 8 * (r / 4) + 4 * (l / 32) + r % 4, column l % 32
    const size_t slab = SPLIT ? (size_t)blockIdx.x * 2 + grp : (size_t)blockIdx.x;      // (SPLIT: one slab per wave pair)
    float *pw = partial + slab * cout_pad * Cin;
#pragma unroll
    for (int t = 0; t < TI; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = 32 * wv + 8 * (r >> 2) + 4 * half + (r & 3);
            pw[(size_t)i * Cin + 32 * t + (lane & 31)] = acc[t][r];
        }
    bsum += __shfl_xor(bsum, 32, 64);
    if (half == 0) bpartial[slab * cout_pad + o] = bsum;
}

// Heads with <= 12 outputs (xyz offsets, rotations, scale, opacity): the product is a handful of dot products per input column --
// a streaming read of x (HBM-bound) instead of a 32-row MFMA tile of which 1-3 rows are used (80 us for 128 inputs).
// Thread = one float4 of input columns x one of 256 / (Cin / 4) row phases; fixed-order tree over the phases in LDS.
template <int CO>
__global__ void __launch_bounds__(256)
sg_wgrad_small_kernel(int N, int Cin, const float *__restrict__ dz, const float *__restrict__ x,
                      float *__restrict__ partial, float *__restrict__ bpartial)
{
    __shared__ float4 sAcc[CO][256];
    __shared__ float sB[CO][256];
    const int c4n = Cin >> 2, c4 = threadIdx.x % c4n, ph = threadIdx.x / c4n, nph = 256 / c4n;
    float4 acc[CO];
    float bs[CO];
#pragma unroll
    for (int c = 0; c < CO; c++) { acc[c] = make_float4(0, 0, 0, 0); bs[c] = 0.0f; }
    if (ph < nph) {
        const int stride = gridDim.x * nph;
        int r = blockIdx.x * nph + ph;
        for (; r + 3 * stride < N; r += 4 * stride) {
            float4 xv[4];
            float g[4][CO];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                xv[u] = *(const float4 *)(x + (size_t)(r + u * stride) * Cin + 4 * c4);
#pragma unroll
                for (int c = 0; c < CO; c++) g[u][c] = dz[(size_t)(r + u * stride) * CO + c];
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int c = 0; c < CO; c++) {
                    acc[c].x += g[u][c] * xv[u].x; acc[c].y += g[u][c] * xv[u].y;
                    acc[c].z += g[u][c] * xv[u].z; acc[c].w += g[u][c] * xv[u].w;
                    bs[c] += g[u][c];
                }
        }
        for (; r < N; r += stride) {
            const float4 xv = *(const float4 *)(x + (size_t)r * Cin + 4 * c4);
#pragma unroll
            for (int c = 0; c < CO; c++) {
                const float g = dz[(size_t)r * CO + c];
                acc[c].x += g * xv.x; acc[c].y += g * xv.y; acc[c].z += g * xv.z; acc[c].w += g * xv.w;
                bs[c] += g;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CO; c++) { sAcc[c][threadIdx.x] = acc[c]; sB[c][threadIdx.x] = bs[c]; }
    __syncthreads();
    if (ph == 0) {
#pragma unroll
        for (int c = 0; c < CO; c++) {
            float4 t = make_float4(0, 0, 0, 0);
            for (int q = 0; q < nph; q++) {
                const float4 v = sAcc[c][q * c4n + c4];
                t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
            }
            *(float4 *)(partial + ((size_t)blockIdx.x * CO + c) * Cin + 4 * c4) = t;
            if (c4 == 0) {                                     // every phase saw the same dz rows only once: column 0's copy
                float b = 0.0f;
                for (int q = 0; q < nph; q++) b += sB[c][q * c4n];
                bpartial[(size_t)blockIdx.x * CO + c] = b;
            }
        }
    }
}

// 16 output elements x 16 slices of the per-workgroup partials per 256-thread workgroup (fixed slices, fixed order):
// the sum over <= 256 partials is latency-bound, so it is spread over many short chains
__global__ void __launch_bounds__(256)
sg_wgrad_reduce_kernel(const float *__restrict__ partial, const float *__restrict__ bpartial, int nwg, int Cout, int Cin,
                       int cout_pad, float *__restrict__ dW, float *__restrict__ db)
{
    __shared__ float sS[16][17];
    const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    const int total = Cout * Cin;
    const int per = (nwg + 15) / 16, w0 = sl * per, w1 = min(w0 + per, nwg);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    // sixteen partials per round, every load issued before the first addition (clamped indices, zero weights beyond the slice): with
    // <= 256 workgroups a slice IS one round -- as a 4-at-a-time loop it was four dependent memory round trips, the whole kernel
    if (e < total || (db && e < total + Cout)) {
        const bool isw = e < total;
        const int o = isw ? e / Cin : e - total, c = isw ? e - o * Cin : 0;
        const float *p = isw ? partial + (size_t)o * Cin + c : bpartial + o;
        const size_t st = isw ? (size_t)cout_pad * Cin : (size_t)cout_pad;
        for (int w = w0; w < w1; w += 16) {
            float v[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int wi = w + i < w1 ? w + i : w1 - 1;
                v[i] = p[(size_t)wi * st];
            }
#pragma unroll
            for (int i = 0; i < 16; i += 4) {
                s0 += w + i < w1 ? v[i] : 0.0f; s1 += w + i + 1 < w1 ? v[i + 1] : 0.0f;
                s2 += w + i + 2 < w1 ? v[i + 2] : 0.0f; s3 += w + i + 3 < w1 ? v[i + 3] : 0.0f;
            }
        }
    }
    sS[sl][el] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl == 0) {
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; q++) t += sS[q][el];
        if (e < total) dW[e] = t;
        else if (db && e < total + Cout) db[e - total] = t;
    }
}

// MFMA kernel: ONE workgroup per CU (256 equal row ranges; a range need not be a whole number of rounds -- the rows beyond it read
// as zero).  A wave's TI independent accumulator chains keep its SIMD's matrix core busy on their own, and the partials -- one
// Cout x Cin slab per workgroup, written once and read once by the reduce kernel -- are what more workgroups multiply: 768 / 512 /
// 256 workgroups: 76 / 65 / 59 us for a 128 x 128 layer at 150 k points, of which the reduce is 15 / 11 / 6.
static inline int sg_wg_chunk(int N)
{
    const int c = (N + 255) / 256;
    return c < 32 ? 32 : c;
}
static inline int sg_wg_count(int N) { const int n = (N + SG_WG_ROWS - 1) / SG_WG_ROWS; return n < 512 ? n : 512; }
static inline int sg_wg_count_max(int N) { const int n = 2 * ((N + 31) / 32); return n < 768 ? n : 768; }   // bound over the kernels' slab counts (SPLIT: two per workgroup)
size_t sg_weight_grad_ws_bytes_impl(int N, int Cout, int Cin)
{
    const size_t cp = (size_t)((Cout + 31) / 32) * 32;
    return sg_align((size_t)sg_wg_count_max(N) * cp * Cin * 4) + sg_align((size_t)sg_wg_count_max(N) * cp * 4);
}
int sg_launch_weight_grad(int N, int Cout, int Cin, const float *dz, const float *x, void *ws, float *dW, float *db,
                          hipStream_t st)
{
    if (Cin % 32 != 0 || Cin > 128 || Cout > 128 || Cout < 1) return 1;
    int cp = ((Cout + 31) / 32) * 32;
    int nwg = sg_wg_count(N);
    const int ti = Cin / 32;
    float *partial = (float *)ws;
    float *bpartial = (float *)((char *)ws + sg_align((size_t)sg_wg_count_max(N) * cp * Cin * 4));
    if (Cout <= 12) {
        // (partials are [nwg][Cout][Cin] here: the reduce kernel takes the row pitch as a parameter)
#define SG_WGS(C) case C: hipLaunchKernelGGL(sg_wgrad_small_kernel<C>, dim3(nwg), dim3(256), 0, st, N, Cin, dz, x, partial, bpartial); break
        switch (Cout) {
            SG_WGS(1); SG_WGS(2); SG_WGS(3); SG_WGS(4); SG_WGS(5); SG_WGS(6); SG_WGS(7); SG_WGS(8); SG_WGS(9); SG_WGS(10); SG_WGS(11);
            default: hipLaunchKernelGGL(sg_wgrad_small_kernel<12>, dim3(nwg), dim3(256), 0, st, N, Cin, dz, x, partial, bpartial); break;
        }
#undef SG_WGS
        cp = Cout;
    } else {
        const int chunk = sg_wg_chunk(N);
        nwg = (N + chunk - 1) / chunk;
        const bool split = cp <= 64;                          // two waves own output rows: the other pair shares the round's rows
#define SG_WGK(T)                                                                                                                   \
        do {                                                                                                                        \
            if (split) hipLaunchKernelGGL((sg_wgrad_kernel<T, (T == 4 ? 16 : 32), true>), dim3(nwg), dim3(256), 0, st, N, Cout, Cin, dz, x, partial, bpartial, cp, chunk); \
            else hipLaunchKernelGGL((sg_wgrad_kernel<T, (T == 4 ? 16 : 32), false>), dim3(nwg), dim3(256), 0, st, N, Cout, Cin, dz, x, partial, bpartial, cp, chunk);    \
        } while (0)
        switch (ti) { case 1: SG_WGK(1); break; case 2: SG_WGK(2); break; case 3: SG_WGK(3); break; default: SG_WGK(4); break; }
#undef SG_WGK
        if (split) nwg *= 2;                                  // (slabs for the reduce)
    }
    hipLaunchKernelGGL(sg_wgrad_reduce_kernel, dim3((Cout * Cin + Cout + 15) / 16), dim3(256), 0, st, partial, bpartial, nwg,
                       Cout, Cin, cp, dW, db);
    return 0;
}
