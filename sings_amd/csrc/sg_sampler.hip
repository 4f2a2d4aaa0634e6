// The corners of the LPIPS patches, drawn on the device (include/sings_sampler.h states the rule; sings_amd/patch_sampler.py
// origins_host is its numpy twin).  Two launches: count the valid positions of the crop per chunk, then one workgroup per frame
// scans the counts, draws the ranks and finds each rank's position by reading its one chunk again.  Integers only, plain stores,
// no spin between workgroups: two calls with the same state give the same bits.
#include "sg_host.h"
#include "../../include/sings_sampler.h"
#include "sg_philox.h"

#define SP_BLOCK 256
#define SP_WAVES (SP_BLOCK / SG_WAVE)
#define SP_STEP 64                       // ballots per step of a wave's rescan: SP_STEP * 64 positions, their loads in flight together
#define SP_SEARCH 8                      // tiles of 64 prefix sums per step of a wave's search, their loads in flight together

// A dependent round trip to memory is what these kernels wait for (about 2 us each in the kernel trace, LAB "Patch sampler"), so
// every batch of loads is issued before the first of them is used: no branch and no division between two loads of a batch.

// (row, col) of q + d in a crop Wc columns wide, for d = dq Wc + dr with dr < Wc
__device__ __forceinline__ void sp_advance(uint32_t &row, uint32_t &col, uint32_t dq, uint32_t dr, uint32_t Wc)
{
    row += dq;
    col += dr;
    if (col >= Wc) { col -= Wc; row += 1u; }
}

// the mask at crop position (row, col) of a full image W wide with margin o; behind the crop's end (!inside): at position 0, a load
// that is in bounds and that the caller does not count.  Valid is > 0 (a NaN is not).
__device__ __forceinline__ float sp_load(const float *__restrict__ m, int W, int o, uint32_t row, uint32_t col, bool inside)
{
    return m[inside ? (size_t)(o + row) * W + o + col : (size_t)o * W + o];
}

// cnt[k][c] = valid positions among [c SG_PATCH_CHUNK, (c + 1) SG_PATCH_CHUNK) of frame k's crop.  Workgroup (0,0) moves the counter.
__global__ void __launch_bounds__(SP_BLOCK)
sg_patch_count_kernel(int W, int o, uint32_t Wc, uint32_t total, size_t mask_stride, const float *__restrict__ mask,
                      int64_t *__restrict__ state, uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t sC[SP_WAVES];
    const float *m = mask + blockIdx.y * mask_stride;
    const uint32_t q0 = blockIdx.x * SG_PATCH_CHUNK + threadIdx.x, dq = SP_BLOCK / Wc, dr = SP_BLOCK % Wc;
    uint32_t row = q0 / Wc, col = q0 % Wc, c = 0;
    float f[SG_PATCH_CHUNK / SP_BLOCK];
#pragma unroll
    for (int it = 0; it < SG_PATCH_CHUNK / SP_BLOCK; it++) {
        f[it] = sp_load(m, W, o, row, col, q0 + it * SP_BLOCK < total);
        sp_advance(row, col, dq, dr, Wc);
    }
#pragma unroll
    for (int it = 0; it < SG_PATCH_CHUNK / SP_BLOCK; it++)                       // (the wave's count, in every lane)
        c += (uint32_t)__popcll(__ballot(q0 + it * SP_BLOCK < total && f[it] > 0.0f));
    if ((threadIdx.x & (SG_WAVE - 1)) == 0) sC[threadIdx.x / SG_WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < SP_WAVES; w++) s += sC[w];
        cnt[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
        if (blockIdx.x == 0 && blockIdx.y == 0) {                                // this call's counter, and the next call's
            const int64_t c0 = state[0];
            state[1] = c0;
            state[0] = (int64_t)((uint64_t)c0 + 1u);
        }
    }
}

// One workgroup per frame.  pre: the frame's chunk counts, turned into their exclusive prefix sums in place.
__global__ void __launch_bounds__(SP_BLOCK)
sg_patch_pick_kernel(int H, int W, int P, int n, uint32_t nch, uint32_t total, uint64_t thr, size_t mask_stride,
                     const float *__restrict__ mask, int64_t *__restrict__ state, uint32_t *ws, int32_t *__restrict__ origins,
                     int32_t *__restrict__ info)
{
    __shared__ uint32_t sW[SP_WAVES], sRank[SG_PATCH_MAX_N];
    __shared__ int sBranch;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & (SG_WAVE - 1), wave = tid / SG_WAVE;
    const int o = P / 2;
    const uint32_t Wc = (uint32_t)(W - P);
    const float *m = mask + k * mask_stride;
    uint32_t *pre = ws + (size_t)k * nch;
    int32_t *org = origins + (size_t)k * n * 2;
    const uint64_t seed = (uint64_t)state[2], counter = (uint64_t)state[1];      // (asked for first: they arrive during the scan)

    // ---- exclusive scan of the chunk counts, SP_BLOCK at a time
    uint32_t M = 0;
    for (uint32_t base = 0; base < nch; base += SP_BLOCK) {
        const uint32_t i = base + tid, c = i < nch ? pre[i] : 0u;
        uint32_t x = c;
#pragma unroll
        for (int d = 1; d < SG_WAVE; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, SG_WAVE);
            if (lane >= d) x += y;
        }
        if (lane == SG_WAVE - 1) sW[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < SP_WAVES; w++) { before += w < wave ? sW[w] : 0u; all += sW[w]; }
        if (i < nch) pre[i] = M + before + x - c;
        M += all;
        __syncthreads();
    }

    // ---- the branch and the ranks (thread 0; a handful of Philox blocks)
    if (tid == 0) {
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        uint32_t ctr[4] = { (uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)k, 0u }, w[4];
        uint32_t block = 0;
        sg_philox4x32(ctr, k0, k1, w);
        auto word = [&](uint32_t t) {
            if (t / 4 != block) { block = t / 4; ctr[3] = block; sg_philox4x32(ctr, k0, k1, w); }
            return w[t % 4];
        };
        // (the draw first, as in the reference: a frame counts as forced only where np.random.choice would have raised)
        const int branch = (uint64_t)word(0) >= thr ? SG_PATCH_BRANCH_UNIFORM : M < (uint32_t)n ? SG_PATCH_BRANCH_FORCED : SG_PATCH_BRANCH_MASKED;
        if (branch == SG_PATCH_BRANCH_MASKED) {
            for (int i = 0; i < n; i++) {                                        // Floyd: n distinct ranks of [0, M)
                const uint32_t j = M - (uint32_t)n + (uint32_t)i;
                uint32_t t = sg_bounded(word(1u + i), j + 1u);
                for (int e = 0; e < i; e++)
                    if (sRank[e] == t) { t = j; break; }
                sRank[i] = t;
            }
        } else {
            for (int i = 0; i < n; i++) {
                org[2 * i] = (int32_t)sg_bounded(word(1u + 2u * i), (uint32_t)(H - P));
                org[2 * i + 1] = (int32_t)sg_bounded(word(2u + 2u * i), (uint32_t)(W - P));
            }
        }
        sBranch = branch;
        info[2 * k] = (int32_t)M;
        info[2 * k + 1] = branch;
        if (branch == SG_PATCH_BRANCH_FORCED) atomicAdd((unsigned long long *)&state[3], 1ull);      // (nothing reads the old value)
    }
    __syncthreads();                                                             // (and pre[] is visible to the whole workgroup)
    if (sBranch != SG_PATCH_BRANCH_MASKED) return;

    // ---- a wave per rank: the chunk that holds it, then the position inside that chunk
    const uint32_t dq = SG_WAVE / Wc, dr = SG_WAVE % Wc;
    for (int i = wave; i < n; i += SP_WAVES) {
        const uint32_t t = sRank[i];
        // the prefix sums do not decrease and pre[0] = 0: those <= t are the first `le` of them, and chunk c = le - 1 holds rank t
        uint32_t le = 0, before = 0;                                             // before: pre[c]
        for (uint32_t base = 0; base < nch; base += SP_SEARCH * SG_WAVE) {
            uint32_t p[SP_SEARCH];
#pragma unroll
            for (int u = 0; u < SP_SEARCH; u++) {
                const uint32_t j = base + u * SG_WAVE + lane;
                p[u] = pre[j < nch ? j : nch - 1u];
            }
#pragma unroll
            for (int u = 0; u < SP_SEARCH; u++) {
                const uint32_t j = base + u * SG_WAVE + lane;
                const uint32_t here = (uint32_t)__popcll(__ballot(j < nch && p[u] <= t));        // (the tile's first `here` lanes)
                if (here) before = __shfl(p[u], (int)here - 1, SG_WAVE);
                le += here;
            }
        }
        const uint32_t c = le - 1u, r = t - before;                              // rank r among the valid positions of chunk c
        const uint32_t q0 = c * SG_PATCH_CHUNK + lane;
        uint32_t row = q0 / Wc, col = q0 % Wc, seen = 0, found = 0xffffffffu;
        for (int step = 0; step < SG_PATCH_CHUNK / (SP_STEP * SG_WAVE); step++) {
            const uint32_t qs = q0 + step * SP_STEP * SG_WAVE;
            float f[SP_STEP];
#pragma unroll
            for (int s = 0; s < SP_STEP; s++) {
                f[s] = sp_load(m, W, o, row, col, qs + s * SG_WAVE < total);
                sp_advance(row, col, dq, dr, Wc);
            }
#pragma unroll
            for (int s = 0; s < SP_STEP; s++) {
                unsigned long long b = __ballot(qs + s * SG_WAVE < total && f[s] > 0.0f);
                const uint32_t here = (uint32_t)__popcll(b);
                if (found == 0xffffffffu && r < seen + here) {
                    for (uint32_t e = seen; e < r; e++) b &= b - 1ull;           // drop the r - seen lowest set bits
                    found = qs - lane + (uint32_t)s * SG_WAVE + (uint32_t)(__ffsll((long long)b) - 1);
                }
                seen += here;
            }
        }
        if (found == 0xffffffffu) found = 0u;                                    // (cannot happen: the counts are of this mask)
        if (lane == 0) {
            org[2 * i] = (int32_t)(found / Wc);
            org[2 * i + 1] = (int32_t)(found % Wc);
        }
    }
}

static inline uint32_t sp_chunks(int H, int W, int P)
{
    const uint64_t total = (uint64_t)(H - P) * (uint64_t)(W - P);
    return (uint32_t)((total + SG_PATCH_CHUNK - 1) / SG_PATCH_CHUNK);
}

static inline bool sp_size_ok(int K, int H, int W, int P)
{
    return K >= 1 && K <= 65535 && P >= 2 && P % 2 == 0 && H > P && W > P && (uint64_t)H * (uint64_t)W < (1ull << 31);
}

extern "C" size_t sg_patch_sampler_ws_bytes(int K, int H, int W, int P)
{
    return sp_size_ok(K, H, W, P) ? (size_t)K * sp_chunks(H, W, P) * sizeof(uint32_t) : 0;
}

extern "C" int sg_patch_origins(int K, int H, int W, int P, int n, int mask_stride, float ratio_mask, const float *mask,
                                int64_t *state, void *ws, int32_t *origins, int32_t *info, void *stream)
{
    const char *who = "sg_patch_origins";
    if (K < 1 || K > 65535) return sg_failf("%s: K = %d outside 1..65535", who, K);
    if (n < 1 || n > SG_PATCH_MAX_N) return sg_failf("%s: n = %d outside 1..%d", who, n, SG_PATCH_MAX_N);
    if (P < 2 || P % 2) return sg_failf("%s: patch size %d must be even and at least 2", who, P);
    if (H <= P || W <= P) return sg_failf("%s: a %d x %d image has no room for a patch of %d", who, H, W, P);
    if ((uint64_t)H * (uint64_t)W >= (1ull << 31)) return sg_failf("%s: a %d x %d image has 2^31 pixels or more", who, H, W);
    if (mask_stride != 0 && mask_stride != H * W)
        return sg_failf("%s: mask_stride %d is neither 0 nor H*W = %d", who, mask_stride, H * W);
    if (!mask || !state || !ws || !origins || !info) return sg_failf("%s: null pointer", who);
    const double r = (double)ratio_mask;                                         // (a NaN: never the masked branch)
    const uint64_t thr = r >= 1.0 ? (1ull << 32) : r > 0.0 ? (uint64_t)(r * 4294967296.0) : 0ull;
    const uint32_t nch = sp_chunks(H, W, P), total = (uint32_t)(H - P) * (uint32_t)(W - P);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_patch_count_kernel, dim3(nch, K), dim3(SP_BLOCK), 0, st, W, P / 2, (uint32_t)(W - P), total,
                       (size_t)mask_stride, mask, state, (uint32_t *)ws);
    hipLaunchKernelGGL(sg_patch_pick_kernel, dim3(K), dim3(SP_BLOCK), 0, st, H, W, P, n, nch, total, thr, (size_t)mask_stride, mask,
                       state, (uint32_t *)ws, origins, info);
    return sg_launched(who);
}
