// The zlib streams of n PNG files to the uint8 [F,H,W,4] frame store (sg_unpng_decode; include/sings_unpng.h states the table, the
// statuses and the rules, sings_amd/unpng.py holds the Python restatement).  Two launches, integer arithmetic throughout:
//
//   inflate    one wave per stream.  Every lane runs the decode core of sg_inflate.h on the same bits (inflate is serial within a
//              stream: the parallelism is across streams); the two primitives the core leaves open use the wave.  The last 32 KiB
//              of output live in LDS, a ring: a literal is one LDS byte by lane 0, a copy is LDS to LDS with a lane per byte, and
//              every SG_UNPNG_CHUNK bytes the wave moves what is new to the stream's slot in the workspace, a lane per byte, folding
//              the chunk into the Adler-32 (sum d and sum (n - i) d: chunks combine exactly) and looking at the filter bytes that
//              lie in it.  A copy never reads global memory, so no store to it has to become visible inside the launch.
//   unfilter   one wave per scanline.  The wave of a None / Sub row (or of row 0) rebuilds that row -- Sub: a wave scan modulo 256
//              per channel -- and then walks the Up / Average / Paeth rows below it, in order, two rows in LDS; the waves of those
//              rows return at once.  Average and Paeth run serially inside a row, a lane per channel.  Every rebuilt row is
//              scattered to channels 0..2 (colour) or 3 (mask) of its frame.
#include "sg_host.h"
#include "../../include/sings_unpng.h"

#define SG_INFLATE_UNIFORM(x) sg_unpng_uniform(x)
__host__ __device__ __forceinline__ uint32_t sg_unpng_uniform(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
#else
    return x;
#endif
}
#include "sg_inflate.h"

#define SG_UNPNG_CHUNK 4096u                     // bytes the ring may hold that the workspace does not: far below the ring's 32 768
#define SG_UNPNG_RING_MASK (SG_INFLATE_WINDOW - 1u)
#define SG_UNPNG_ADLER 65521u

__device__ __forceinline__ unsigned long long sg_unpng_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The core's output on the device.  Every lane holds the same pos / flushed / s1 / s2; only `lane` differs.  A store to the ring by
// one lane is read by others only behind a __syncthreads() (one wave per workgroup: a wait for the LDS queue and a compiler fence).
struct SgUnpngOut {
    uint8_t *ring;                               // LDS, SG_INFLATE_WINDOW bytes: byte p of the output at p & SG_UNPNG_RING_MASK
    uint8_t *slot;                               // the stream's slot in the workspace
    uint32_t pos, flushed, s1, s2, line, bad_filter;
    int lane;

    __device__ __forceinline__ void flush()
    {
        __syncthreads();
        const uint32_t n = pos - flushed;        // <= SG_UNPNG_CHUNK + 257
        unsigned long long a = 0, w = 0;
        for (uint32_t i = (uint32_t)lane; i < n; i += 64u) {
            const uint32_t d = ring[(flushed + i) & SG_UNPNG_RING_MASK];
            slot[flushed + i] = (uint8_t)d;
            a += d;
            w += (unsigned long long)(n - i) * d;
        }
        // the filter bytes in [flushed, pos): every `line`-th byte of the output
        for (uint32_t p = (flushed + line - 1u) / line * line + (uint32_t)lane * line; p < pos; p += 64u * line)
            if (ring[p & SG_UNPNG_RING_MASK] > 4) bad_filter = 1u;
        a = sg_unpng_wave_sum(a);
        w = sg_unpng_wave_sum(w);
        s2 = (uint32_t)(((unsigned long long)s2 + (unsigned long long)n * s1 + w) % SG_UNPNG_ADLER);
        s1 = (uint32_t)(((unsigned long long)s1 + a) % SG_UNPNG_ADLER);
        flushed = pos;
        __syncthreads();
    }
    __device__ __forceinline__ void literal(uint8_t b)
    {
        if (lane == 0) ring[pos & SG_UNPNG_RING_MASK] = b;
        pos++;
        if (pos - flushed >= SG_UNPNG_CHUNK) flush();
    }
    // Every byte of a copy is one of the `dist` bytes in front of pos: byte i is byte i % dist of them.  All of a round's loads come
    // before its stores, and nothing a round stores is loaded by a later one except through the ring's wrap, in program order.
    __device__ __forceinline__ void copy(uint32_t dist, uint32_t len)
    {
        __syncthreads();
        const uint32_t from = pos - dist;
        for (uint32_t i = (uint32_t)lane; i < len; i += 64u) {
            const uint32_t j = i < dist ? i : i % dist;
            ring[(pos + i) & SG_UNPNG_RING_MASK] = ring[(from + j) & SG_UNPNG_RING_MASK];
        }
        pos += len;
        if (pos - flushed >= SG_UNPNG_CHUNK) flush();
    }
    __device__ __forceinline__ uint32_t adler()
    {
        flush();
        return s2 << 16 | s1;
    }
};

// grid: n, one wave each.  ONE WAVE PER WORKGROUP IS A PRECONDITION, not a tuning choice: all 64 lanes run the core on the shared
// `tabs` (sg_inflate_build's count[..]++ and next[len]++, the code-length reader's lens[at++]) with plain LDS read-modify-writes.
// That is only right because the lanes of one wave step together and every lane stores the value every other lane stores; a second
// wave in the workgroup would interleave its own updates with them.  __launch_bounds__(64) caps the block but does not fix it:
// the dim3(64) of the launch in sg_unpng_decode does, and the two must change together (with lane 0 building the tables behind a
// barrier, or tables per wave, if a workgroup ever holds more than one).
__global__ void __launch_bounds__(64)
sg_unpng_inflate_kernel(const uint8_t *__restrict__ streams, const long long *__restrict__ table, uint8_t *__restrict__ ws, size_t pitch,
                        int F, int H, int W, int32_t *__restrict__ status)
{
    __shared__ uint8_t ring[SG_INFLATE_WINDOW];
    __shared__ SgInflateTables tabs;
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x;
    const long long *row = table + s * SG_UNPNG_TABLE_COLS;
    const long long off = row[SG_UNPNG_T_OFFSET], len = row[SG_UNPNG_T_LENGTH], w = row[SG_UNPNG_T_WIDTH], h = row[SG_UNPNG_T_HEIGHT];
    const long long ch = row[SG_UNPNG_T_CHANNELS], dest = row[SG_UNPNG_T_DEST];
    int st = 0;
    if (off < 0 || len < 0 || (ch != 1 && ch != 3 && ch != 4) || w < 1 || h < 1 || w > SG_UNPNG_MAX_ROW_BYTES ||
        w * ch > SG_UNPNG_MAX_ROW_BYTES || h > SG_UNPNG_MAX_HEIGHT || dest < 0 || (dest >> 2) >= (long long)F ||
        (dest & 3) != (ch == 1 ? 3 : 0))
        st = SG_UNPNG_E_TABLE;
    else if (w != (long long)W || h != (long long)H)
        st = SG_UNPNG_E_SIZE;
    else if ((unsigned long long)(h * (1 + w * ch)) > (unsigned long long)pitch)
        st = SG_UNPNG_E_WORKSPACE;
    if (st == 0) {
        SgUnpngOut out = {ring, ws + s * pitch, 0u, 0u, 1u, 0u, (uint32_t)(1 + w * ch), 0u, lane};
        st = sg_inflate(streams + off, (size_t)len, (size_t)(h * (1 + w * ch)), tabs, out);
        if (st == 0 && __any((int)out.bad_filter)) st = SG_UNPNG_E_FILTER;
    }
    if (lane == 0) status[s] = st;
}

__device__ __forceinline__ int sg_unpng_paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// grid: (H, n), one wave each; dynamic LDS: two rows of `row_pitch` >= 4 W bytes
extern __shared__ uint8_t sg_unpng_rows[];
__global__ void __launch_bounds__(64)
sg_unpng_unfilter_kernel(const long long *__restrict__ table, const uint8_t *__restrict__ ws, size_t pitch, uint8_t *__restrict__ dst,
                         int H, int W, int row_pitch, const int32_t *__restrict__ status)
{
    const int lane = threadIdx.x, y = blockIdx.x;
    const size_t s = blockIdx.y;
    if (status[s] != 0) return;                                   // a failed stream writes nothing
    const int ch = (int)table[s * SG_UNPNG_TABLE_COLS + SG_UNPNG_T_CHANNELS];
    const size_t frame = (size_t)(table[s * SG_UNPNG_TABLE_COLS + SG_UNPNG_T_DEST] >> 2);
    const int nb = W * ch, L = nb + 1;                            // (1 <= nb <= SG_UNPNG_MAX_ROW_BYTES, H L <= pitch: the inflate kernel's checks)
    const uint8_t *raw = ws + s * pitch;
    int type = raw[(size_t)y * (size_t)L];
    if (type > 4 || (y > 0 && type >= 2)) return;                 // a link of the chain the wave of a row above walks
    int cur = 0;
    if (type >= 2) {
        for (int i = lane; i < nb; i += 64) sg_unpng_rows[row_pitch + i] = 0;       // the row above the first
    }
    for (int r = y;;) {
        uint8_t *out = sg_unpng_rows + cur * row_pitch;
        const uint8_t *prev = sg_unpng_rows + (cur ^ 1) * row_pitch, *line = raw + (size_t)r * (size_t)L + 1;
        for (int i = lane; i < nb; i += 64) out[i] = line[i];
        __syncthreads();
        if (type == 1) {
            for (int c = 0; c < ch; c++) {
                uint32_t carry = 0;
                for (int base = 0; base < W; base += 64) {
                    const int p = base + lane;
                    uint32_t v = p < W ? out[p * ch + c] : 0u;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t t = __shfl_up(v, d, 64);
                        if (lane >= d) v += t;
                    }
                    v = (v + carry) & 255u;
                    if (p < W) out[p * ch + c] = (uint8_t)v;
                    carry = __shfl(v, 63, 64);
                }
            }
        } else if (type == 2) {
            for (int i = lane; i < nb; i += 64) out[i] = (uint8_t)(out[i] + prev[i]);
        } else if (type >= 3 && lane < ch) {
            int a = 0, c = 0;
            for (int i = lane; i < nb; i += ch) {
                const int b = prev[i];
                a = (out[i] + (type == 3 ? (a + b) >> 1 : sg_unpng_paeth(a, b, c))) & 255;
                out[i] = (uint8_t)a;
                c = b;
            }
        }
        __syncthreads();
        uint8_t *px = dst + ((frame * (size_t)H + (size_t)r) * (size_t)W) * 4;
        if (ch == 1) {
            for (int p = lane; p < W; p += 64) px[(size_t)p * 4 + 3] = out[p];
        } else {
            for (int p = lane; p < W; p += 64) {
                px[(size_t)p * 4] = out[p * ch];
                px[(size_t)p * 4 + 1] = out[p * ch + 1];
                px[(size_t)p * 4 + 2] = out[p * ch + 2];
            }
        }
        if (++r >= H) break;
        type = raw[(size_t)r * (size_t)L];
        if (type < 2 || type > 4) break;                          // the next head: its own wave's
        cur ^= 1;
        __syncthreads();
    }
}

// ---- the boundary
extern "C" int sg_unpng_layout(int n_streams, size_t max_raw_bytes, size_t out[SG_UNPNG_LAYOUT_WORDS])
{
    const char *who = "sg_unpng_layout";
    if (!out) return sg_failf("%s: null pointer", who);
    if (n_streams < 1 || n_streams > SG_UNPNG_MAX_STREAMS) return sg_failf("%s: n_streams = %d, 1..%d per call", who, n_streams, SG_UNPNG_MAX_STREAMS);
    if (max_raw_bytes < 1 || max_raw_bytes >= ((size_t)1 << 40) / (size_t)n_streams)
        return sg_failf("%s: max_raw_bytes = %llu for %d streams, a workspace of 1..2^40 - 1 bytes", who, (unsigned long long)max_raw_bytes, n_streams);
    const size_t pitch = (max_raw_bytes + 15) & ~(size_t)15;
    out[SG_UNPNG_L_WS_BYTES] = pitch * (size_t)n_streams;
    out[SG_UNPNG_L_SLOT_PITCH] = pitch;
    return 0;
}

extern "C" int sg_unpng_decode(int n, const uint8_t *streams, const int64_t *table, void *ws, size_t ws_bytes, uint8_t *dst, int F, int H,
                               int W, int32_t *status, void *stream)
{
    const char *who = "sg_unpng_decode";
    if (!streams || !table || !ws || !dst || !status) return sg_failf("%s: null pointer", who);
    if (n < 1 || n > SG_UNPNG_MAX_STREAMS) return sg_failf("%s: n = %d streams, 1..%d per call", who, n, SG_UNPNG_MAX_STREAMS);
    if (F < 1 || H < 1 || H > SG_UNPNG_MAX_HEIGHT || W < 1 || 4 * (long long)W > SG_UNPNG_MAX_ROW_BYTES)
        return sg_failf("%s: a store of %d frames of %d x %d pixels, 1..%d wide and 1..%d high", who, F, W, H, SG_UNPNG_MAX_ROW_BYTES / 4,
                        SG_UNPNG_MAX_HEIGHT);
    if ((unsigned long long)F * (unsigned long long)H * (unsigned long long)W >= (1ull << 40))
        return sg_failf("%s: a store of %d x %d x %d pixels, fewer than 2^40", who, F, H, W);
    const size_t pitch = (ws_bytes / (size_t)n) & ~(size_t)15;
    if (pitch < 16) return sg_failf("%s: a workspace of %llu bytes for %d streams, at least 16 each", who, (unsigned long long)ws_bytes, n);
    if ((uintptr_t)ws & 15) return sg_failf("%s: the workspace must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const long long *tab = (const long long *)table;
    // dim3(64): exactly one wave per workgroup -- what sg_unpng_inflate_kernel's use of its shared tables rests on (see there)
    hipLaunchKernelGGL(sg_unpng_inflate_kernel, dim3((unsigned)n), dim3(64), 0, st, streams, tab, (uint8_t *)ws, pitch, F, H, W, status);
    const int row_pitch = (4 * W + 15) & ~15;                     // <= SG_UNPNG_MAX_ROW_BYTES: 32 KiB of LDS at the most
    hipLaunchKernelGGL(sg_unpng_unfilter_kernel, dim3((unsigned)H, (unsigned)n), dim3(64), 2 * (size_t)row_pitch, st, tab,
                       (const uint8_t *)ws, pitch, dst, H, W, row_pitch, status);
    return sg_launched(who);
}
