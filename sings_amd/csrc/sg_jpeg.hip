// K uint8 frames to K baseline JPEG files (sg_jpeg_encode_frames; include/sings_jpeg.h states the stream, the pinned arithmetic and
// the table layout, sings_amd/video.py holds the numpy restatement the bytes are tested against).  Three stages, four launches:
//
//   block pass    one wave per 8 x 8 pixel block (a workgroup: four blocks side by side, 96 contiguous bytes per pixel row): colour
//                 conversion, the two DCT passes through LDS, quantisation; int16 coefficients in zig-zag order to the workspace.
//   entropy pass  one wave per restart segment, 64 coefficient blocks (a lane each) per round: a lane counts its block's bits, a
//                 wave scan places them, the lanes OR their codes into LDS words (integer atomics on LDS, nothing else: the result
//                 does not depend on their order), and the round's complete words leave for the segment's slot with a second scan
//                 over their 0xFF bytes for the stuffing.  The partial last word is carried into the next round.
//   gather pass   per frame a scan of the segments' byte counts (sizes[k], or -needed), then one workgroup per segment copies its
//                 slot behind the header, followed by its RST marker or EOI.  A frame that does not fit writes nothing.
//
// The restart segments are what makes the entropy stage parallel: a segment starts byte-aligned with its DC predictors at 0.
#include "sg_codec.h"
#include "../../include/sings_jpeg.h"

#define SG_JPEG_BLOCK_WAVES 4
#define SG_JPEG_BLOCK_BITS 1664                  // >= 22 (DC: an 11-bit code, 11 bits) + 63 * 26 (AC: a 16-bit code, 10 bits)
#define SG_JPEG_LDS_WORDS 3336                   // > (31 carried bits + 64 blocks * 1664) / 32 + the word a code may spill into
#define SG_JPEG_T_BASIS 0
#define SG_JPEG_T_QUANT 64
#define SG_JPEG_T_ZIGZAG 192
#define SG_JPEG_T_HUFF 256

// ---- block pass.  grid: (ceil(nbx / 4), nby, K); wave w of a workgroup: block column 4 blockIdx.x + w; lane: pixel (y, x) = (lane >> 3,
// lane & 7) for the colour conversion, output (y, u) of the row pass, coefficient (v, u) of the column pass.
__global__ void __launch_bounds__(64 * SG_JPEG_BLOCK_WAVES)
sg_jpeg_block_kernel(int W, int H, int nbx, int bgr, const uint8_t *__restrict__ frames, const uint32_t *__restrict__ tables,
                     int16_t *__restrict__ coef)
{
    __shared__ float sm[SG_JPEG_BLOCK_WAVES][4][64];              // per wave: the samples of Y, Cb, Cr; the row pass's result
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bx = blockIdx.x * SG_JPEG_BLOCK_WAVES + wave, by = blockIdx.y, k = blockIdx.z;
    const bool active = bx < nbx;
    const int hi = lane >> 3, lo = lane & 7;
    // edge replication: the last column / row repeats (an inactive wave reads the frame's last block column and stores nothing)
    const int px = min((active ? bx : nbx - 1) * 8 + lo, W - 1), py = min(by * 8 + hi, H - 1);
    const uint8_t *p = frames + (((size_t)k * (size_t)H + (size_t)py) * (size_t)W + (size_t)px) * 3;
    const float c0 = (float)p[0], G = (float)p[1], c2 = (float)p[2];
    const float R = bgr ? c2 : c0, B = bgr ? c0 : c2;
    sm[wave][0][lane] = ((0.299f * R + 0.587f * G) + 0.114f * B) - 128.0f;
    sm[wave][1][lane] = ((-0.168736f * R) + (-0.331264f * G)) + 0.5f * B;
    sm[wave][2][lane] = (0.5f * R + (-0.418688f * G)) + (-0.081312f * B);
    const float *basis = (const float *)(tables + SG_JPEG_T_BASIS);
    float cu[8], cv[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { cu[i] = basis[lo * 8 + i]; cv[i] = basis[hi * 8 + i]; }
    const int zz = (int)tables[SG_JPEG_T_ZIGZAG + lane];
    int16_t *dst = coef + ((size_t)k * (size_t)gridDim.y * (size_t)nbx + (size_t)by * (size_t)nbx + (size_t)(active ? bx : 0)) * 192;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *s = sm[wave][c] + hi * 8;
        float t = cu[0] * s[0];
#pragma unroll
        for (int i = 1; i < 8; i++) t = t + cu[i] * s[i];
        sm[wave][3][lane] = t;
        __syncthreads();
        const float *tt = sm[wave][3] + lo;
        float F = cv[0] * tt[0];
#pragma unroll
        for (int i = 1; i < 8; i++) F = F + cv[i] * tt[8 * i];
        __syncthreads();
        const float Q = ((const float *)(tables + SG_JPEG_T_QUANT))[(c ? 64 : 0) + lane];
        float q = rintf(F / Q);                                   // ties to even
        q = fminf(fmaxf(q, lane == 0 ? -1024.0f : -1023.0f), 1023.0f);
        if (active) dst[c * 64 + zz] = (int16_t)(int)q;
    }
}

// ---- entropy pass
__device__ __forceinline__ uint32_t sg_wave_scan(uint32_t v, int lane)       // inclusive
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// A lane's writer into the round's bit buffer: bit p of the round is bit 31 - p % 32 of word p / 32.  Codes of one lane arrive in
// ascending position, so the word in progress is kept in a register and ORed into LDS when the lane moves on.
struct SgBitWriter {
    uint32_t *words;
    uint32_t w, acc;
    __device__ __forceinline__ void flush() { if (acc && w < SG_JPEG_LDS_WORDS) atomicOr(&words[w], acc); }
    __device__ __forceinline__ void put(uint32_t p, uint32_t val, uint32_t n)         // n in 1..32 bits of val
    {
        const uint32_t W = p >> 5, sh = p & 31u;
        if (n == 0u) return;
        if (W != w) { flush(); w = W; acc = 0u; }
        const uint64_t v = (uint64_t)val << (64u - n - sh);
        acc |= (uint32_t)(v >> 32);
        if (n + sh > 32u) { flush(); w = W + 1u; acc = (uint32_t)v; }
    }
};

// One coefficient block (c: 64 int16 in zig-zag order, two per word) with DC predictor `pred` through the Huffman tables of its
// class (`huff`: 16 DC categories, then 256 AC symbols, code << 8 | length) -> its bits; with EMIT they go to `bw` from bit `p` on.
template <bool EMIT>
__device__ __forceinline__ uint32_t sg_jpeg_code_block(const uint32_t (&c)[32], int pred, const uint32_t *huff, SgBitWriter &bw, uint32_t p)
{
    uint32_t bits = 0;
    auto symbol = [&](uint32_t entry, int v, uint32_t n) {       // a code, then the n magnitude bits of v (one's complement below 0)
        const uint32_t len = entry & 255u, total = len + n;
        if (EMIT) {
            const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
            bw.put(p + bits, (entry >> 8) << n | mag, total);
        }
        bits += total;
    };
    {
        const int d = (int)(int16_t)(c[0] & 0xFFFFu) - pred;
        const uint32_t n = d ? 32u - (uint32_t)__clz(d < 0 ? -d : d) : 0u;
        symbol(huff[n], d, n);
    }
    uint32_t run = 0;
#pragma unroll
    for (int i = 1; i < 64; i++) {
        const int v = (int)(int16_t)((c[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu);
        if (v == 0) { run++; continue; }
        for (; run >= 16u; run -= 16u) symbol(huff[16 + 0xF0], 0, 0u);        // ZRL
        const uint32_t n = 32u - (uint32_t)__clz(v < 0 ? -v : v);
        symbol(huff[16 + (run << 4 | n)], v, n);
        run = 0;
    }
    if (run) symbol(huff[16 + 0x00], 0, 0u);                     // EOB (none when coefficient 63 is not zero)
    return bits;
}

// grid: (segments, K), one wave each
__global__ void __launch_bounds__(64)
sg_jpeg_entropy_kernel(int nmcu, int ri, size_t pitch, const uint32_t *__restrict__ tables, const int16_t *__restrict__ coef,
                       uint8_t *__restrict__ slots, uint32_t *__restrict__ seg_bytes)
{
    __shared__ uint32_t huff[2 * SG_JPEG_HUFF_STRIDE];
    __shared__ uint32_t words[SG_JPEG_LDS_WORDS];
    const int lane = threadIdx.x, s = blockIdx.x, k = blockIdx.y, nseg = gridDim.x;
    const int mcu0 = s * ri, nb = 3 * min(ri, nmcu - mcu0);
    const int16_t *cbase = coef + ((size_t)k * (size_t)nmcu + (size_t)mcu0) * 192;
    uint8_t *slot = slots + ((size_t)k * (size_t)nseg + (size_t)s) * pitch;
    for (int i = lane; i < 2 * SG_JPEG_HUFF_STRIDE; i += 64) huff[i] = tables[SG_JPEG_T_HUFF + i];
    if (lane == 0) words[0] = 0u;
    __syncthreads();
    uint32_t carry = 0;                                           // bits of words[0] the last round left (< 32)
    size_t out = 0;                                               // bytes of the slot written
    auto store = [&](size_t o, uint32_t byte) { if (o < pitch) slot[o] = (uint8_t)byte; };       // (the pitch is the worst case)

    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;
        const bool has = b < nb;
        uint32_t c[32];
        if (has) {
            const uint4 *src = (const uint4 *)(cbase + (size_t)b * 64);
#pragma unroll
            for (int i = 0; i < 8; i++) { const uint4 q = src[i]; c[4 * i] = q.x; c[4 * i + 1] = q.y; c[4 * i + 2] = q.z; c[4 * i + 3] = q.w; }
        } else {
#pragma unroll
            for (int i = 0; i < 32; i++) c[i] = 0u;
        }
        // the previous block of the same component in this segment (blocks go Y, Cb, Cr per MCU)
        const int pred = has && b >= 3 ? (int)cbase[(size_t)(b - 3) * 64] : 0;
        const uint32_t *h = huff + (b % 3 ? SG_JPEG_HUFF_STRIDE : 0);
        SgBitWriter bw = {words, 0u, 0u};
        const uint32_t n = has ? sg_jpeg_code_block<false>(c, pred, h, bw, 0u) : 0u;
        const uint32_t incl = sg_wave_scan(n, lane);
        const uint32_t total = carry + __shfl(incl, 63, 64);
        const uint32_t nwords = (total + 31u) >> 5;
        for (uint32_t w = 1u + lane; w <= nwords && w < SG_JPEG_LDS_WORDS; w += 64u) words[w] = 0u;
        __syncthreads();
        if (has) {
            sg_jpeg_code_block<true>(c, pred, h, bw, carry + incl - n);
            bw.flush();
        }
        __syncthreads();
        // the complete words leave, 64 per step, every 0xFF followed by 0x00
        const uint32_t full = total >> 5;
        for (uint32_t w0 = 0; w0 < full; w0 += 64u) {
            const uint32_t w = w0 + lane;
            const bool mine = w < full && w < SG_JPEG_LDS_WORDS;
            const uint32_t word = mine ? words[w] : 0u;
            uint32_t ff = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) ff += ((word >> (24 - 8 * j)) & 255u) == 255u ? 1u : 0u;
            const uint32_t iff = sg_wave_scan(ff, lane);
            if (mine) {
                size_t o = out + 4u * (size_t)lane + (size_t)(iff - ff);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t byte = (word >> (24 - 8 * j)) & 255u;
                    store(o++, byte);
                    if (byte == 255u) store(o++, 0u);
                }
            }
            const uint32_t step = full - w0 < 64u ? full - w0 : 64u;
            out += 4u * (size_t)step + (size_t)__shfl(iff, 63, 64);
        }
        const uint32_t rest = full < SG_JPEG_LDS_WORDS ? words[full] : 0u;       // (zero when the round ended on a word boundary)
        carry = total & 31u;
        __syncthreads();
        if (lane == 0) words[0] = rest;
        __syncthreads();
    }
    if (lane == 0) {
        if (carry) {                                              // the last byte is padded with 1-bits
            const uint32_t word = words[0] | (0xFFFFFFFFu >> carry);
            const uint32_t nbytes = (carry + 7u) >> 3;
            for (uint32_t j = 0; j < nbytes; j++) {
                const uint32_t byte = (word >> (24 - 8 * j)) & 255u;
                store(out++, byte);
                if (byte == 255u) store(out++, 0u);
            }
        }
        seg_bytes[(size_t)k * (size_t)nseg + (size_t)s] = (uint32_t)out;
    }
}

// ---- gather pass.  grid: K; where every segment of frame k starts in its file, and the file's size.
__global__ void __launch_bounds__(256)
sg_jpeg_scan_kernel(int nseg, int header_bytes, size_t capacity, const uint32_t *__restrict__ seg_bytes, uint32_t *__restrict__ seg_off,
                    int32_t *__restrict__ sizes)
{
    __shared__ uint32_t sm[256];
    const int k = blockIdx.x;
    // a segment, then its RST marker / EOI (the end is < 2^31 with every segment at its worst: refused otherwise)
    const uint32_t running = (uint32_t)sg_codec_segment_offsets(k, nseg, 2u, header_bytes, seg_bytes, seg_off, sm);
    if (threadIdx.x == 0) sizes[k] = (size_t)running <= capacity ? (int32_t)running : -(int32_t)running;
}

// grid: (segments, K)
__global__ void __launch_bounds__(256)
sg_jpeg_gather_kernel(size_t pitch, int header_bytes, size_t capacity, const uint8_t *__restrict__ header, const uint8_t *__restrict__ slots,
                      const uint32_t *__restrict__ seg_bytes, const uint32_t *__restrict__ seg_off, const int32_t *__restrict__ sizes,
                      uint8_t *__restrict__ out)
{
    const int tid = threadIdx.x, s = blockIdx.x, k = blockIdx.y, nseg = gridDim.x;
    if (sizes[k] < 0) return;                                     // does not fit: nothing of this frame is written
    uint8_t *dst = out + (size_t)k * capacity;
    if (s == 0)
        for (int i = tid; i < header_bytes; i += 256) dst[i] = header[i];
    const size_t at = (size_t)k * (size_t)nseg + (size_t)s;
    const uint32_t n = seg_bytes[at], off = seg_off[at];
    const uint8_t *src = slots + at * pitch;
    for (uint32_t i = tid; i < n; i += 256u) dst[(size_t)off + i] = src[i];
    if (tid == 0) {
        dst[(size_t)off + n] = 0xFF;
        dst[(size_t)off + n + 1] = s == nseg - 1 ? 0xD9 : (uint8_t)(0xD0 + (s & 7));
    }
}

// ---- the boundary
struct SgJpegPlan {
    int nbx, nby;
    size_t nmcu, nseg, pitch, worst, coef_off, bytes_off, off_off, slots_off, ws_bytes;
};

static int sg_jpeg_plan(const char *who, int width, int height, int K, int ri, int header_bytes, SgJpegPlan *p)
{
    if (width < 1 || width > SG_JPEG_MAX_DIM || height < 1 || height > SG_JPEG_MAX_DIM)
        return sg_failf("%s: a frame of %d x %d pixels, 1..%d each way", who, width, height, SG_JPEG_MAX_DIM);
    if (K < 1 || K > SG_JPEG_MAX_FRAMES) return sg_failf("%s: K = %d frames, 1..%d per call", who, K, SG_JPEG_MAX_FRAMES);
    if (ri < 1 || ri > 65535) return sg_failf("%s: restart_interval = %d MCUs, 1..65535", who, ri);
    if (header_bytes < 1) return sg_failf("%s: header_bytes = %d", who, header_bytes);
    p->nbx = (width + 7) / 8; p->nby = (height + 7) / 8;
    p->nmcu = (size_t)p->nbx * (size_t)p->nby;
    p->nseg = (p->nmcu + (size_t)ri - 1) / (size_t)ri;
    const size_t per = (size_t)ri < p->nmcu ? (size_t)ri : p->nmcu;
    p->pitch = per * SG_JPEG_MCU_BYTES + 16;
    p->worst = (size_t)header_bytes + p->nmcu * SG_JPEG_MCU_BYTES + p->nseg * 18;
    if (p->worst >= ((size_t)1 << 31))
        return sg_failf("%s: a frame of %d x %d pixels can become a file of %llu bytes, at most 2^31 - 1 (sizes are int32)", who, width,
                        height, (unsigned long long)p->worst);
    auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
    p->coef_off = 0;
    p->bytes_off = up((size_t)K * p->nmcu * 192 * sizeof(int16_t));
    p->off_off = p->bytes_off + up((size_t)K * p->nseg * sizeof(uint32_t));
    p->slots_off = p->off_off + up((size_t)K * p->nseg * sizeof(uint32_t));
    p->ws_bytes = p->slots_off + (size_t)K * p->nseg * p->pitch;
    return 0;
}

extern "C" int sg_jpeg_layout(int width, int height, int K, int restart_interval, int header_bytes, size_t out[SG_JPEG_LAYOUT_WORDS])
{
    const char *who = "sg_jpeg_layout";
    if (!out) return sg_failf("%s: null pointer", who);
    SgJpegPlan p;
    if (sg_jpeg_plan(who, width, height, K, restart_interval, header_bytes, &p)) return 1;
    out[SG_JPEG_L_WS_BYTES] = p.ws_bytes;
    out[SG_JPEG_L_MCUS] = p.nmcu;
    out[SG_JPEG_L_SEGMENTS] = p.nseg;
    out[SG_JPEG_L_SLOT_PITCH] = p.pitch;
    out[SG_JPEG_L_WORST_BYTES] = p.worst;
    out[SG_JPEG_L_DEFAULT_CAPACITY] = (size_t)header_bytes + (size_t)width * (size_t)height * 3 / 2;
    return 0;
}

extern "C" int sg_jpeg_encode_frames(int K, int width, int height, int restart_interval, int bgr, const uint8_t *frames,
                                     const void *tables, const uint8_t *header, int header_bytes, void *ws, size_t ws_bytes, uint8_t *out,
                                     size_t capacity, int32_t *sizes, void *stream)
{
    const char *who = "sg_jpeg_encode_frames";
    if (!frames || !tables || !header || !ws || !out || !sizes) return sg_failf("%s: null pointer", who);
    SgJpegPlan p;
    if (sg_jpeg_plan(who, width, height, K, restart_interval, header_bytes, &p)) return 1;
    if (sg_codec_check_buffers(who, "sg_jpeg_layout", capacity, ws, ws_bytes, p.ws_bytes)) return 1;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *base = (uint8_t *)ws;
    int16_t *coef = (int16_t *)(base + p.coef_off);
    uint32_t *seg_bytes = (uint32_t *)(base + p.bytes_off), *seg_off = (uint32_t *)(base + p.off_off);
    uint8_t *slots = base + p.slots_off;
    const uint32_t *tab = (const uint32_t *)tables;
    hipLaunchKernelGGL(sg_jpeg_block_kernel, dim3((p.nbx + SG_JPEG_BLOCK_WAVES - 1) / SG_JPEG_BLOCK_WAVES, p.nby, K),
                       dim3(64 * SG_JPEG_BLOCK_WAVES), 0, st, width, height, p.nbx, bgr ? 1 : 0, frames, tab, coef);
    hipLaunchKernelGGL(sg_jpeg_entropy_kernel, dim3((unsigned)p.nseg, K), dim3(64), 0, st, (int)p.nmcu, restart_interval, p.pitch, tab, coef,
                       slots, seg_bytes);
    hipLaunchKernelGGL(sg_jpeg_scan_kernel, dim3(K), dim3(256), 0, st, (int)p.nseg, header_bytes, capacity, seg_bytes, seg_off, sizes);
    hipLaunchKernelGGL(sg_jpeg_gather_kernel, dim3((unsigned)p.nseg, K), dim3(256), 0, st, p.pitch, header_bytes, capacity, header, slots,
                       seg_bytes, seg_off, sizes, out);
    return sg_launched(who);
}
