// K uint8 frames to K PNG files (sg_png_encode_frames; include/sings_png.h states the stream and the table layout, sings_amd/png.py
// holds the numpy restatement the bytes are tested against).  Four launches, integer arithmetic throughout:
//
//   filter pass   one workgroup per scanline: the five candidate costs, the chosen type, the filtered scanline to the workspace, and
//                 the row's Adler partials (sum d and sum (L - i) d modulo 65521: rows combine exactly, whatever their order).
//   deflate pass  one wave per segment, 64 bytes (a lane each) per round.  A lane whose byte differs from the one before it closes
//                 the run that ends there: a ballot finds where that run began (or the open run carried from earlier rounds), and
//                 the run's tokens follow in closed form.  A count sweep sums their bits under all tables at once and the wave
//                 chooses the candidate; a write sweep places the codes -- positions by wave scan, codes ORed into LDS words (integer
//                 atomics on LDS, nothing else: the result does not depend on their order), complete words leave each round.  Then
//                 the CRC-32 of "IDAT" + the segment's bytes: lanes take equal spans and the spans are combined by multiplication
//                 with x^(8 * bytes behind the span) modulo the CRC polynomial.  A stored segment writes no slot: the gather copies
//                 the scanlines themselves.
//   scan          per frame: where every chunk starts, the file's size (or -needed), the Adler-32 from the rows' partials, and the
//                 last 30 bytes of the file (the closing IDAT with its CRC, and IEND).
//   gather        one workgroup per segment: length, "IDAT", data, CRC behind the header; the last one appends the 30 bytes.
#include "sg_codec.h"
#include "../../include/sings_png.h"

#define SG_PNG_LDS_WORDS 256                     // a round's bits: < 32 carried + 3215 (a 32 767-byte run closed) + 960 (64 literals) + 15
#define SG_PNG_ADLER 65521u
#define SG_PNG_CRC_POLY 0xEDB88320u
#define SG_PNG_TAIL_BYTES 30

__device__ __forceinline__ uint32_t sg_png_scan(uint32_t v, int lane)          // inclusive
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ unsigned long long sg_png_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- filter pass.  grid: (H, K), 256 threads: byte i of the row by thread i % 256.
__device__ __forceinline__ int sg_png_paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__global__ void __launch_bounds__(256)
sg_png_filter_kernel(int W, int H, int filter, int bgr, const uint8_t *__restrict__ frames, uint8_t *__restrict__ lines,
                     uint32_t *__restrict__ row_sums)
{
    __shared__ unsigned long long sm[4][5];
    __shared__ int s_type;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, y = blockIdx.x, k = blockIdx.y;
    const int n3 = 3 * W;
    const size_t row = (size_t)k * (size_t)H + (size_t)y;
    const uint8_t *cur = frames + row * (size_t)n3, *up = cur - n3;
    const bool has_up = y > 0;
    auto at = [&](const uint8_t *r, int i) -> int {               // byte i of a scanline: R G B, whatever the frame's order
        const int j = i % 3;
        return (int)r[bgr ? i + 2 - 2 * j : i];
    };
    int type = filter;
    if (filter == SG_PNG_FILTER_ADAPTIVE) {
        unsigned long long cost[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < n3; i += 256) {
            const int x = at(cur, i), a = i >= 3 ? at(cur, i - 3) : 0, b = has_up ? at(up, i) : 0, c = has_up && i >= 3 ? at(up, i - 3) : 0;
            const int f[5] = {x, x - a, x - b, x - ((a + b) >> 1), x - sg_png_paeth(a, b, c)};
#pragma unroll
            for (int t = 0; t < 5; t++) {
                const int v = f[t] & 255;
                cost[t] += (unsigned long long)(v < 128 ? v : 256 - v);
            }
        }
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const unsigned long long s = sg_png_wave_sum(cost[t]);
            if (lane == 0) sm[wave][t] = s;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            unsigned long long least = sm[0][0] + sm[1][0] + sm[2][0] + sm[3][0];
            for (int t = 1; t < 5; t++) {
                const unsigned long long s = sm[0][t] + sm[1][t] + sm[2][t] + sm[3][t];
                if (s < least) { least = s; best = t; }
            }
            s_type = best;
        }
        __syncthreads();
        type = s_type;
        __syncthreads();
    }
    const int L = 1 + n3;
    uint8_t *dst = lines + row * (size_t)L;
    unsigned long long s1 = 0, s2 = 0;                            // sum d, sum (L - index) d over this thread's bytes
    if (tid == 0) {
        dst[0] = (uint8_t)type;
        s1 = (unsigned long long)type;
        s2 = (unsigned long long)type * (unsigned long long)L;
    }
    for (int i = tid; i < n3; i += 256) {
        const int x = at(cur, i), a = i >= 3 ? at(cur, i - 3) : 0, b = has_up ? at(up, i) : 0, c = has_up && i >= 3 ? at(up, i - 3) : 0;
        int f = x;
        if (type == SG_PNG_FILTER_SUB) f = x - a;
        else if (type == SG_PNG_FILTER_UP) f = x - b;
        else if (type == SG_PNG_FILTER_AVERAGE) f = x - ((a + b) >> 1);
        else if (type == SG_PNG_FILTER_PAETH) f = x - sg_png_paeth(a, b, c);
        const unsigned long long d = (unsigned long long)(f & 255);
        dst[1 + i] = (uint8_t)d;
        s1 += d;
        s2 += d * (unsigned long long)(n3 - i);
    }
    s1 = sg_png_wave_sum(s1);
    s2 = sg_png_wave_sum(s2);
    if (lane == 0) { sm[wave][0] = s1; sm[wave][1] = s2; }
    __syncthreads();
    if (tid == 0) {
        row_sums[2 * row] = (uint32_t)((sm[0][0] + sm[1][0] + sm[2][0] + sm[3][0]) % SG_PNG_ADLER);
        row_sums[2 * row + 1] = (uint32_t)((sm[0][1] + sm[1][1] + sm[2][1] + sm[3][1]) % SG_PNG_ADLER);
    }
}

// ---- deflate pass
// A lane's writer into the round's bit buffer: bit p of the round is bit p % 32 of word p / 32 (the stream is LSB-first).  Codes of
// one lane arrive in ascending position, so the word in progress is kept in a register and ORed into LDS when the lane moves on.
struct SgPngBitWriter {
    uint32_t *words;
    uint32_t w, acc;
    __device__ __forceinline__ void flush() { if (acc && w < SG_PNG_LDS_WORDS) atomicOr(&words[w], acc); }
    __device__ __forceinline__ void put(uint32_t p, uint32_t entry)              // entry: value << 8 | bits, 1..25 bits
    {
        const uint32_t W = p >> 5, sh = p & 31u, n = entry & 255u;
        if (W != w) { flush(); w = W; acc = 0u; }
        const uint64_t v = (uint64_t)(entry >> 8) << sh;
        acc |= (uint32_t)v;
        if (n + sh > 32u) { flush(); w = W + 1u; acc = (uint32_t)(v >> 32); }
    }
};

__device__ __forceinline__ uint32_t sg_png_crc_mul(uint32_t a, uint32_t b)     // a(x) b(x) modulo the CRC polynomial, reflected
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? SG_PNG_CRC_POLY : 0u);
    }
    return p;
}

// grid: (segments, K), one wave each
__global__ void __launch_bounds__(64)
sg_png_deflate_kernel(int H, int L, int rps, int force, size_t pitch, const uint32_t *__restrict__ tables, const uint8_t *__restrict__ lines,
                      uint8_t *__restrict__ slots, uint32_t *__restrict__ seg_bytes, uint32_t *__restrict__ seg_kind,
                      uint32_t *__restrict__ seg_crc)
{
    __shared__ uint32_t tab[SG_PNG_TABLES * SG_PNG_TABLE_STRIDE];
    __shared__ uint32_t crct[256];
    __shared__ uint32_t words[SG_PNG_LDS_WORDS];
    const int lane = threadIdx.x, s = blockIdx.x, k = blockIdx.y, nseg = gridDim.x;
    const int row0 = s * rps, n = min(rps, H - row0) * L;        // 1 <= n <= SG_PNG_MAX_SEGMENT_BYTES
    const uint8_t *src = lines + ((size_t)k * (size_t)H + (size_t)row0) * (size_t)L;
    const size_t at = (size_t)k * (size_t)nseg + (size_t)s;
    uint8_t *slot = slots + at * pitch;
    for (int i = lane; i < SG_PNG_TABLES * SG_PNG_TABLE_STRIDE; i += 64) tab[i] = tables[i];
    for (int i = lane; i < 256; i += 64) crct[i] = tables[SG_PNG_T_CRC + i];
    for (int i = lane; i < SG_PNG_LDS_WORDS; i += 64) words[i] = 0u;
    __syncthreads();

    // One round of either sweep: lane's position p = base + lane; a lane at a run's first byte (or at p == n) closes the run in front
    // of it -- value v, length len -- when `closes` comes back true.  open: where the run still open began; last: the byte before base.
    int open = 0;
    uint32_t last = 0x200u;
    auto round = [&](int base, uint32_t &v, int &len) -> bool {
        const int p = base + lane;
        const uint32_t x = p < n ? (uint32_t)src[p] : 0x100u;     // (position n: a byte like no other, so the last run closes there)
        uint32_t prev = __shfl_up(x, 1, 64);
        if (lane == 0) prev = last;
        const bool start = p <= n && x != prev;
        const unsigned long long mask = __ballot(start);
        bool closes = false;
        if (start && p > 0) {
            const unsigned long long below = mask & ((1ull << lane) - 1ull);
            const int st = below ? base + 63 - __clzll((long long)below) : open;
            v = prev;
            len = p - st;
            closes = true;
        }
        if (mask) open = base + 63 - __clzll((long long)mask);
        last = __shfl(x, 63, 64);
        return closes;
    };

    // count sweep: the bits of this lane's tokens under every table
    uint32_t bits[SG_PNG_TABLES];
#pragma unroll
    for (int t = 0; t < SG_PNG_TABLES; t++) bits[t] = 0u;
    for (int base = 0; base <= n; base += 64) {
        uint32_t v = 0;
        int len = 0;
        if (round(base, v, len)) {
            const int m = len - 1, q = m / 258, r = m % 258;
#pragma unroll
            for (int t = 0; t < SG_PNG_TABLES; t++) {
                const uint32_t *tb = tab + t * SG_PNG_TABLE_STRIDE;
                const uint32_t lit = tb[v] & 255u;
                bits[t] += lit + (uint32_t)q * (tb[257 + 255] & 255u) + (r >= 3 ? (tb[257 + r - 3] & 255u) : (uint32_t)r * lit);
            }
        }
    }
    int choice = SG_PNG_TABLES;
    uint32_t size = (uint32_t)n + 5u;                             // the stored form
#pragma unroll
    for (int t = SG_PNG_TABLES - 1; t >= 0; t--) {                // (descending: ties go to the lowest index)
        const uint32_t total = (uint32_t)sg_png_wave_sum((unsigned long long)bits[t]) + tables[SG_PNG_T_PREFIX + t * SG_PNG_PREFIX_STRIDE] +
                               (tab[t * SG_PNG_TABLE_STRIDE + 256] & 255u);
        const uint32_t bytes = (total + 3u + 7u) / 8u + 4u;
        if (force < 0 ? bytes <= size : t == force) { size = bytes; choice = t; }
    }

    if (choice < SG_PNG_TABLES) {
        // write sweep
        const uint32_t *tb = tab + choice * SG_PNG_TABLE_STRIDE;
        const uint32_t *pre = tables + SG_PNG_T_PREFIX + choice * SG_PNG_PREFIX_STRIDE;
        const uint32_t pbits = pre[0];
        uint32_t outw = pbits >> 5, carry = pbits & 31u;          // words of the slot written; bits of words[0] in use (< 32)
        uint32_t *slotw = (uint32_t *)slot;
        if ((uint32_t)lane < outw && ((size_t)lane + 1) * 4 <= pitch) slotw[lane] = pre[1 + lane];     // (outw < SG_PNG_PREFIX_STRIDE <= 64)
        if (lane == 0) words[0] = carry ? pre[1 + outw] : 0u;
        __syncthreads();
        open = 0;
        last = 0x200u;
        for (int base = 0; base <= n; base += 64) {
            uint32_t v = 0;
            int len = 0;
            const bool closes = round(base, v, len);
            const bool end = base + lane == n;
            if (!__any(closes || end)) continue;                  // (a round inside one run: nothing to write)
            int q = 0, r = 0;
            uint32_t nb = 0;
            if (closes) {
                const int m = len - 1;
                q = m / 258;
                r = m % 258;
                const uint32_t lit = tb[v] & 255u;
                nb = lit + (uint32_t)q * (tb[257 + 255] & 255u) + (r >= 3 ? (tb[257 + r - 3] & 255u) : (uint32_t)r * lit);
            }
            if (end) nb += tb[256] & 255u;
            const uint32_t incl = sg_png_scan(nb, lane);
            const uint32_t total = carry + __shfl(incl, 63, 64);
            if (nb) {
                uint32_t p = carry + incl - nb;
                SgPngBitWriter bw = {words, p >> 5, 0u};
                if (closes) {
                    const uint32_t lit = tb[v];
                    bw.put(p, lit);
                    p += lit & 255u;
                    const uint32_t far = tb[257 + 255];
                    for (int i = 0; i < q; i++) { bw.put(p, far); p += far & 255u; }
                    if (r >= 3) {
                        const uint32_t e = tb[257 + r - 3];
                        bw.put(p, e);
                        p += e & 255u;
                    } else {
                        for (int i = 0; i < r; i++) { bw.put(p, lit); p += lit & 255u; }
                    }
                }
                if (end) bw.put(p, tb[256]);
                bw.flush();
            }
            __syncthreads();
            // the complete words leave; the partial last word is carried into the next round
            const uint32_t full = min(total >> 5, (uint32_t)SG_PNG_LDS_WORDS - 1u);
            uint32_t mine[SG_PNG_LDS_WORDS / 64];
#pragma unroll
            for (int j = 0; j < SG_PNG_LDS_WORDS / 64; j++) mine[j] = words[64 * j + lane];
            const uint32_t rest = words[full];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SG_PNG_LDS_WORDS / 64; j++) {
                const uint32_t w = 64u * j + lane;
                if (w < full && ((size_t)outw + w + 1) * 4 <= pitch) slotw[outw + w] = mine[j];
                words[w] = w == 0u ? rest : 0u;
            }
            outw += full;
            carry = total & 31u;
            __syncthreads();
        }
        if (lane == 0) {
            // the empty stored block: three zero bits, zeros to the byte boundary, LEN = 0, NLEN = FFFF
            const uint32_t nbytes = (carry + 3u + 7u) / 8u, w0 = words[0];
            size_t o = (size_t)outw * 4;
            for (uint32_t j = 0; j < nbytes + 4u; j++, o++) {
                const uint32_t byte = j < nbytes ? (j < 4u ? (w0 >> (8u * j)) & 255u : 0u) : (j < nbytes + 2u ? 0u : 255u);
                if (o < pitch) slot[o] = (uint8_t)byte;
            }
            size = (uint32_t)o;
        }
        size = __shfl(size, 0, 64);
        __threadfence_block();
        __syncthreads();
    }

    // CRC-32 of "IDAT" + the segment's bytes
    const uint32_t M = 4u + size, span = (M + 63u) / 64u;
    const uint32_t b0 = min((uint32_t)lane * span, M), b1 = min(b0 + span, M);
    uint32_t reg = lane == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t i = b0; i < b1; i++) {
        uint32_t byte;
        if (i < 4u) byte = (0x54414449u >> (8u * i)) & 255u;     // 'I' 'D' 'A' 'T'
        else if (choice < SG_PNG_TABLES) byte = (size_t)(i - 4u) < pitch ? slot[i - 4u] : 0u;
        else {
            const uint32_t j = i - 4u;
            byte = j == 0u ? 0u : j == 1u ? (uint32_t)n & 255u : j == 2u ? (uint32_t)n >> 8 : j == 3u ? ~(uint32_t)n & 255u
                 : j == 4u ? (~(uint32_t)n >> 8) & 255u : (uint32_t)src[j - 5u];
        }
        reg = crct[(reg ^ byte) & 255u] ^ (reg >> 8);
    }
    const uint32_t behind = M - b1;                               // < 2^SG_PNG_POW_WORDS
    for (int j = 0; j < SG_PNG_POW_WORDS; j++)
        if ((behind >> j) & 1u) reg = sg_png_crc_mul(reg, tables[SG_PNG_T_POW + j]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) reg ^= __shfl_xor(reg, d, 64);
    if (lane == 0) {
        seg_bytes[at] = size;
        seg_kind[at] = choice == SG_PNG_TABLES ? 1u : 0u;
        seg_crc[at] = reg ^ 0xFFFFFFFFu;
    }
}

// ---- scan.  grid: K, 256 threads.
__global__ void __launch_bounds__(256)
sg_png_scan_kernel(int H, int L, int nseg, int header_bytes, size_t capacity, const uint32_t *__restrict__ tables,
                   const uint32_t *__restrict__ row_sums, const uint32_t *__restrict__ seg_bytes, uint32_t *__restrict__ seg_off,
                   uint8_t *__restrict__ tails, int32_t *__restrict__ sizes)
{
    __shared__ uint32_t sm[256];
    __shared__ unsigned long long red[4][2];
    const int tid = threadIdx.x, k = blockIdx.x;
    // a segment inside its chunk: + length, type and CRC
    const unsigned long long running = sg_codec_segment_offsets(k, nseg, 12u, header_bytes, seg_bytes, seg_off, sm);
    // Adler-32 of the H scanlines from their partials: a = 1 + sum A_r, b = H L + sum (B_r + (H - 1 - r) L A_r), modulo 65521
    unsigned long long sa = 0, sb = 0;
    for (int r = tid; r < H; r += 256) {
        const unsigned long long A = row_sums[2 * ((size_t)k * (size_t)H + (size_t)r)], B = row_sums[2 * ((size_t)k * (size_t)H + (size_t)r) + 1];
        const unsigned long long behind = ((unsigned long long)(H - 1 - r) * (unsigned long long)L) % SG_PNG_ADLER;
        sa += A;
        sb += B + behind * A;
    }
    sa = sg_png_wave_sum(sa);
    sb = sg_png_wave_sum(sb);
    if ((tid & 63) == 0) { red[tid >> 6][0] = sa; red[tid >> 6][1] = sb; }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long needed = running + SG_PNG_TAIL_BYTES;
        sizes[k] = needed <= (unsigned long long)capacity ? (int32_t)needed : -(int32_t)(needed < 0x7FFFFFFFull ? needed : 0x7FFFFFFFull);
        const uint32_t a = (uint32_t)((1ull + red[0][0] + red[1][0] + red[2][0] + red[3][0]) % SG_PNG_ADLER);
        const uint32_t b = (uint32_t)(((unsigned long long)H * (unsigned long long)L + red[0][1] + red[1][1] + red[2][1] + red[3][1]) % SG_PNG_ADLER);
        const uint32_t adler = b << 16 | a;
        uint8_t *t = tails + (size_t)k * 32;
        const uint8_t head[10] = {0, 0, 0, 6, 'I', 'D', 'A', 'T', 0x03, 0x00};
        for (int i = 0; i < 10; i++) t[i] = head[i];
        for (int i = 0; i < 4; i++) t[10 + i] = (uint8_t)(adler >> (24 - 8 * i));
        uint32_t reg = 0xFFFFFFFFu;
        for (int i = 4; i < 14; i++) reg = tables[SG_PNG_T_CRC + ((reg ^ t[i]) & 255u)] ^ (reg >> 8);
        reg ^= 0xFFFFFFFFu;
        for (int i = 0; i < 4; i++) t[14 + i] = (uint8_t)(reg >> (24 - 8 * i));
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; i++) t[18 + i] = iend[i];
    }
}

// ---- gather.  grid: (segments, K)
__global__ void __launch_bounds__(256)
sg_png_gather_kernel(int H, int L, int rps, size_t pitch, int header_bytes, size_t capacity, const uint8_t *__restrict__ header,
                     const uint8_t *__restrict__ lines, const uint8_t *__restrict__ slots, const uint32_t *__restrict__ seg_bytes,
                     const uint32_t *__restrict__ seg_kind, const uint32_t *__restrict__ seg_crc, const uint32_t *__restrict__ seg_off,
                     const uint8_t *__restrict__ tails, const int32_t *__restrict__ sizes, uint8_t *__restrict__ out)
{
    const int tid = threadIdx.x, s = blockIdx.x, k = blockIdx.y, nseg = gridDim.x;
    if (sizes[k] < 0) return;                                     // does not fit: nothing of this frame is written
    uint8_t *dst = out + (size_t)k * capacity;
    if (s == 0)
        for (int i = tid; i < header_bytes; i += 256) dst[i] = header[i];
    const size_t at = (size_t)k * (size_t)nseg + (size_t)s;
    const uint32_t n = seg_bytes[at], crc = seg_crc[at];
    uint8_t *chunk = dst + seg_off[at];
    if (tid < 4) {
        chunk[tid] = (uint8_t)(n >> (24 - 8 * tid));
        chunk[4 + tid] = (uint8_t)(0x54414449u >> (8 * tid));
        chunk[8 + n + tid] = (uint8_t)(crc >> (24 - 8 * tid));
    }
    uint8_t *data = chunk + 8;
    if (seg_kind[at]) {
        const uint32_t raw = n - 5u;
        const uint8_t *src = lines + ((size_t)k * (size_t)H + (size_t)s * (size_t)rps) * (size_t)L;
        if (tid == 0) {
            data[0] = 0;
            data[1] = (uint8_t)(raw & 255u);
            data[2] = (uint8_t)(raw >> 8);
            data[3] = (uint8_t)(~raw & 255u);
            data[4] = (uint8_t)((~raw >> 8) & 255u);
        }
        for (uint32_t i = tid; i < raw; i += 256u) data[5u + i] = src[i];
    } else {
        const uint8_t *src = slots + at * pitch;
        for (uint32_t i = tid; i < n; i += 256u) data[i] = src[i];
    }
    if (s == nseg - 1 && tid < SG_PNG_TAIL_BYTES) chunk[12u + n + tid] = tails[(size_t)k * 32 + tid];
}

// ---- the boundary
struct SgPngPlan {
    int L;
    size_t nseg, seg_bytes, pitch, worst, lines_off, rows_off, bytes_off, kind_off, crc_off, off_off, tails_off, slots_off, ws_bytes;
};

static int sg_png_plan(const char *who, int width, int height, int K, int rps, int header_bytes, SgPngPlan *p)
{
    if (width < 1 || width > SG_PNG_MAX_WIDTH || height < 1 || height > SG_PNG_MAX_HEIGHT)
        return sg_failf("%s: a frame of %d x %d pixels, 1..%d wide and 1..%d high", who, width, height, SG_PNG_MAX_WIDTH, SG_PNG_MAX_HEIGHT);
    if (K < 1 || K > SG_PNG_MAX_FRAMES) return sg_failf("%s: K = %d frames, 1..%d per call", who, K, SG_PNG_MAX_FRAMES);
    if (header_bytes < 1) return sg_failf("%s: header_bytes = %d", who, header_bytes);
    p->L = 1 + 3 * width;
    const size_t rows = (size_t)(rps < height ? rps : height);
    if (rps < 1 || rows * (size_t)p->L > SG_PNG_MAX_SEGMENT_BYTES)
        return sg_failf("%s: rows_per_segment = %d scanlines of %d bytes, a segment holds 1..%d bytes", who, rps, p->L, SG_PNG_MAX_SEGMENT_BYTES);
    p->nseg = ((size_t)height + (size_t)rps - 1) / (size_t)rps;
    p->seg_bytes = rows * (size_t)p->L;
    // (a forced table may spend 15 bits on every byte: the slot holds that, whatever `force` is)
    p->pitch = (2 * p->seg_bytes + 4 * SG_PNG_PREFIX_STRIDE + 16 + 15) & ~(size_t)15;
    p->worst = (size_t)header_bytes + (size_t)height * (size_t)p->L + p->nseg * 17 + SG_PNG_TAIL_BYTES;
    if (p->worst >= ((size_t)1 << 31))
        return sg_failf("%s: a frame of %d x %d pixels can become a file of %llu bytes, at most 2^31 - 1 (sizes are int32)", who, width,
                        height, (unsigned long long)p->worst);
    auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t per_seg = up((size_t)K * p->nseg * sizeof(uint32_t));
    p->lines_off = 0;
    p->rows_off = up((size_t)K * (size_t)height * (size_t)p->L);
    p->bytes_off = p->rows_off + up((size_t)K * (size_t)height * 2 * sizeof(uint32_t));
    p->kind_off = p->bytes_off + per_seg;
    p->crc_off = p->kind_off + per_seg;
    p->off_off = p->crc_off + per_seg;
    p->tails_off = p->off_off + per_seg;
    p->slots_off = p->tails_off + (size_t)K * 32;
    p->ws_bytes = p->slots_off + (size_t)K * p->nseg * p->pitch;
    return 0;
}

extern "C" int sg_png_layout(int width, int height, int K, int rows_per_segment, int header_bytes, size_t out[SG_PNG_LAYOUT_WORDS])
{
    const char *who = "sg_png_layout";
    if (!out) return sg_failf("%s: null pointer", who);
    SgPngPlan p;
    if (sg_png_plan(who, width, height, K, rows_per_segment, header_bytes, &p)) return 1;
    out[SG_PNG_L_WS_BYTES] = p.ws_bytes;
    out[SG_PNG_L_SEGMENTS] = p.nseg;
    out[SG_PNG_L_SEGMENT_BYTES] = p.seg_bytes;
    out[SG_PNG_L_SLOT_PITCH] = p.pitch;
    out[SG_PNG_L_WORST_BYTES] = p.worst;
    return 0;
}

extern "C" int sg_png_encode_frames(int K, int width, int height, int rows_per_segment, int filter, int bgr, int force,
                                    const uint8_t *frames, const void *tables, const uint8_t *header, int header_bytes, void *ws,
                                    size_t ws_bytes, uint8_t *out, size_t capacity, int32_t *sizes, void *stream)
{
    const char *who = "sg_png_encode_frames";
    if (!frames || !tables || !header || !ws || !out || !sizes) return sg_failf("%s: null pointer", who);
    SgPngPlan p;
    if (sg_png_plan(who, width, height, K, rows_per_segment, header_bytes, &p)) return 1;
    if (filter < SG_PNG_FILTER_NONE || filter > SG_PNG_FILTER_ADAPTIVE) return sg_failf("%s: filter = %d, 0..%d", who, filter, SG_PNG_FILTER_ADAPTIVE);
    if (force < -1 || force > SG_PNG_TABLES) return sg_failf("%s: force = %d, -1 or a candidate 0..%d", who, force, SG_PNG_TABLES);
    if (sg_codec_check_buffers(who, "sg_png_layout", capacity, ws, ws_bytes, p.ws_bytes)) return 1;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *base = (uint8_t *)ws;
    uint8_t *lines = base + p.lines_off, *tails = base + p.tails_off, *slots = base + p.slots_off;
    uint32_t *row_sums = (uint32_t *)(base + p.rows_off), *seg_bytes = (uint32_t *)(base + p.bytes_off);
    uint32_t *seg_kind = (uint32_t *)(base + p.kind_off), *seg_crc = (uint32_t *)(base + p.crc_off), *seg_off = (uint32_t *)(base + p.off_off);
    const uint32_t *tab = (const uint32_t *)tables;
    hipLaunchKernelGGL(sg_png_filter_kernel, dim3(height, K), dim3(256), 0, st, width, height, filter, bgr ? 1 : 0, frames, lines, row_sums);
    hipLaunchKernelGGL(sg_png_deflate_kernel, dim3((unsigned)p.nseg, K), dim3(64), 0, st, height, p.L, rows_per_segment, force, p.pitch, tab,
                       lines, slots, seg_bytes, seg_kind, seg_crc);
    hipLaunchKernelGGL(sg_png_scan_kernel, dim3(K), dim3(256), 0, st, height, p.L, (int)p.nseg, header_bytes, capacity, tab, row_sums,
                       seg_bytes, seg_off, tails, sizes);
    hipLaunchKernelGGL(sg_png_gather_kernel, dim3((unsigned)p.nseg, K), dim3(256), 0, st, height, p.L, rows_per_segment, p.pitch,
                       header_bytes, capacity, header, lines, slots, seg_bytes, seg_kind, seg_crc, seg_off, tails, sizes, out);
    return sg_launched(who);
}
