// The decode core of include/sings_unpng.h: a zlib stream (RFC 1950 around RFC 1951) to `expected` raw bytes, or the first error as an
// SG_UNPNG_E_* code.  One text for the host and the device: the bit reader, the code-length reader, the table build, the symbol loop
// and every bounds check are here; the caller brings the two primitives that differ, as an object with
//     void literal(uint8_t b)                     append one byte
//     void copy(uint32_t dist, uint32_t len)      append len bytes, each the byte dist behind it (dist may be shorter than len)
//     uint32_t adler()                            the Adler-32 of everything appended
// Both primitives are only called with arguments the core has checked: the output never grows past `expected`, and
// 1 <= dist <= bytes appended so far, dist <= 32 768, 3 <= len <= 258.  sings_amd/unpng.py inflate_host restates this file in Python,
// code for code; tests/tools/inflate_check.cpp runs it on the host under the sanitizers.
//
// No input can make it loop for ever or index outside a table: every symbol consumes at least one bit of the input, so the loops end
// with the stream; a code-length set is counted before it is used (over-subscribed or incomplete: refused); a decoded symbol is looked
// up only below the number of symbols the set has.  No HIP types; SG_INFLATE_UNIFORM(x) is the identity unless the includer defines it
// (the device build: every lane of the wave decodes the same bits, and the macro tells the compiler so).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sings_unpng.h"

#if defined(__HIPCC__)
#define SG_INFLATE_HD __host__ __device__ inline
#else
#define SG_INFLATE_HD inline
#endif
#ifndef SG_INFLATE_UNIFORM
#define SG_INFLATE_UNIFORM(x) (x)
#endif

#define SG_INFLATE_FAST_BITS 9
#define SG_INFLATE_FAST_SIZE 512        // 1 << SG_INFLATE_FAST_BITS
#define SG_INFLATE_MAX_LITLEN 288
#define SG_INFLATE_MAX_DIST 32
#define SG_INFLATE_WINDOW 32768

// One Huffman code: fast[the next 9 bits] = symbol << 4 | bits for codes of at most 9 bits (0: a longer code, or none); count[] and
// symbol[] are the canonical code by length, walked a bit at a time for the rest.
struct SgInflateCode {
    uint16_t fast[SG_INFLATE_FAST_SIZE];
    uint16_t count[16];
    uint16_t symbol[SG_INFLATE_MAX_LITLEN];
    uint16_t n;                                                   // symbols the set has: symbol[] holds fewer than this
};

struct SgInflateTables {
    SgInflateCode litlen, dist;
    uint16_t next[16];                                            // the build's running offsets and codes
    uint8_t lens[SG_INFLATE_MAX_LITLEN + SG_INFLATE_MAX_DIST];
    int32_t fixed;                                                // litlen and dist hold the fixed code
};

struct SgInflateBits {
    const uint8_t *in;
    size_t len, pos;
    uint64_t buf;                                                 // the next `n` bits, LSB first (above them: see sg_inflate_refill)
    int n;
};

// Eight bytes at a time while the stream has them: the whole bytes that fit below bit 63 are counted in, and the bits of the next
// byte that land above `n` are that byte's own low bits -- the next refill reads the same byte to the same place, and OR-ing them
// again changes nothing.  (So "zeros above them" holds for the last seven bytes of the stream, where it is needed: a code is only
// looked up beyond `n` bits when the stream has ended.)
SG_INFLATE_HD void sg_inflate_refill(SgInflateBits &b)
{
    if (b.n <= 56 && b.len - b.pos >= 8) {
        const uint8_t *p = b.in + b.pos;
        uint32_t lo, hi;
        __builtin_memcpy(&lo, p, 4);
        __builtin_memcpy(&hi, p + 4, 4);
        const uint64_t w = (uint64_t)SG_INFLATE_UNIFORM(hi) << 32 | (uint64_t)SG_INFLATE_UNIFORM(lo);      // (little-endian hosts and devices)
        const int bytes = (63 - b.n) >> 3;
        b.buf |= w << b.n;
        b.pos += (size_t)bytes;
        b.n += 8 * bytes;
        return;
    }
    while (b.n <= 56 && b.pos < b.len) {
        b.buf |= (uint64_t)SG_INFLATE_UNIFORM((uint32_t)b.in[b.pos]) << b.n;
        b.pos++;
        b.n += 8;
    }
}

// k <= 32 bits into v: false when the stream has fewer
SG_INFLATE_HD bool sg_inflate_take(SgInflateBits &b, int k, uint32_t &v)
{
    if (b.n < k) sg_inflate_refill(b);
    if (b.n < k) return false;
    v = (uint32_t)(b.buf & ((1ull << k) - 1ull));
    b.buf >>= k;
    b.n -= k;
    return true;
}

// lens[0..n) to a code.  0: complete (or empty); 1: incomplete; -1: over-subscribed.  `longest` receives the longest code's bits.
SG_INFLATE_HD int sg_inflate_build(SgInflateCode &c, const uint8_t *lens, int n, uint16_t *next, int &longest)
{
    for (int i = 0; i < 16; i++) c.count[i] = 0;
    for (int i = 0; i < SG_INFLATE_FAST_SIZE; i++) c.fast[i] = 0;
    c.n = (uint16_t)n;
    for (int s = 0; s < n; s++) c.count[lens[s] & 15]++;
    longest = 0;
    int left = 1;
    for (int len = 1; len <= 15; len++) {
        left = (left << 1) - (int)c.count[len];
        if (left < 0) return -1;
        if (c.count[len]) longest = len;
    }
    // symbol[]: the symbols in the order of their codes
    next[1] = 0;
    for (int len = 1; len < 15; len++) next[len + 1] = (uint16_t)(next[len] + c.count[len]);
    for (int s = 0; s < n; s++) {
        const int len = lens[s] & 15;
        if (len) {
            const uint16_t at = next[len]++;
            if (at < SG_INFLATE_MAX_LITLEN) c.symbol[at] = (uint16_t)s;
        }
    }
    // fast[]: the first code of every length, then the codes of at most 9 bits, bit-reversed (the stream is LSB first)
    uint32_t code = 0;
    for (int len = 1; len <= 15; len++) {
        code = (code + c.count[len - 1] * (len > 1 ? 1u : 0u)) << 1;
        next[len] = (uint16_t)code;
    }
    for (int s = 0; s < n; s++) {
        const int len = lens[s] & 15;
        if (len == 0 || len > SG_INFLATE_FAST_BITS) continue;
        uint32_t v = next[len]++, rev = 0;
        for (int i = 0; i < len; i++) { rev = rev << 1 | (v & 1u); v >>= 1; }
        for (uint32_t k = rev; k < SG_INFLATE_FAST_SIZE; k += 1u << len) c.fast[k] = (uint16_t)(s << 4 | len);
    }
    return longest == 0 ? 0 : (left > 0 ? 1 : 0);
}

// The next symbol of code c: >= 0, or -1 when the stream ends inside it, or -2 for a bit pattern that is no code.
SG_INFLATE_HD int sg_inflate_symbol(const SgInflateCode &c, SgInflateBits &b)
{
    if (b.n < 15) sg_inflate_refill(b);
    const uint32_t e = SG_INFLATE_UNIFORM((uint32_t)c.fast[b.buf & (SG_INFLATE_FAST_SIZE - 1)]);
    if (e) {
        const int len = (int)(e & 15u);
        if (len > b.n) return -1;
        b.buf >>= len;
        b.n -= len;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; len++) {
        if (len > b.n) return -1;
        code |= (int)((b.buf >> (len - 1)) & 1ull);
        const int count = (int)SG_INFLATE_UNIFORM((uint32_t)c.count[len]);
        if (code - count < first) {
            const int at = index + (code - first);
            if (at < 0 || at >= (int)c.n || at >= SG_INFLATE_MAX_LITLEN) return -2;
            b.buf >>= len;
            b.n -= len;
            return (int)SG_INFLATE_UNIFORM((uint32_t)c.symbol[at]);
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -2;
}

SG_INFLATE_HD void sg_inflate_fixed(SgInflateTables &t)
{
    if (t.fixed) return;
    for (int s = 0; s < 288; s++) t.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < 32; s++) t.lens[288 + s] = 5;             // (30 and 31 take part in the code and are refused when decoded)
    int longest;
    sg_inflate_build(t.litlen, t.lens, 288, t.next, longest);
    sg_inflate_build(t.dist, t.lens + 288, 32, t.next, longest);
    t.fixed = 1;
}

// The header of a dynamic block: 0 or an SG_UNPNG_E_* code.
SG_INFLATE_HD int sg_inflate_dynamic(SgInflateTables &t, SgInflateBits &b)
{
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v;
    if (!sg_inflate_take(b, 14, v)) return SG_UNPNG_E_INPUT;
    const int nlen = (int)(v & 31u) + 257, ndist = (int)((v >> 5) & 31u) + 1, ncode = (int)(v >> 10) + 4;
    if (nlen > 286 || ndist > 30) return SG_UNPNG_E_COUNTS;
    t.fixed = 0;
    for (int i = 0; i < 19; i++) t.lens[i] = 0;
    for (int i = 0; i < ncode; i++) {
        if (!sg_inflate_take(b, 3, v)) return SG_UNPNG_E_INPUT;
        t.lens[order[i]] = (uint8_t)v;
    }
    int longest;
    // (the code-length code is built where the distance code will be: 19 symbols)
    if (sg_inflate_build(t.dist, t.lens, 19, t.next, longest) != 0 || longest == 0) return SG_UNPNG_E_CODE_LENGTHS;
    int at = 0;
    while (at < nlen + ndist) {
        const int sym = sg_inflate_symbol(t.dist, b);
        if (sym == -1) return SG_UNPNG_E_INPUT;
        if (sym < 0 || sym > 18) return SG_UNPNG_E_CODE_LENGTHS;
        if (sym < 16) {
            t.lens[at++] = (uint8_t)sym;
            continue;
        }
        uint8_t value = 0;
        int repeat;
        if (sym == 16) {
            if (at == 0) return SG_UNPNG_E_REPEAT;
            value = t.lens[at - 1];
            if (!sg_inflate_take(b, 2, v)) return SG_UNPNG_E_INPUT;
            repeat = 3 + (int)v;
        } else if (sym == 17) {
            if (!sg_inflate_take(b, 3, v)) return SG_UNPNG_E_INPUT;
            repeat = 3 + (int)v;
        } else {
            if (!sg_inflate_take(b, 7, v)) return SG_UNPNG_E_INPUT;
            repeat = 11 + (int)v;
        }
        if (at + repeat > nlen + ndist) return SG_UNPNG_E_REPEAT;
        for (int i = 0; i < repeat; i++) t.lens[at++] = value;
    }
    if (t.lens[256] == 0) return SG_UNPNG_E_NO_END;
    // (the distance lengths move behind the 288 literal/length places before the literal/length build reads its own)
    for (int i = ndist - 1; i >= 0; i--) t.lens[288 + i] = t.lens[nlen + i];
    int r = sg_inflate_build(t.litlen, t.lens, nlen, t.next, longest);
    if (r < 0 || (r > 0 && longest != 1)) return SG_UNPNG_E_LITLEN_SET;
    r = sg_inflate_build(t.dist, t.lens + 288, ndist, t.next, longest);
    if (r < 0 || (r > 0 && longest != 1)) return SG_UNPNG_E_DIST_SET;
    return 0;
}

template <class Out>
SG_INFLATE_HD int sg_inflate(const uint8_t *in, size_t in_len, size_t expected, SgInflateTables &t, Out &out)
{
    SgInflateBits b = {in, in_len, 0, 0ull, 0};
    uint32_t v;
    t.fixed = 0;
    // RFC 1950: CMF, FLG
    if (!sg_inflate_take(b, 16, v)) return SG_UNPNG_E_INPUT;
    const uint32_t cmf = v & 255u, flg = v >> 8;
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return SG_UNPNG_E_HEADER;
    // (The window size the header declares is not held against the distances: zlib's inflate does that only when it is built strict,
    // so a stream it reads may reach further back than its header says, up to 32 768, and is read here too.)
    size_t produced = 0;
    for (;;) {
        if (!sg_inflate_take(b, 3, v)) return SG_UNPNG_E_INPUT;
        const uint32_t last = v & 1u, type = v >> 1;
        if (type == 3u) return SG_UNPNG_E_BLOCK_TYPE;
        if (type == 0u) {
            const int drop = b.n & 7;                             // to the byte boundary
            b.buf >>= drop;
            b.n -= drop;
            if (!sg_inflate_take(b, 32, v)) return SG_UNPNG_E_INPUT;
            const uint32_t len = v & 0xFFFFu;
            if ((len ^ 0xFFFFu) != (v >> 16)) return SG_UNPNG_E_STORED;
            for (uint32_t i = 0; i < len; i++) {
                uint32_t byte;
                if (!sg_inflate_take(b, 8, byte)) return SG_UNPNG_E_INPUT;
                if (produced >= expected) return SG_UNPNG_E_OUTPUT_LONG;
                out.literal((uint8_t)byte);
                produced++;
            }
        } else {
            if (type == 1u) sg_inflate_fixed(t);
            else {
                const int e = sg_inflate_dynamic(t, b);
                if (e) return e;
            }
            for (;;) {
                int sym = sg_inflate_symbol(t.litlen, b);
                if (sym == -1) return SG_UNPNG_E_INPUT;
                if (sym < 0 || sym > 285) return SG_UNPNG_E_LITLEN_SYMBOL;
                if (sym < 256) {
                    if (produced >= expected) return SG_UNPNG_E_OUTPUT_LONG;
                    out.literal((uint8_t)sym);
                    produced++;
                    continue;
                }
                if (sym == 256) break;
                uint32_t len, extra = 0;
                if (sym < 265) len = (uint32_t)sym - 254u;
                else if (sym == 285) len = 258u;
                else {
                    const int bits = (sym - 261) >> 2;
                    if (!sg_inflate_take(b, bits, extra)) return SG_UNPNG_E_INPUT;
                    len = 3u + ((4u + (uint32_t)((sym - 265) & 3)) << bits) + extra;
                }
                sym = sg_inflate_symbol(t.dist, b);
                if (sym == -1) return SG_UNPNG_E_INPUT;
                if (sym < 0 || sym > 29) return SG_UNPNG_E_DIST_SYMBOL;
                uint32_t dist;
                if (sym < 4) dist = (uint32_t)sym + 1u;
                else {
                    const int bits = (sym >> 1) - 1;
                    if (!sg_inflate_take(b, bits, extra)) return SG_UNPNG_E_INPUT;
                    dist = 1u + ((2u + (uint32_t)(sym & 1)) << bits) + extra;
                }
                if ((size_t)dist > produced || dist > SG_INFLATE_WINDOW) return SG_UNPNG_E_DISTANCE;
                if ((size_t)len > expected - produced) return SG_UNPNG_E_OUTPUT_LONG;
                out.copy(dist, len);
                produced += len;
            }
        }
        if (last) break;
    }
    if (produced != expected) return SG_UNPNG_E_OUTPUT_SHORT;
    // RFC 1950: the Adler-32, big-endian, from the next byte boundary
    const int drop = b.n & 7;
    b.buf >>= drop;
    b.n -= drop;
    if (!sg_inflate_take(b, 32, v)) return SG_UNPNG_E_INPUT;
    const uint32_t adler = (v & 255u) << 24 | (v >> 8 & 255u) << 16 | (v >> 16 & 255u) << 8 | v >> 24;
    if (adler != out.adler()) return SG_UNPNG_E_ADLER;
    return 0;
}
