"""Frames out as PNG files encoded on the device.

Every picture the reference writes is a PNG.  Here the K uint8 frames an animation launch already produces (``frame_out.frames_to_u8``) are
filtered, deflated and wrapped into K complete PNG files by four HIP launches (``sg_png_encode_frames``, include/sings_png.h) and read
back in one copy.

 * ``PngEncoder`` (on ``codec._FrameEncoder``): pre-allocated workspaces for K frames of W x H; ``encode`` (device buffers, legal
   inside a graph capture) and ``encode_to_host`` (a list of ``bytes``).
 * ``png_encode_host``: the numpy twin -- the same stream, byte for byte, without a device.  It is the restatement the device path is
   tested against, not a fallback: nothing in the product calls it.
 * ``animate_to_frames``: ``posed.animate_chunk(out="png")`` into numbered files -- the reference's ``animate(keep_images=True)``.

The stream is fixed so that bytes can be compared (include/sings_png.h states it in full): 8-bit RGB, no ancillary chunks, one zlib
stream cut into segments of ``rows_per_segment`` scanlines, each compressed on its own into an ``IDAT`` chunk and ended by an empty
stored block, so that segments are independent and byte aligned.  A segment's tokens are zlib's RLE strategy in closed form (matches at
distance 1 only); they are coded with the fixed code, with one of four pre-built dynamic codes (``CODE_LENGTHS``) or left stored,
whichever is smallest.  Everything is integer arithmetic.  Out of scope: RGBA, grey and 16-bit, interlace, matches at other distances,
Huffman codes built per image, APNG.
"""
import os
import struct
import zlib

import numpy as np

from .codec import MAX_FRAMES, _FrameEncoder       # MAX_FRAMES: SG_PNG_MAX_FRAMES

MAX_WIDTH = 10922                    # SG_PNG_MAX_WIDTH: a scanline (1 + 3 W bytes) must fit in a segment
MAX_HEIGHT = 65535                   # SG_PNG_MAX_HEIGHT
MAX_SEGMENT_BYTES = 32768            # SG_PNG_MAX_SEGMENT_BYTES
TABLES = 5                           # SG_PNG_TABLES: the fixed code and four dynamic codes; candidate TABLES is the stored form
TABLE_STRIDE = 520                   # SG_PNG_TABLE_STRIDE: 256 literals | end of block | matches of 3..258 bytes
PREFIX_STRIDE = 48                   # SG_PNG_PREFIX_STRIDE: the bits of a table's block prefix, then the bits themselves
TABLE_WORDS = 3120                   # SG_PNG_TABLE_WORDS
T_PREFIX = TABLES * TABLE_STRIDE                                  # SG_PNG_T_PREFIX
T_CRC = T_PREFIX + TABLES * PREFIX_STRIDE                         # SG_PNG_T_CRC
T_POW = T_CRC + 256                                               # SG_PNG_T_POW
POW_WORDS = 20                       # SG_PNG_POW_WORDS
HEADER_BYTES = 47                    # signature, IHDR, and the IDAT that holds the zlib header
FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")   # SG_PNG_FILTER_*: 0..4 the PNG filter types, 5 per row
SIGNATURE = b"\x89PNG\r\n\x1a\n"

# The code lengths of the four dynamic codes over the 286 literal / length symbols (tools/png_tables.py generates them and states the
# model; tests/test_png_host.py holds these literals to it).
CODE_LENGTHS = (
    (
        2, 3, 3, 4, 6, 7, 7, 9, 9, 10, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 10, 9, 8, 7, 6, 5, 4, 3, 3,
        13, 8, 9, 9, 10, 10, 10, 11, 12, 13, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 7,
    ),
    (
        3, 3, 4, 4, 5, 5, 5, 6, 6, 7, 7, 8, 8, 8, 9, 9, 10, 10, 11, 11, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 13, 11, 11, 10, 10, 9, 9, 8, 8, 8, 7, 7, 6, 6, 5, 5, 4, 4, 4, 3,
        11, 8, 9, 10, 10, 11, 11, 11, 11, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 7,
    ),
    (
        4, 4, 4, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 10, 10,
        10, 10, 10, 10, 11, 11, 11, 11, 11, 12, 12, 12, 13, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 12, 12, 12, 12, 11, 11, 11, 11, 11, 10, 10, 10,
        10, 10, 10, 9, 9, 9, 9, 9, 8, 8, 8, 8, 8, 8, 7, 7, 7, 7, 7, 6, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 4, 4,
        11, 8, 9, 10, 10, 10, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 7,
    ),
    (
        5, 5, 5, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8,
        8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 10,
        10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12,
        13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15,
        15, 15, 15, 15, 15, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13,
        13, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 10, 10, 10, 10, 10,
        10, 10, 10, 10, 10, 10, 10, 10, 10, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8,
        8, 8, 8, 8, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 5, 5,
        11, 8, 9, 10, 10, 10, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 13, 13, 13, 13, 13, 13, 13, 13, 7,
    ),
)
FIXED_LENGTHS = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8      # RFC 1951 3.2.6 (288 symbols: 286 and 287 take part in the code)
# the length symbol 257 + i codes matches from LENGTH_BASE[i] on, with LENGTH_EXTRA[i] further bits (RFC 1951 3.2.5)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _reverse(code, n):
    return int(format(code, f"0{n}b")[::-1], 2) if n else 0


def canonical_codes(lengths):
    """Code lengths -> the codes of RFC 1951 3.2.2, bit-reversed (the stream is LSB-first, Huffman codes go in MSB-first)."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for n in lengths:
        out.append(_reverse(nxt[n], n))
        nxt[n] += n > 0
    return out


class _Bits:
    """An LSB-first bit string."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        self.acc |= value << self.n
        self.n += n

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _prefix(lengths):
    """The constant bits in front of a dynamic block's tokens: BFINAL = 0, BTYPE = 10, HLIT = 286 codes, HDIST = 1 code, HCLEN = 19, a
    code-length code that gives the lengths 0..15 four bits each (16, 17 and 18 are unused), the 286 lengths, and the one distance code
    of length 1."""
    b = _Bits()
    b.put(0, 1)
    b.put(2, 2)
    b.put(286 - 257, 5)
    b.put(0, 5)
    b.put(19 - 4, 4)
    for sym in _CL_ORDER:
        b.put(4 if sym < 16 else 0, 3)
    for n in tuple(lengths) + (1,):
        b.put(_reverse(n, 4), 4)
    return b


def png_tables():
    """The T = ``TABLES`` candidate codes as the encoder reads them: a list of dicts with ``lit`` [257] (value, bits) of the literals and
    end of block, ``match`` {m: (value, bits)} for m in 3..258 (the length symbol's code, its extra bits above it, and the distance
    symbol 0 -- zeros -- counted in ``bits``), and ``prefix`` (value, bits).  Table 0 is the fixed code."""
    out = []
    for t in range(TABLES):
        lengths = FIXED_LENGTHS if t == 0 else CODE_LENGTHS[t - 1]
        codes = canonical_codes(lengths)
        dist_bits = 5 if t == 0 else 1
        match = {}
        for i, (base, extra) in enumerate(zip(LENGTH_BASE, LENGTH_EXTRA)):
            for e in range(1 << extra):
                m = base + e
                if m <= 258 and (i == 28 or m < LENGTH_BASE[i + 1]):
                    match[m] = (codes[257 + i] | e << lengths[257 + i], lengths[257 + i] + extra + dist_bits)
        assert len(match) == 256 and match[258] == (codes[285], lengths[285] + dist_bits)       # (258: symbol 285, not 284 + 31)
        if t == 0:
            prefix = (2, 3)                                       # BFINAL = 0, BTYPE = 01
        else:
            b = _prefix(lengths)
            prefix = (b.acc, b.n)
        out.append(dict(lit=[(codes[s], lengths[s]) for s in range(257)], match=match, prefix=prefix, lengths=tuple(lengths)))
    return out


_TABLES = None


def _tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = png_tables()
    return _TABLES


_CRC_POLY = 0xEDB88320


def _crc_mul(a, b):
    """a(x) b(x) modulo the CRC-32 polynomial, reflected (zlib's multmodp)."""
    p, m = 0, 1 << 31
    while True:
        if a & m:
            p ^= b
            if a & (m - 1) == 0:
                return p
        m >>= 1
        b = (b >> 1) ^ _CRC_POLY if b & 1 else b >> 1


def device_tables():
    """The ``SG_PNG_TABLE_WORDS`` 32-bit words ``sg_png_encode_frames`` reads (include/sings_png.h): per table ``value << 8 | bits`` of
    the 256 literals, end of block and the 256 match lengths; per table the bit count of its block prefix and the bits; the CRC-32
    byte table; x^(8 2^j) modulo the CRC polynomial for j < ``POW_WORDS``."""
    w = np.zeros(TABLE_WORDS, dtype=np.uint32)
    for t, tab in enumerate(_tables()):
        base = t * TABLE_STRIDE
        for s, (value, bits) in enumerate(tab["lit"]):
            w[base + s] = value << 8 | bits
        for m, (value, bits) in tab["match"].items():
            w[base + 257 + m - 3] = value << 8 | bits
        value, bits = tab["prefix"]
        assert bits <= 32 * (PREFIX_STRIDE - 1)
        at = T_PREFIX + t * PREFIX_STRIDE
        w[at] = bits
        for i in range((bits + 31) // 32):
            w[at + 1 + i] = (value >> (32 * i)) & 0xFFFFFFFF
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ _CRC_POLY if c & 1 else c >> 1
        w[T_CRC + i] = c
    p = 0x00800000                                                # x^8
    for j in range(POW_WORDS):
        w[T_POW + j] = p
        p = _crc_mul(p, p)
    return w


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def _check_geometry(W, H, rows_per_segment):
    W, H = int(W), int(H)
    if not (1 <= W <= MAX_WIDTH and 1 <= H <= MAX_HEIGHT):
        raise ValueError(f"a PNG frame is 1..{MAX_WIDTH} pixels wide and 1..{MAX_HEIGHT} high, got {W} x {H}")
    rps = max(1, 16384 // (1 + 3 * W)) if rows_per_segment is None else int(rows_per_segment)
    if rps < 1 or min(rps, H) * (1 + 3 * W) > MAX_SEGMENT_BYTES:
        raise ValueError(f"rows_per_segment = {rows_per_segment!r}: a segment holds 1..{MAX_SEGMENT_BYTES} bytes, a scanline here is "
                         f"{1 + 3 * W}")
    return W, H, rps


def _check_filter(filter):
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
    return FILTERS.index(filter)


def png_header(W, H):
    """The ``HEADER_BYTES`` in front of the segments: signature, IHDR (8-bit RGB, no interlace) and an IDAT that holds the zlib header
    78 01."""
    W, H, _ = _check_geometry(W, H, 1)
    return SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", b"\x78\x01")


# ---- the numpy twin
def filter_scanlines(frame, filter="adaptive"):
    """uint8 [H,W,3] RGB -> (scanlines uint8 [H, 1 + 3 W], filter type per row).  bpp = 3; the row above the first is zeros; adaptive:
    per row the type with the smallest sum of |filtered byte as int8|, ties to the lowest type."""
    f = _check_filter(filter)
    H, W = frame.shape[:2]
    x = frame.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, 3:] = b[:, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)      # [5, H, 3W]
    if f < 5:
        types = np.full(H, f, dtype=np.int64)
    else:
        cost = np.abs(cand.view(np.int8).astype(np.int64)).sum(axis=2)                     # [5, H]
        types = np.argmin(cost, axis=0)                                                    # (the first of equal minima)
    out = np.empty((H, 1 + 3 * W), dtype=np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(H)]
    return out, types


def segment_tokens(data):
    """The bytes of one segment -> its tokens, zlib's RLE strategy in closed form: per maximal run of equal bytes the literal, then of
    the m = L - 1 further bytes matches of 258 while m >= 258, a match of m if m >= 3, else m literals.  A token is ("lit", v) or
    ("match", m); the end-of-block symbol is not listed."""
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1, [len(d)]])
    out = []
    for s, e in zip(starts[:-1].tolist(), starts[1:].tolist()):
        v, m = int(d[s]), e - s - 1
        out.append(("lit", v))
        out.extend([("match", 258)] * (m // 258))
        m %= 258
        out.extend([("match", m)] if m >= 3 else [("lit", v)] * m)
    return out


def _encode_segment(data, force, log):
    tokens = segment_tokens(data)
    n = len(data)
    tabs = _tables()
    sizes = []
    for tab in tabs:
        bits = tab["prefix"][1] + tab["lit"][256][1]
        bits += sum(tab["lit"][v][1] if kind == "lit" else tab["match"][v][1] for kind, v in tokens)
        sizes.append((bits + 3 + 7) // 8 + 4)
    sizes.append(n + 5)
    c = sizes.index(min(sizes)) if force < 0 else force
    if log is not None:
        log["candidates"].append(c)
        log["tokens"].append(tokens)
        log["sizes"].append(tuple(sizes))
    if c == TABLES:
        return b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(data)
    tab = tabs[c]
    b = _Bits()
    b.put(*tab["prefix"])
    for kind, v in tokens:
        b.put(*(tab["lit"][v] if kind == "lit" else tab["match"][v]))
    b.put(*tab["lit"][256])
    b.put(0, 3)                                                   # an empty stored block: byte aligned, not final
    out = b.bytes() + b"\x00\x00\xff\xff"
    assert len(out) == sizes[c]
    return out


def png_encode_host(frames_u8, filter="adaptive", rows_per_segment=None, bgr=False, force=-1, log=None):
    """The numpy twin of ``PngEncoder``: uint8 [K,H,W,3] (or one [H,W,3]) -> a list of K ``bytes``, each a complete PNG file, the same
    bytes the device path writes.  ``log``: a dict that receives, over all frames, ``candidates`` (the candidate of every segment: 0
    fixed, 1..4 dynamic, 5 stored), ``filters`` (the filter type of every row), ``tokens`` and ``sizes`` (per segment: its tokens, the
    bytes of every candidate) and ``scanlines`` (per frame: the filtered scanlines), for tests."""
    frames = np.asarray(frames_u8)
    if frames.dtype != np.uint8 or frames.ndim not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError(f"png_encode_host: uint8 [K,H,W,3] or [H,W,3] expected, got {frames.dtype} {frames.shape}")
    if frames.ndim == 3:
        frames = frames[None]
    H, W = frames.shape[1:3]
    W, H, rps = _check_geometry(W, H, rows_per_segment)
    _check_filter(filter)
    force = int(force)
    if not -1 <= force <= TABLES:
        raise ValueError(f"force = {force} outside -1..{TABLES}")
    if log is not None:
        for key in ("candidates", "filters", "tokens", "sizes", "scanlines"):
            log.setdefault(key, [])
    header = png_header(W, H)
    out = []
    for frame in frames:
        lines, types = filter_scanlines(frame[..., ::-1] if bgr else frame, filter)
        if log is not None:
            log["filters"].extend(int(t) for t in types)
            log["scanlines"].append(lines.tobytes())
        data = [header]
        for r0 in range(0, H, rps):
            data.append(_chunk(b"IDAT", _encode_segment(lines[r0:r0 + rps].tobytes(), force, log)))
        data.append(_chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", zlib.adler32(lines.tobytes()))))
        data.append(_chunk(b"IEND", b""))
        out.append(b"".join(data))
    return out


# ---- the device encoder
class PngEncoder(_FrameEncoder):
    """K frames of W x H, uint8 RGB (or BGR), to K PNG files per call (``sg_png_encode_frames``: filter pass, deflate pass, scan and
    gather, on torch's current stream or ``stream``).  Everything is allocated here: ``encode`` allocates and synchronises nothing, so
    it may be captured into a graph.  ``capacity``: bytes per frame of the output; the default is the largest file a frame can
    become, so nothing ever overflows it.  With a smaller capacity a frame that needs more reports ``sizes[k] = -needed`` and writes
    nothing (so does a frame whose forced candidate outgrows the default), and ``encode_to_host`` raises RuntimeError."""
    _INCLUDE, _FLAG, _TWIN, _DEFAULT_CAPACITY = "sings_png.h", "HAS_PNG", "png_encode_host", "worst_bytes"

    def __init__(self, W, H, K, device, filter="adaptive", rows_per_segment=None, capacity=None):
        self.W, self.H, self.rows_per_segment = _check_geometry(W, H, rows_per_segment)
        self.filter = filter
        self._filter = _check_filter(filter)
        super().__init__(K, device, capacity)

    def _describe(self):
        from . import _marshal
        header = png_header(self.W, self.H)
        return header, device_tables(), _marshal.png_layout(self.W, self.H, self.K, self.rows_per_segment, len(header))

    def _launch(self, k, frames, bgr, buf, sizes, stream, force=-1):
        from . import _marshal
        if not -1 <= int(force) <= TABLES:
            raise ValueError(f"PngEncoder.encode: force = {force} outside -1..{TABLES}")
        _marshal.png_encode_frames(k, self.W, self.H, self.rows_per_segment, self._filter, bgr, int(force), frames, self._tables,
                                   self._header, self._ws, buf, int(buf.shape[1]), sizes, stream)

    def encode(self, frames_u8, bgr=False, stream=None, force=-1, out=None):
        """``_FrameEncoder.encode``; ``force``: -1, or the candidate every segment takes."""
        return super().encode(frames_u8, bgr, stream, out, force=force)

    def encode_to_host(self, frames_u8, bgr=False, force=-1):
        """``_FrameEncoder.encode_to_host``: RuntimeError when a frame does not fit ``capacity`` (a capacity of the caller's, or a
        forced candidate)."""
        return super().encode_to_host(frames_u8, bgr, force=force)


def write_atomic(path, data):
    """``data`` to ``path`` under a temporary name beside it, then renamed: no partial file is ever seen under ``path``."""
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def animate_to_frames(dirname, canon, poses, joints_rest, A_t2cano, cameras, bg_color, pattern="{:05d}.png", frames_per_launch=8,
                      **kwargs):
    """``posed.animate_chunk(..., out="png")`` into ``dirname``/``pattern.format(f)``, one lossless file per frame: the reference's
    ``animate(keep_images=True)`` without a host PNG writer.  ``kwargs``: ``animate_chunk``'s other arguments (transl, smpl_scale,
    ext_tfs, parents, streams, animator).  Every file is written under a temporary name and renamed.  Returns the number of frames
    written."""
    pattern = str(pattern)
    if pattern.format(0) == pattern.format(1) or os.path.basename(pattern.format(0)) != pattern.format(0):
        raise ValueError(f"animate_to_frames: pattern = {pattern!r} must be a file name with a field for the frame's number")
    for key in ("out", "return_aux"):
        if key in kwargs:
            raise TypeError(f"animate_to_frames: {key} is not an argument here (the frames go to files)")
    from .posed import animate_chunk
    os.makedirs(dirname, exist_ok=True)
    n = 0
    for f, data in animate_chunk(canon, poses, joints_rest, A_t2cano, cameras, bg_color, frames_per_launch=frames_per_launch,
                                 out="png", **kwargs):
        write_atomic(os.path.join(dirname, pattern.format(f)), data)
        n += 1
    return n
