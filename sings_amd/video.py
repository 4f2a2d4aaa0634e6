"""Frames out as JPEG streams encoded on the device, and Motion-JPEG video.

The reference turns its animation frames into a video by shelling out to ffmpeg (``create_video``, utils/general.py:36).  Here the
K uint8 frames an animation launch already produces (``frame_out.frames_to_u8``) are encoded to K complete baseline JPEG files by four
HIP launches (``sg_jpeg_encode_frames``, include/sings_jpeg.h), read back in one copy, and wrapped into an AVI by a small host writer.

 * ``JpegEncoder`` (on ``codec._FrameEncoder``): pre-allocated workspaces for K frames of W x H; ``encode`` (device buffers, legal
   inside a graph capture) and ``encode_to_host`` (a list of ``bytes``; a frame that does not fit its capacity grows the buffer and is encoded again).
 * ``jpeg_encode_host``: the numpy twin -- the same stream, byte for byte, without a device.  It is the restatement the device path
   is tested against, not a fallback: nothing in the product calls it.
 * ``MjpegWriter``: RIFF AVI 1.0 with one ``MJPG`` video stream, written atomically, below 2 GiB (no OpenDML).
 * ``animate_to_video``: ``posed.animate_chunk(out="jpeg")`` into an ``MjpegWriter`` -- the reference's ``animate_chunk(save_video=True)``.

The stream is fixed so that bytes can be compared: baseline sequential DCT (SOF0), 8 bit, Y/Cb/Cr at 4:4:4 (an MCU is one 8 x 8 pixel
block: a Y, a Cb and a Cr coefficient block), the Annex K tables scaled by libjpeg's quality rule, a DRI segment always, restart
markers every ``restart_interval`` MCUs (default: one MCU row).  The arithmetic is pinned: fp32, every multiply and add rounded on
its own, sums left to right, quantisation ``rint(F / Q)`` with ties to even.  Out of scope: chroma subsampling, progressive streams,
optimised Huffman tables, mp4 / H.264, audio (lossless files: sings_amd/png.py).
"""
import math
import os
import struct
from fractions import Fraction

import numpy as np

from .codec import MAX_FRAMES, _FrameEncoder       # MAX_FRAMES: SG_JPEG_MAX_FRAMES

# ---- the Annex K tables, as a non-optimised libjpeg file at quality 50 carries them (tests/golden/gen_jpeg_tables.py reads such a
# file into tests/golden/jpeg_tables.npz; tests/test_video_host.py holds these literals to it).  Quantisation: zig-zag order.
QUANT_LUMA = (
    16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37,
    29, 40, 58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87,
    95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99,
)
QUANT_CHROMA = (
    17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
)
# Huffman tables: BITS (codes of length 1..16) and the symbols in code order
DC0_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC0_VALS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
AC0_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
AC0_VALS = (
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8,
    35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40,
    41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
    90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137,
    138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182,
    183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
    227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250,
)
DC1_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC1_VALS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
AC1_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)
AC1_VALS = (
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145,
    161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38,
    39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
    89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135,
    136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
    181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
    226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250,
)
HUFFMAN = (("dc0", DC0_BITS, DC0_VALS), ("ac0", AC0_BITS, AC0_VALS), ("dc1", DC1_BITS, DC1_VALS), ("ac1", AC1_BITS, AC1_VALS))

MAX_DIM = 65535                      # SG_JPEG_MAX_DIM: a SOF0 dimension is 16 bit
TABLE_WORDS = 800                    # SG_JPEG_TABLE_WORDS: basis 64 | quantisers 2 x 64 | zig-zag position 64 | Huffman 2 x 272
HUFF_STRIDE = 272                    # SG_JPEG_HUFF_STRIDE: 16 DC categories, then the 256 AC run/size symbols


def _zigzag():
    """ZIGZAG[i]: the natural index (8 v + u) of the i-th coefficient in zig-zag order."""
    order = sorted(range(64), key=lambda n: (n // 8 + n % 8, (n // 8) if (n // 8 + n % 8) % 2 else (n % 8)))
    return np.array(order, dtype=np.int64)


ZIGZAG = _zigzag()


def dct_basis():
    """C[u][x] = fp32(a(u) / 2 * cos((2 x + 1) u pi / 16)), a(0) = 1 / sqrt(2): computed in fp64, rounded once.  The one source of
    the basis: the twin uses this array and the device an upload of it."""
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    a = np.where(u == 0, 1.0 / math.sqrt(2.0), 1.0)
    return (a / 2.0 * np.cos((2.0 * x + 1.0) * u * math.pi / 16.0)).astype(np.float32)


def quant_tables(quality):
    """libjpeg's quality rule on the Annex K tables -> (luma, chroma) [64] uint8 in zig-zag order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be in 1..100, got {quality!r}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(base, dtype=np.int64) * scale + 50) // 100, 1, 255).astype(np.uint8)
                 for base in (QUANT_LUMA, QUANT_CHROMA))


def huffman_codes(bits, vals):
    """BITS / symbols -> {symbol: (code, length)}, the canonical assignment."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


_CODES = {name: huffman_codes(bits, vals) for name, bits, vals in HUFFMAN}


def _check_geometry(W, H, restart_interval):
    W, H = int(W), int(H)
    if not (1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM):
        raise ValueError(f"a JPEG frame is 1..{MAX_DIM} pixels wide and high, got {W} x {H}")
    ri = (W + 7) // 8 if restart_interval is None else int(restart_interval)
    if not 1 <= ri <= 65535:
        raise ValueError(f"restart_interval must be in 1..65535 MCUs, got {restart_interval!r} (default: one MCU row; "
                         f"{(W + 7) // 8} here)")
    return W, H, ri


def jpeg_header(W, H, quality, restart_interval=None):
    """The fixed bytes in front of the entropy-coded data: SOI, APP0 (JFIF 1.01), DQT 0, DQT 1, SOF0, DHT DC0 / AC0 / DC1 / AC1, DRI,
    SOS."""
    W, H, ri = _check_geometry(W, H, restart_interval)
    ql, qc = quant_tables(quality)
    seg = lambda marker, payload: bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload
    out = b"\xff\xd8"
    out += seg(0xE0, b"JFIF\x00" + bytes((1, 1, 0)) + struct.pack(">HH", 1, 1) + bytes((0, 0)))
    out += seg(0xDB, bytes((0,)) + ql.tobytes())
    out += seg(0xDB, bytes((1,)) + qc.tobytes())
    out += seg(0xC0, bytes((8,)) + struct.pack(">HH", H, W) + bytes((3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for name, bits, vals in HUFFMAN:
        out += seg(0xC4, bytes(((0x10 if name[0] == "a" else 0) | int(name[2]),)) + bytes(bits) + bytes(vals))
    out += seg(0xDD, struct.pack(">H", ri))
    out += seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))
    return out


def device_tables(quality):
    """The ``SG_JPEG_TABLE_WORDS`` 32-bit words ``sg_jpeg_encode_frames`` reads (include/sings_jpeg.h): the DCT basis (fp32, C[u][x] at
    8 u + x), the two quantisers (fp32, natural order), the zig-zag position of every natural index (int32), and per table class
    (0: DC0 / AC0, 1: DC1 / AC1) ``code << 8 | length`` of the 16 DC categories and the 256 AC symbols (0: no such symbol)."""
    t = np.zeros(TABLE_WORDS, dtype=np.uint32)
    t[0:64] = dct_basis().reshape(64).view(np.uint32)
    pos = np.empty(64, dtype=np.int64)
    pos[ZIGZAG] = np.arange(64)
    for c, q in enumerate(quant_tables(quality)):
        nat = np.empty(64, dtype=np.float32)
        nat[ZIGZAG] = q.astype(np.float32)
        t[64 + 64 * c:128 + 64 * c] = nat.view(np.uint32)
    t[192:256] = pos.astype(np.uint32)
    for c in (0, 1):
        base = 256 + HUFF_STRIDE * c
        for sym, (code, length) in _CODES[f"dc{c}"].items():
            t[base + sym] = code << 8 | length
        for sym, (code, length) in _CODES[f"ac{c}"].items():
            t[base + 16 + sym] = code << 8 | length
    return t


# ---- the numpy twin
_F = np.float32


def jpeg_coefficients(frame, quality):
    """One uint8 [H,W,3] RGB frame -> int32 [rows of blocks, blocks per row, 3, 64]: the quantised coefficients in zig-zag order,
    by the pinned arithmetic (module docstring)."""
    H, W = frame.shape[:2]
    by, bx = (H + 7) // 8, (W + 7) // 8
    px = np.pad(frame, ((0, by * 8 - H), (0, bx * 8 - W), (0, 0)), mode="edge").astype(np.float32)
    R, G, B = px[..., 0], px[..., 1], px[..., 2]
    Y = ((_F(0.299) * R + _F(0.587) * G) + _F(0.114) * B) - _F(128.0)
    Cb = ((_F(-0.168736) * R) + (_F(-0.331264) * G)) + _F(0.5) * B
    Cr = (_F(0.5) * R + (_F(-0.418688) * G)) + (_F(-0.081312) * B)
    s = np.stack([Y, Cb, Cr]).reshape(3, by, 8, bx, 8).transpose(1, 3, 0, 2, 4)      # [by, bx, 3, y, x]
    C = dct_basis()
    t = s[..., :, 0, None] * C[:, 0]                              # rows: t[y][u] = sum_x C[u][x] s[y][x], x ascending
    for x in range(1, 8):
        t = t + s[..., :, x, None] * C[:, x]
    F = C[:, 0, None] * t[..., None, 0, :]                        # columns: F[v][u] = sum_y C[v][y] t[y][u]
    for y in range(1, 8):
        F = F + C[:, y, None] * t[..., None, y, :]
    assert F.dtype == np.float32
    ql, qc = quant_tables(quality)
    Q = np.empty((3, 64), dtype=np.float32)
    Q[0, ZIGZAG], Q[1, ZIGZAG] = ql, qc
    Q[2] = Q[1]
    q = np.rint(F.reshape(by, bx, 3, 64) / Q).astype(np.int32)
    q[..., 0] = np.clip(q[..., 0], -1024, 1023)
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q[..., ZIGZAG]


def _magnitude(v):
    """A coefficient (or DC difference) -> (category, its magnitude bits: one's complement for negatives)."""
    n = abs(v).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def _entropy_segment(blocks, symbol_log):
    """The coefficient blocks [n MCUs, 3, 64] of one restart segment -> its bytes: padded with 1-bits, 0xFF followed by 0x00."""
    acc, nbits = 0, 0
    pred = [0, 0, 0]
    for mcu in blocks:
        for c in range(3):
            dc, ac = _CODES["dc0" if c == 0 else "dc1"], _CODES["ac0" if c == 0 else "ac1"]
            b = mcu[c]
            n, bits = _magnitude(int(b[0]) - pred[c])
            pred[c] = int(b[0])
            code, length = dc[n]
            acc, nbits = (acc << length | code) << n | bits, nbits + length + n
            last = 0
            for i in np.flatnonzero(b[1:]) + 1:
                run = int(i) - last - 1
                last = int(i)
                while run >= 16:
                    code, length = ac[0xF0]
                    acc, nbits = acc << length | code, nbits + length
                    run -= 16
                    if symbol_log is not None:
                        symbol_log.append(0xF0)
                n, bits = _magnitude(int(b[i]))
                code, length = ac[run << 4 | n]
                acc, nbits = (acc << length | code) << n | bits, nbits + length + n
                if symbol_log is not None:
                    symbol_log.append(run << 4 | n)
            if last != 63:
                code, length = ac[0x00]
                acc, nbits = acc << length | code, nbits + length
                if symbol_log is not None:
                    symbol_log.append(0x00)
    pad = -nbits % 8
    acc, nbits = acc << pad | ((1 << pad) - 1), nbits + pad
    return acc.to_bytes(nbits // 8, "big").replace(b"\xff", b"\xff\x00")


def jpeg_encode_host(frames_u8, quality=90, restart_interval=None, bgr=False, symbol_log=None):
    """The numpy twin of ``JpegEncoder``: uint8 [K,H,W,3] (or one [H,W,3]) -> a list of K ``bytes``, each a complete JPEG file, the
    same bytes the device path writes.  ``symbol_log``: a list that receives every AC symbol coded (run << 4 | size; 0xF0 ZRL, 0x00
    EOB), for tests."""
    frames = np.asarray(frames_u8)
    if frames.dtype != np.uint8 or frames.ndim not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError(f"jpeg_encode_host: uint8 [K,H,W,3] or [H,W,3] expected, got {frames.dtype} {frames.shape}")
    if frames.ndim == 3:
        frames = frames[None]
    H, W = frames.shape[1:3]
    W, H, ri = _check_geometry(W, H, restart_interval)
    header = jpeg_header(W, H, quality, ri)
    out = []
    for frame in frames:
        q = jpeg_coefficients(frame[..., ::-1] if bgr else frame, quality).reshape(-1, 3, 64)
        nseg = (len(q) + ri - 1) // ri
        data = [header]
        for s in range(nseg):
            data.append(_entropy_segment(q[s * ri:(s + 1) * ri], symbol_log))
            data.append(b"\xff\xd9" if s == nseg - 1 else bytes((0xFF, 0xD0 + s % 8)))
        out.append(b"".join(data))
    return out


# ---- the device encoder
class JpegEncoder(_FrameEncoder):
    """K frames of W x H, uint8 RGB (or BGR), to K baseline JPEG files per call (``sg_jpeg_encode_frames``: block pass, entropy pass,
    scan and gather, on torch's current stream or ``stream``).  Everything is allocated here: ``encode`` allocates and synchronises
    nothing, so it may be captured into a graph.  ``capacity``: bytes per frame of the output (default: header + H W 3 / 2); a frame
    that needs more reports ``sizes[k] = -needed`` and writes nothing, and ``encode_to_host`` grows the buffer and encodes again (at
    most twice, RuntimeError after that)."""
    _INCLUDE, _FLAG, _TWIN, _DEFAULT_CAPACITY, _GROWS = "sings_jpeg.h", "HAS_JPEG", "jpeg_encode_host", "default_capacity", True

    def __init__(self, W, H, K, device, quality=90, restart_interval=None, capacity=None):
        self.W, self.H, self.ri = _check_geometry(W, H, restart_interval)
        self.quality = int(quality)
        super().__init__(K, device, capacity)

    def _describe(self):
        from . import _marshal
        header = jpeg_header(self.W, self.H, self.quality, self.ri)
        return header, device_tables(self.quality), _marshal.jpeg_layout(self.W, self.H, self.K, self.ri, len(header))

    def _launch(self, k, frames, bgr, buf, sizes, stream):
        from . import _marshal
        _marshal.jpeg_encode_frames(k, self.W, self.H, self.ri, bgr, frames, self._tables, self._header, self._ws, buf, int(buf.shape[1]),
                                    sizes, stream)


# ---- Motion-JPEG in a RIFF AVI
class MjpegWriter:
    """``write(jpeg_bytes)`` per frame, ``close()`` at the end (or use it as a context manager): a RIFF AVI 1.0 file -- ``hdrl`` with
    ``avih`` and one ``strl`` (``strh`` vids / MJPG, ``strf`` a BITMAPINFOHEADER), ``movi`` of ``00dc`` chunks, ``idx1``.  Frame count
    and sizes are patched in on close.  The file is written under a temporary name beside ``path`` and renamed on close; an
    exception inside the ``with`` block (or ``abort()``) leaves nothing under ``path``.  AVI 1.0 ends below 2 GiB: ``write`` raises
    before the file would pass ``MAX_BYTES`` (OpenDML is out of scope)."""

    MAX_BYTES = 2 ** 31 - 1
    _MOVI_AT = 12 + 8 + 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))          # where the LIST chunk of 'movi' starts

    def __init__(self, path, W, H, fps):
        self.path, self.W, self.H = str(path), int(W), int(H)
        rate = Fraction(fps).limit_denominator(10000)
        if rate <= 0 or not (1 <= self.W <= MAX_DIM and 1 <= self.H <= MAX_DIM):
            raise ValueError(f"MjpegWriter: fps = {fps!r}, W = {W}, H = {H}")
        self.rate, self.scale = rate.numerator, rate.denominator
        self.usec = int(round(1e6 * self.scale / self.rate))
        self._tmp = f"{self.path}.{os.getpid()}.tmp"
        self._f = open(self._tmp, "wb")
        self._index = []                                          # (offset from the 'movi' fourcc, payload bytes)
        self._f.write(self._headers(0, 0))
        self._bytes = self._f.tell()
        assert self._bytes == self._MOVI_AT + 12

    def _headers(self, frames, largest, riff_size=0, movi_size=4):
        bps = 0 if not frames else int(sum(n for _, n in self._index) * self.rate / (self.scale * frames))
        avih = struct.pack("<14I", self.usec, bps, 0, 0x10, frames, 0, 1, largest, self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, frames, largest, 0xFFFFFFFF, 0,
                           0, 0, self.W, self.H)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        chunk = lambda tag, data: tag + struct.pack("<I", len(data)) + data
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf)
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + chunk(b"avih", avih) + strl
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_size) + b"movi"

    def _final_bytes(self, extra_payload):
        """The file's size if a frame of ``extra_payload`` bytes were written and the file closed."""
        return self._bytes + 8 + extra_payload + (extra_payload & 1) + 8 + 16 * (len(self._index) + 1)

    def write(self, jpeg_bytes):
        if self._f is None:
            raise ValueError("MjpegWriter: write after close")
        data = bytes(jpeg_bytes)
        if self._final_bytes(len(data)) > self.MAX_BYTES:
            raise RuntimeError(f"MjpegWriter: {self.path} would pass {self.MAX_BYTES} bytes, the end of a RIFF AVI 1.0 file (OpenDML "
                               "is not written): close this file and start another")
        self._index.append((self._bytes - (self._MOVI_AT + 8), len(data)))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b""))
        self._bytes += 8 + len(data) + (len(data) & 1)

    @property
    def frames(self):
        return len(self._index)

    def close(self):
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            movi_end = self._bytes
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            for off, n in self._index:
                f.write(b"00dc" + struct.pack("<III", 0x10, off, n))
            total = movi_end + 8 + 16 * len(self._index)
            f.seek(0)
            f.write(self._headers(len(self._index), max((n for _, n in self._index), default=0), total - 8,
                                  movi_end - (self._MOVI_AT + 8)))
            f.close()
            os.replace(self._tmp, self.path)
        except BaseException:
            f.close()
            if os.path.exists(self._tmp):
                os.remove(self._tmp)
            raise

    def abort(self):
        """Drops the file: nothing appears under ``path``."""
        if self._f is not None:
            self._f.close()
            self._f = None
            if os.path.exists(self._tmp):
                os.remove(self._tmp)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()
        return False


def _write_video(path, cameras, fps, frames):
    """``frames``: an iterable of (index, JPEG ``bytes``), in order, of the size of ``cameras`` (one camera dict or a list: the first
    one's) -> a Motion-JPEG AVI at ``path``.  Returns the number of frames written."""
    cam = cameras[0] if isinstance(cameras, (list, tuple)) else cameras
    with MjpegWriter(path, int(cam["image_width"]), int(cam["image_height"]), fps) as w:
        for _, data in frames:
            w.write(data)
        return w.frames


def animate_to_video(path, canon, poses, joints_rest, A_t2cano, cameras, bg_color, fps=20, quality=90, frames_per_launch=8, **kwargs):
    """``posed.animate_chunk(..., out=("jpeg", quality))`` into a Motion-JPEG AVI at ``path``: the reference's ``animate_chunk(save_video=True)``
    without ffmpeg.  ``kwargs``: ``animate_chunk``'s other arguments (transl, smpl_scale, ext_tfs, parents, streams, animator).
    Returns the number of frames written."""
    from .posed import animate_chunk
    return _write_video(path, cameras, fps, animate_chunk(canon, poses, joints_rest, A_t2cano, cameras, bg_color,
                                                          frames_per_launch=frames_per_launch, out=("jpeg", int(quality)), **kwargs))
