"""The PNG files and zlib streams the decode tests read (tests/test_unpng_host.py and tests/test_inflate_sanitized.py on the CPU,
tests/test_gpu_unpng.py against the device), built once per process, and the twin's results of them, computed once.

VALID: (name, file bytes) -- complete PNG files, so PIL can say what their pixels are:
  (a) every frame of every case of tests/png_case.py through the twin encoder ``png.png_encode_host``: every filter type forced, the
      adaptive mix, segments, scanlines of 64, 67 and 256 bytes;
  (b) ``zlib.compressobj`` over the filtered scanlines of ``png_case.body`` pictures at 1x1, 21x13, 22x9, 85x7 and 200x120 with 1, 3 and
      4 bytes per pixel (row y has filter type y % 5): level 0 (at 200x120 RGB 72 120 raw bytes: two stored blocks), Z_FIXED, level 1
      with Z_RLE (cv2's kind of stream), level 9, memLevel 1 (many short dynamic blocks), wbits 9;
  (c) hand-written streams of the fixed code (``FixedWriter``) with what zlib never emits: see ``handmade``, and
      ``beyond_declared_window`` for distances past the window its zlib header declares (zlib reads them, so the decoder does);
  (e) the kit files under tests/golden/.
CORRUPT: (name, stream, the status its name stands for, inflate-level?) -- all of them streams of an 85 x 7 RGB picture
(``CORRUPT_SHAPE``; 1792 raw bytes), so that one device call can hold them all.  An inflate-level case is one zlib.decompress judges
too; the others (a raw length that is not the picture's, a filter byte of 5) are the PNG's business.
``write_kit``: a training kit of 24 frames of 22 x 9 written with PIL, for the loader's tests.
"""
import os
import struct
import zlib

import numpy as np

import png_case as pc
from sings_amd import unpng as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KIT_FILES = ("kit_mask_000000.png", "kit_mask_000040.png", "kit_image_000040.png")
SIZES = ((1, 1), (21, 13), (22, 9), (85, 7), (200, 120))           # (W, H)
CORRUPT_SHAPE = (85, 7, 3)                                          # W, H, channels
_COLOUR = {1: 0, 3: 2, 4: 6}


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(W, H, ch, stream, cut=None):
    """A PNG file around a zlib stream; ``cut``: the stream in two IDAT chunks, the first of ``cut`` bytes."""
    idat = _chunk(b"IDAT", stream) if cut is None else _chunk(b"IDAT", stream[:cut]) + _chunk(b"IDAT", stream[cut:])
    return U.SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, _COLOUR[ch], 0, 0, 0)) + idat + _chunk(b"IEND", b"")


def picture(W, H, ch, seed=3):
    """uint8 [H,W,ch]: ``png_case.body`` (grey: its first channel; RGBA: an alpha ramp behind it)."""
    rgb = pc.body(H, W, 6, seed)
    if ch == 1:
        return rgb[..., :1].copy()
    if ch == 3:
        return rgb
    y, x = np.mgrid[0:H, 0:W]
    return np.concatenate([rgb, ((7 * x + 13 * y) & 255).astype(np.uint8)[..., None]], -1)


def filter_lines(img, types):
    """uint8 [H,W,ch] -> the filtered scanlines (bytes), row y with filter type ``types[y]``; bpp = ch."""
    H, W, ch = img.shape
    x = img.reshape(H, W * ch).astype(np.int64)
    a = np.zeros_like(x)
    a[:, ch:] = x[:, :-ch]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, ch:] = b[:, :-ch]
    p = a + b - c
    pa, pb, pcc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pcc), a, np.where(pb <= pcc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)
    out = np.empty((H, 1 + W * ch), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[np.asarray(types), np.arange(H)]
    return out.tobytes()


ZLIB_KINDS = {
    "level0": dict(level=0), "fixed": dict(level=6, strategy=zlib.Z_FIXED), "rle1": dict(level=1, strategy=zlib.Z_RLE),
    "level9": dict(level=9), "mem1": dict(level=6, memLevel=1), "wbits9": dict(level=6, wbits=9),
}


def deflate(raw, level=6, wbits=15, memLevel=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, memLevel, strategy)
    return c.compress(raw) + c.flush()


# ---- (c) a writer of the fixed code ------------------------------------------------------------------------------------------------
class FixedWriter:
    """Deflate blocks of the fixed code (and stored ones), token by token; ``out`` is what the tokens decode to."""

    def __init__(self, header=b"\x78\x01"):
        self.acc, self.n, self.data, self.out = 0, 0, bytearray(header), bytearray()

    def bits(self, v, n):                                         # LSB first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.data.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):                                         # a Huffman code: its most significant bit first
        self.bits(int(format(v, f"0{n}b")[::-1], 2), n)

    def block(self, last=0):
        self.bits(last | 2, 3)

    def symbol(self, s):                                          # literal/length symbol 0..287
        self.code(*((0x30 + s, 8) if s < 144 else (0x190 + s - 144, 9) if s < 256 else (s - 256, 7) if s < 280 else (0xC0 + s - 280, 8)))

    def lit(self, v):
        self.symbol(v)
        self.out.append(v)

    def match(self, dist, n, far=True, record=True):
        s = 285 if n == 258 and far else max(i for i in range(28) if length_base(i) <= n) + 257
        self.symbol(s)
        if s != 285:
            self.bits(n - length_base(s - 257), length_extra(s - 257))
        d = max(i for i in range(30) if dist_base(i) <= dist)
        self.code(d, 5)
        self.bits(dist - dist_base(d), max(0, d // 2 - 1))
        if record:
            for _ in range(n):
                self.out.append(self.out[-dist])

    def end(self):
        self.symbol(256)

    def stored(self, data=b"", last=0, nlen=None):
        self.bits(last, 3)
        self.bits(0, -self.n % 8)
        self.data += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + bytes(data)
        self.out += data

    def finish(self, adler=None):
        self.bits(0, -self.n % 8)
        return bytes(self.data) + struct.pack(">I", zlib.adler32(bytes(self.out)) if adler is None else adler)


def length_base(i):
    from sings_amd import png as P
    return P.LENGTH_BASE[i]


def length_extra(i):
    from sings_amd import png as P
    return P.LENGTH_EXTRA[i]


def dist_base(d):
    return d + 1 if d < 4 else 1 + ((2 + (d & 1)) << (d // 2 - 1))


def handmade():
    """-> (W, H, ch, stream): 130 identical scanlines of 256 bytes (a 255 x 130 grey picture, filter None) whose tokens are a copy at
    distance 1, 2 and 3 longer than its distance; length 258 by symbol 285; an empty stored block in mid-stream; length 3; a match at
    distance 32 768 exactly (it reaches the first byte of the output); a match at 24 577, the first distance of symbol 29."""
    row = bytearray((37 * i + 11) & 255 for i in range(256))
    row[0] = 0
    row[10:20] = bytes([7]) * 10
    row[20:32] = bytes([200, 100]) * 6
    row[32:47] = bytes([1, 2, 3]) * 5
    target = bytes(row) * 130
    w = FixedWriter()
    w.block()
    for v in row[:11]:
        w.lit(v)
    w.match(1, 9)
    w.lit(200), w.lit(100), w.match(2, 10)
    w.lit(1), w.lit(2), w.lit(3), w.match(3, 12)
    for v in row[47:]:
        w.lit(v)
    w.match(256, 258)
    w.end()
    w.stored()                                                    # empty, not final
    w.block()
    w.match(256, 3)

    def until(pos):                                               # rows repeat: distance 256 carries the output to `pos`
        while len(w.out) < pos:
            n = min(258, pos - len(w.out))
            if n >= 3:
                w.match(256, n)
            else:
                w.lit(target[len(w.out)])
    until(32768)
    w.match(32768, 3)
    until(33035)                                                  # 129 * 256 + 11: inside the run of sevens, 24 577 = 96 * 256 + 1
    w.match(24577, 3)
    until(len(target))
    w.end()
    w.block(1)
    w.end()
    assert bytes(w.out) == target
    return 255, 130, 1, w.finish()


def beyond_declared_window():
    """-> (W, H, ch, stream): 8 identical scanlines of 64 bytes (a 63 x 8 grey picture, filter None) under the zlib header ``08 1D``,
    which declares a window of 256 bytes; rows 5 and 6 are matches at distance 320 and 384, further back than that.  zlib holds the
    declared window against the distances only when built strict, so ``zlib.decompress`` and PIL read this stream: it is a VALID one."""
    row = bytes([0]) + bytes((29 * i + 5) & 255 for i in range(63))
    w = FixedWriter(header=b"\x08\x1d")
    w.block(1)
    for v in row:
        w.lit(v)
    for _ in range(4):
        w.match(64, 64)
    w.match(320, 64)
    for v in row[:1]:
        w.lit(v)
    w.match(384, 63)                                              # byte 385 from byte 1: the rest of the row, from the first one
    w.match(64, 64)
    w.end()
    assert bytes(w.out) == row * 8
    return 63, 8, 1, w.finish()


# ---- the lists ---------------------------------------------------------------------------------------------------------------------
def _valid():
    out = []
    for name, frames, _, _, _ in pc.CASES:
        for i, data in enumerate(pc.twin(name)[0]):
            out.append((f"twin-{name}-{i}", data))
    for W, H in SIZES:
        for ch in (1, 3, 4):
            raw = filter_lines(picture(W, H, ch), [y % 5 for y in range(H)])
            for kind, kw in ZLIB_KINDS.items():
                out.append((f"zlib-{W}x{H}x{ch}-{kind}", png_file(W, H, ch, deflate(raw, **kw))))
    out.append(("handmade", png_file(*handmade())))
    out.append(("handmade-beyond-declared-window", png_file(*beyond_declared_window())))
    for f in KIT_FILES:
        with open(os.path.join(GOLDEN, f), "rb") as fh:
            out.append((f, fh.read()))
    return out


def _dynamic_header(cl, symbols):
    """A final dynamic block's header: HLIT = 257, HDIST = 1, the code-length code ``cl`` {symbol: (code, bits, length)}, then
    ``symbols``: (code-length symbol, extra value, extra bits)."""
    w = FixedWriter()
    w.bits(1 | 4, 3)
    w.bits(0, 5), w.bits(0, 5), w.bits(15, 4)
    for s in U._CL_ORDER:
        w.bits(cl[s][2] if s in cl else 0, 3)
    for s, extra, n in symbols:
        w.code(cl[s][0], cl[s][1])
        w.bits(extra, n)
    return w


def _corrupt():
    W, H, ch = CORRUPT_SHAPE
    raw = filter_lines(picture(W, H, ch), [y % 5 for y in range(H)])
    good = deflate(raw, level=9)
    out = [("truncated-half", good[:len(good) // 2], U.E_INPUT, True), ("truncated-last-byte", good[:-1], U.E_INPUT, True),
           ("block-type-3", b"\x78\x01\x07", U.E_BLOCK_TYPE, True), ("zlib-header", b"\x78\x02" + good[2:], U.E_HEADER, True),
           ("wrong-adler", good[:-1] + bytes([good[-1] ^ 1]), U.E_ADLER, True)]
    w = FixedWriter()
    w.stored(raw[:5], last=1, nlen=0x1234)
    out.append(("stored-nlen", w.finish(), U.E_STORED, True))
    w = FixedWriter()
    w.block(1), w.lit(65), w.match(2, 3, record=False), w.end()
    out.append(("distance-before-start", w.finish(0), U.E_DISTANCE, True))
    w = FixedWriter()
    w.block(1), w.lit(65), w.symbol(286)
    out.append(("fixed-symbol-286", w.finish(0), U.E_LITLEN_SYMBOL, True))
    w = FixedWriter()
    w.block(1), w.lit(65), w.symbol(257), w.code(30, 5), w.end()
    out.append(("fixed-distance-30", w.finish(0), U.E_DIST_SYMBOL, True))
    # the code-length code {1: '0', 16 / 18: '1'} is complete; 258 lengths of 1 over-subscribe the literal/length set
    w = _dynamic_header({1: (0, 1, 1), 18: (1, 1, 1)}, [(1, 0, 0)] * 258)
    out.append(("oversubscribed-lengths", w.finish(0), U.E_LITLEN_SET, True))
    w = _dynamic_header({s: (0, 1, 1) for s in (0, 1, 2)}, [])     # three codes of one bit: the code-length code itself
    out.append(("oversubscribed-code-length-code", w.finish(0), U.E_CODE_LENGTHS, True))
    w = _dynamic_header({1: (0, 1, 1), 16: (1, 1, 1)}, [(16, 0, 2)])
    out.append(("repeat-without-previous", w.finish(0), U.E_REPEAT, True))
    w = _dynamic_header({1: (0, 1, 1), 18: (1, 1, 1)}, [(18, 127, 7), (18, 127, 7)])
    out.append(("repeat-past-the-end", w.finish(0), U.E_REPEAT, True))
    out.append(("raw-one-byte-long", deflate(raw + b"\x00", level=9), U.E_OUTPUT_LONG, False))
    out.append(("raw-one-byte-short", deflate(raw[:-1], level=9), U.E_OUTPUT_SHORT, False))
    bad = bytearray(raw)
    bad[3 * (1 + W * ch)] = 5
    out.append(("filter-byte-5", deflate(bytes(bad), level=9), U.E_FILTER, False))
    return out


def write_kit(root, frames=24, W=22, H=9, thetas=False, optimized=True, cx=None, rgba_at=()):
    """A kit written with PIL -> (rgb uint8 [frames,H,W,3], mask uint8 [frames,H,W], poses dict)."""
    from PIL import Image
    rng = np.random.default_rng(11)
    os.makedirs(os.path.join(root, "images")), os.makedirs(os.path.join(root, "masks")), os.makedirs(os.path.join(root, "score_demo_video"))
    rgb = np.stack([pc.body(H, W, 6, 100 + f) for f in range(frames)])
    mask = np.where(rgb.sum(-1) > 0, 255, 0).astype(np.uint8)
    mask[:, 0, 0] = np.arange(frames)                             # every frame's mask differs
    for f in range(frames):
        if f in rgba_at:
            Image.fromarray(np.concatenate([rgb[f], np.full((H, W, 1), 99, np.uint8)], -1), "RGBA").save(os.path.join(root, "images", f"{f:06d}.png"))
        else:
            Image.fromarray(rgb[f], "RGB").save(os.path.join(root, "images", f"{f:06d}.png"))
        Image.fromarray(mask[f], "L").save(os.path.join(root, "masks", f"{f:06d}.png"))
    K = np.array([[5000.0, 0, W / 2 if cx is None else cx], [0, 5000.0, H / 2], [0, 0, 1]])
    np.savez(os.path.join(root, "score_demo_video", "cameras.npz"), intrinsic=K, extrinsic=np.eye(4), height=np.int64(H), width=np.int64(W))
    poses = {"betas": rng.normal(size=16).astype(np.float32), "global_orient": rng.normal(size=(frames, 3)).astype(np.float32),
             "body_pose": rng.normal(size=(frames, 69)).astype(np.float32), "transl": rng.normal(size=(frames, 3)).astype(np.float32)}
    saved = dict(poses)
    if thetas:
        saved["thetas"] = np.concatenate([saved.pop("global_orient"), saved.pop("body_pose")], -1)
    np.savez(os.path.join(root, "score_demo_video", "poses_optimized.npz" if optimized else "poses.npz"), **saved)
    return rgb, mask, poses


def golden_splits():
    """tests/golden/kit_splits_golden.json -> {"train": {str(n): [...]}, "val": {str(n): [...]}} for n = 10 .. 400.  The file holds
    (first, step, count) of every val list -- the reference's is a slice -- and the train list is the other frames, ascending: its
    generator checks both against the reference's own lists."""
    import json
    with open(os.path.join(GOLDEN, "kit_splits_golden.json")) as f:
        g = json.load(f)
    lo, hi = g["lengths"]
    assert len(g["val_first_step_count"]) == hi - lo + 1
    out = {"train": {}, "val": {}}
    for n, (first, step, count) in zip(range(lo, hi + 1), g["val_first_step_count"]):
        val = [first + k * step for k in range(count)]
        out["val"][str(n)], out["train"][str(n)] = val, [i for i in range(n) if i not in val]
    return out


VALID = _valid()
CORRUPT = _corrupt()
_TWIN = {}


def fnv(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def pil_pixels(data):
    """uint8 [H,W,ch] of a PNG file by PIL."""
    import io
    from PIL import Image
    a = np.array(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


def twin_valid(name):
    """(W, H, ch, stream, raw, status) of a VALID file by ``parse_png`` and ``inflate_host``; computed once."""
    if name not in _TWIN:
        W, H, ch, stream = U.parse_png(dict(VALID)[name])
        _TWIN[name] = (W, H, ch, stream) + U.inflate_host(stream, H * (1 + W * ch))
    return _TWIN[name]


def twin_corrupt(name):
    """(raw, status) of a CORRUPT stream by ``inflate_host`` and, where that passes, ``unfilter_host``; computed once."""
    if name not in _TWIN:
        W, H, ch = CORRUPT_SHAPE
        stream = next(c[1] for c in CORRUPT if c[0] == name)
        raw, status = U.inflate_host(stream, H * (1 + W * ch))
        _TWIN[name] = (raw, status if status else U.unfilter_host(raw, W, H, ch)[1])
    return _TWIN[name]
