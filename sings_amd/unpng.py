"""PNG files to the frame store on the device (include/sings_unpng.h, csrc/sg_unpng.hip, csrc/sg_inflate.h).

``parse_png`` is the host's share of a decode: it walks a file's chunks, refuses what the device path does not read and joins the IDAT
payloads into the one zlib stream they are.  ``PngDecoder`` stages the streams of a batch of files in one pinned buffer, uploads it
once and lets two launches -- inflate (a wave per stream), unfilter and scatter (a wave per scanline) -- write the pixels into a
``FrameStore``'s ``data``; it reads back one status per stream.  ``inflate_host`` and ``unfilter_host`` restate the two launches in
Python, code for code and status for status: the definition the kernels (and csrc/sg_inflate.h on the host) are tested against.
``inflate_host`` is for tests, not for speed.
"""
import struct
import zlib

import numpy as np

from . import _lib

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_STREAMS = _lib.UNPNG_MAX_STREAMS
MAX_ROW_BYTES = _lib.UNPNG_MAX_ROW_BYTES
MAX_HEIGHT = _lib.UNPNG_MAX_HEIGHT
WINDOW = 32768
FAST_BITS = 9
# SG_UNPNG_E_*: the status of a stream
STATUS = ("OK", "E_INPUT", "E_HEADER", "E_BLOCK_TYPE", "E_STORED", "E_COUNTS", "E_CODE_LENGTHS", "E_REPEAT", "E_NO_END", "E_LITLEN_SET",
          "E_DIST_SET", "E_LITLEN_SYMBOL", "E_DIST_SYMBOL", "E_DISTANCE", "E_OUTPUT_LONG", "E_OUTPUT_SHORT", "E_ADLER", "E_TABLE", "E_SIZE",
          "E_WORKSPACE", "E_FILTER")
(OK, E_INPUT, E_HEADER, E_BLOCK_TYPE, E_STORED, E_COUNTS, E_CODE_LENGTHS, E_REPEAT, E_NO_END, E_LITLEN_SET, E_DIST_SET, E_LITLEN_SYMBOL,
 E_DIST_SYMBOL, E_DISTANCE, E_OUTPUT_LONG, E_OUTPUT_SHORT, E_ADLER, E_TABLE, E_SIZE, E_WORKSPACE, E_FILTER) = range(len(STATUS))
_CHANNELS = {0: 1, 2: 3, 6: 4}           # colour type -> channels (bit depth 8)
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def parse_png(data, verify_crc=True):
    """A PNG file's bytes -> ``(width, height, channels, zlib_stream)``: the chunks walked, the IDAT payloads joined.  ``ValueError``
    naming what is refused: a wrong signature, a chunk that runs past the file, a CRC-32 that is not its chunk's (unless
    ``verify_crc=False``), a first chunk that is not a 13-byte IHDR, bit depth other than 8, colour type other than 0, 2 or 6, a
    compression or filter method other than 0, interlace, no IDAT, IDATs that are not consecutive, no IEND."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file: wrong signature")
    at, ihdr, parts, closed, ended = 8, None, [], False, False
    while at < len(data):
        if len(data) - at < 12:
            raise ValueError(f"truncated PNG: {len(data) - at} bytes where a chunk begins (offset {at})")
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        if n > len(data) - at - 12:
            raise ValueError(f"truncated PNG: chunk {kind!r} at offset {at} holds {n} bytes, the file has {len(data) - at - 12} left")
        body = data[at + 8:at + 8 + n]
        if verify_crc and struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(kind + body):
            raise ValueError(f"chunk {kind!r} at offset {at}: wrong CRC-32")
        if ihdr is None:
            if kind != b"IHDR" or n != 13:
                raise ValueError(f"the first chunk is {kind!r} of {n} bytes, not a 13-byte IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IHDR":
            raise ValueError("a second IHDR chunk")
        elif kind == b"IDAT":
            if closed:
                raise ValueError(f"IDAT chunk at offset {at} behind another chunk: IDATs must be consecutive")
            parts.append(body)
        else:
            closed = closed or bool(parts)
            if kind == b"IEND":
                ended = True
                break
        at += 12 + n
    if ihdr is None:
        raise ValueError("truncated PNG: no IHDR chunk")
    W, H, ch = _check_ihdr(ihdr)
    if not parts:
        raise ValueError("no IDAT chunk")
    if not ended:
        raise ValueError("truncated PNG: no IEND chunk")
    return W, H, ch, b"".join(parts)


def _check_ihdr(ihdr):
    W, H, depth, colour, compression, filter, interlace = ihdr
    if W < 1 or H < 1 or W >= 1 << 31 or H >= 1 << 31:
        raise ValueError(f"a picture of {W} x {H} pixels")
    if depth != 8:
        raise ValueError(f"bit depth {depth}: only 8-bit PNGs are read")
    if colour not in _CHANNELS:
        raise ValueError(f"colour type {colour}: only grey (0), RGB (2) and RGBA (6) are read")
    if compression != 0 or filter != 0:
        raise ValueError(f"compression method {compression}, filter method {filter}: PNG defines 0 and 0")
    if interlace != 0:
        raise ValueError("interlaced (Adam7): only non-interlaced PNGs are read")
    return W, H, _CHANNELS[colour]


def read_png_header(head):
    """The first 33 bytes of a PNG file (or more) -> ``(width, height, channels)``, with ``parse_png``'s refusals of the IHDR."""
    head = bytes(head[:33])
    if head[:8] != SIGNATURE:
        raise ValueError("not a PNG file: wrong signature")
    if len(head) < 33:
        raise ValueError("truncated PNG: no IHDR chunk")
    n, kind = struct.unpack(">I4s", head[8:16])
    if kind != b"IHDR" or n != 13:
        raise ValueError(f"the first chunk is {kind!r} of {n} bytes, not a 13-byte IHDR")
    return _check_ihdr(struct.unpack(">IIBBBBB", head[16:29]))


def check_kit_files(image_paths, mask_paths, size=None):
    """The headers of a kit's files -> ``(W, H, raw)``, ``raw`` the most filtered scanline bytes a file holds.  ``ValueError`` naming
    the file: unequal counts, a file ``read_png_header`` refuses, an image that is not RGB or RGBA, a mask that is not grey, a size
    that is not ``size`` (W, H) -- or, without one, the first image's."""
    if len(image_paths) != len(mask_paths) or not image_paths:
        raise ValueError(f"{len(image_paths)} images and {len(mask_paths)} masks: the counts must be equal and not zero")
    raw = 1
    for paths, channels, what in ((image_paths, (3, 4), "RGB or RGBA"), (mask_paths, (1,), "grey")):
        for path in paths:
            with open(path, "rb") as f:
                head = f.read(33)
            try:
                W, H, ch = read_png_header(head)
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
            if ch not in channels:
                raise ValueError(f"{path}: a PNG of {ch} channels where a {what} one is expected")
            size = size or (W, H)
            if (W, H) != tuple(size):
                raise ValueError(f"{path}: a picture of {W} x {H} pixels, {size[0]} x {size[1]} expected")
            raw = max(raw, H * (1 + W * ch))
    return size[0], size[1], raw


# ---- csrc/sg_inflate.h in Python ----------------------------------------------------------------------------------------------------
class _Bits:
    """SgInflateBits: the next ``n`` bits of the stream in ``buf``, LSB first.  (The C refill takes eight bytes at a time where the
    stream has them; which bits are valid, and when the stream counts as ended, is the same.)"""

    def __init__(self, data):
        self.data, self.pos, self.buf, self.n = data, 0, 0, 0

    def refill(self):
        while self.n <= 56 and self.pos < len(self.data):
            self.buf |= self.data[self.pos] << self.n
            self.pos += 1
            self.n += 8

    def take(self, k):
        """k bits, or None when the stream has fewer."""
        if self.n < k:
            self.refill()
        if self.n < k:
            return None
        v = self.buf & ((1 << k) - 1)
        self.buf >>= k
        self.n -= k
        return v

    def align(self):
        drop = self.n & 7
        self.buf >>= drop
        self.n -= drop


class _Code:
    """SgInflateCode, built by sg_inflate_build: ``state`` 0 complete or empty, 1 incomplete, -1 over-subscribed."""

    def __init__(self, lens):
        n = len(lens)
        self.n, self.count, self.fast = n, [0] * 16, [0] * (1 << FAST_BITS)
        for v in lens:
            self.count[v] += 1
        self.longest, left, self.state = 0, 1, 0
        for bits in range(1, 16):
            left = (left << 1) - self.count[bits]
            if left < 0:
                self.state = -1
                return
            if self.count[bits]:
                self.longest = bits
        nxt = [0] * 16
        for bits in range(1, 15):
            nxt[bits + 1] = nxt[bits] + self.count[bits]
        self.symbol = [0] * n
        for s, bits in enumerate(lens):
            if bits:
                self.symbol[nxt[bits]] = s
                nxt[bits] += 1
        code = 0
        for bits in range(1, 16):
            code = (code + (self.count[bits - 1] if bits > 1 else 0)) << 1
            nxt[bits] = code
        for s, bits in enumerate(lens):
            if bits == 0 or bits > FAST_BITS:
                continue
            v, rev = nxt[bits], 0
            nxt[bits] += 1
            for _ in range(bits):
                rev, v = rev << 1 | (v & 1), v >> 1
            for k in range(rev, 1 << FAST_BITS, 1 << bits):
                self.fast[k] = s << 4 | bits
        self.state = 0 if self.longest == 0 else (1 if left > 0 else 0)

    def decode(self, b):
        """sg_inflate_symbol: a symbol, -1 when the stream ends inside a code, -2 for a bit pattern that is no code."""
        if b.n < 15:
            b.refill()
        e = self.fast[b.buf & ((1 << FAST_BITS) - 1)]
        if e:
            bits = e & 15
            if bits > b.n:
                return -1
            b.buf >>= bits
            b.n -= bits
            return e >> 4
        code = first = index = 0
        for bits in range(1, 16):
            if bits > b.n:
                return -1
            code |= (b.buf >> (bits - 1)) & 1
            count = self.count[bits]
            if code - count < first:
                at = index + (code - first)
                if at < 0 or at >= self.n:
                    return -2
                b.buf >>= bits
                b.n -= bits
                return self.symbol[at]
            index += count
            first = (first + count) << 1
            code <<= 1
        return -2


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _Code([5] * 32))
    return _FIXED


def _dynamic(b):
    """sg_inflate_dynamic -> (litlen, dist) or a status."""
    v = b.take(14)
    if v is None:
        return E_INPUT
    nlen, ndist, ncode = (v & 31) + 257, ((v >> 5) & 31) + 1, (v >> 10) + 4
    if nlen > 286 or ndist > 30:
        return E_COUNTS
    cl = [0] * 19
    for i in range(ncode):
        v = b.take(3)
        if v is None:
            return E_INPUT
        cl[_CL_ORDER[i]] = v
    code = _Code(cl)
    if code.state != 0 or code.longest == 0:
        return E_CODE_LENGTHS
    lens = []
    while len(lens) < nlen + ndist:
        sym = code.decode(b)
        if sym == -1:
            return E_INPUT
        if sym < 0 or sym > 18:
            return E_CODE_LENGTHS
        if sym < 16:
            lens.append(sym)
            continue
        value = 0
        if sym == 16:
            if not lens:
                return E_REPEAT
            value, v = lens[-1], b.take(2)
            repeat = 3 + (v or 0)
        elif sym == 17:
            v = b.take(3)
            repeat = 3 + (v or 0)
        else:
            v = b.take(7)
            repeat = 11 + (v or 0)
        if v is None:
            return E_INPUT
        if len(lens) + repeat > nlen + ndist:
            return E_REPEAT
        lens.extend([value] * repeat)
    if lens[256] == 0:
        return E_NO_END
    litlen = _Code(lens[:nlen])
    if litlen.state < 0 or (litlen.state > 0 and litlen.longest != 1):
        return E_LITLEN_SET
    dist = _Code(lens[nlen:])
    if dist.state < 0 or (dist.state > 0 and dist.longest != 1):
        return E_DIST_SET
    return litlen, dist


def inflate_host(stream, expected):
    """sg_inflate in Python: a zlib stream -> ``(raw, status)``.  ``raw`` is the ``expected`` bytes of the output (``bytes``) when
    ``status`` is 0, else what had been produced at the first error; ``status`` is the SG_UNPNG_E_* code the device and
    csrc/sg_inflate.h give for the same stream."""
    b, out, expected = _Bits(bytes(stream)), bytearray(), int(expected)
    v = b.take(16)
    if v is None:
        return bytes(out), E_INPUT
    cmf, flg = v & 255, v >> 8
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 != 0 or (flg & 32):
        return bytes(out), E_HEADER
    while True:                                                   # (the header's window size is not held against the distances: zlib's is not)
        v = b.take(3)
        if v is None:
            return bytes(out), E_INPUT
        last, kind = v & 1, v >> 1
        if kind == 3:
            return bytes(out), E_BLOCK_TYPE
        if kind == 0:
            b.align()
            v = b.take(32)
            if v is None:
                return bytes(out), E_INPUT
            n = v & 0xFFFF
            if (n ^ 0xFFFF) != (v >> 16):
                return bytes(out), E_STORED
            for _ in range(n):
                byte = b.take(8)
                if byte is None:
                    return bytes(out), E_INPUT
                if len(out) >= expected:
                    return bytes(out), E_OUTPUT_LONG
                out.append(byte)
        else:
            codes = _fixed() if kind == 1 else _dynamic(b)
            if isinstance(codes, int):
                return bytes(out), codes
            litlen, dist = codes
            while True:
                sym = litlen.decode(b)
                if sym == -1:
                    return bytes(out), E_INPUT
                if sym < 0 or sym > 285:
                    return bytes(out), E_LITLEN_SYMBOL
                if sym < 256:
                    if len(out) >= expected:
                        return bytes(out), E_OUTPUT_LONG
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                if sym < 265:
                    n = sym - 254
                elif sym == 285:
                    n = 258
                else:
                    bits = (sym - 261) >> 2
                    extra = b.take(bits)
                    if extra is None:
                        return bytes(out), E_INPUT
                    n = 3 + ((4 + ((sym - 265) & 3)) << bits) + extra
                sym = dist.decode(b)
                if sym == -1:
                    return bytes(out), E_INPUT
                if sym < 0 or sym > 29:
                    return bytes(out), E_DIST_SYMBOL
                if sym < 4:
                    d = sym + 1
                else:
                    bits = (sym >> 1) - 1
                    extra = b.take(bits)
                    if extra is None:
                        return bytes(out), E_INPUT
                    d = 1 + ((2 + (sym & 1)) << bits) + extra
                if d > len(out) or d > WINDOW:
                    return bytes(out), E_DISTANCE
                if n > expected - len(out):
                    return bytes(out), E_OUTPUT_LONG
                if d >= n:
                    out += out[len(out) - d:len(out) - d + n]
                else:                                             # byte i of the copy is byte i % d of the d bytes in front of it
                    piece = bytes(out[len(out) - d:])
                    out += (piece * (n // d + 1))[:n]
        if last:
            break
    if len(out) != expected:
        return bytes(out), E_OUTPUT_SHORT
    b.align()
    v = b.take(32)
    if v is None:
        return bytes(out), E_INPUT
    if struct.unpack(">I", struct.pack("<I", v))[0] != zlib.adler32(bytes(out)):
        return bytes(out), E_ADLER
    return bytes(out), OK


def unfilter_host(raw, width, height, channels):
    """The second launch in numpy: ``height`` scanlines of a filter byte and ``width * channels`` bytes -> ``(pixels, status)``,
    ``pixels`` uint8 [height, width, channels] (None unless ``status`` is 0; E_FILTER for a filter byte above 4).  bpp = channels; the
    row above the first is zeros; Average is floor((a + b) / 2); Paeth breaks ties in the order a, b, c."""
    W, H, ch = int(width), int(height), int(channels)
    nb = W * ch
    lines = np.frombuffer(bytes(raw), np.uint8)
    if lines.size != H * (1 + nb):
        raise ValueError(f"unfilter_host: {lines.size} bytes, {H} scanlines of {1 + nb} expected")
    lines = lines.reshape(H, 1 + nb)
    if (lines[:, 0] > 4).any():
        return None, E_FILTER
    out = np.zeros((H, nb), np.uint8)
    prev = np.zeros(nb, np.int64)
    for y in range(H):
        t, x = int(lines[y, 0]), lines[y, 1:].astype(np.int64)
        if t == 0:
            cur = x
        elif t == 1:
            cur = np.cumsum(x.reshape(W, ch), axis=0).reshape(nb) & 255
        elif t == 2:
            cur = (x + prev) & 255
        else:
            cur = np.zeros(nb, np.int64)
            for i in range(nb):
                a = int(cur[i - ch]) if i >= ch else 0
                b = int(prev[i])
                if t == 3:
                    pred = (a + b) >> 1
                else:
                    c = int(prev[i - ch]) if i >= ch else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (int(x[i]) + pred) & 255
        out[y] = cur
        prev = cur
    return out.reshape(H, W, ch), OK


# ---- the device decoder -------------------------------------------------------------------------------------------------------------
class PngDecoder:
    """``PngDecoder(device, max_streams, max_raw_bytes)``: up to ``max_streams`` PNG files per batch, each of at most ``max_raw_bytes``
    filtered scanline bytes (``H * (1 + W * channels)``).  The workspace and the status words are allocated here;
    the staging buffers (pinned on the host, one on the device) grow to the largest batch seen.

    ``decode_into(store_data, files, dest)``: ``store_data`` uint8 [F,H,W,4] on the device; ``files`` a sequence of paths or of
    ``bytes``; ``dest[i]`` is ``frame * 4 + first_channel`` of file i (first channel 0 for an RGB or RGBA file, 3 for a grey one).
    Per batch: one upload, the two launches, one read of ``status``.  ``ValueError`` naming the file and the code of every failed
    stream -- raised after all batches ran, so every file that can be decoded has been; a failed stream wrote nothing."""

    def __init__(self, device, max_streams, max_raw_bytes, verify_crc=True):
        import torch
        from . import _marshal
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("sings_amd.unpng.PngDecoder runs on the MI355X only; there is no CPU fallback (inflate_host and "
                               "unfilter_host are the restatement the tests compare it with)")
        self.max_streams, self.max_raw_bytes, self.verify_crc = int(max_streams), int(max_raw_bytes), bool(verify_crc)
        self.layout = _marshal.unpng_layout(self.max_streams, self.max_raw_bytes)
        with torch.cuda.device(self.dev):
            self._ws = torch.empty(self.layout["ws_bytes"], dtype=torch.uint8, device=self.dev)
            self.status = torch.zeros(self.max_streams, dtype=torch.int32, device=self.dev)
        self._host = self._staged = None
        self.launches = self.uploads = 0                          # counted for tests and for tools/kit_load_time.py

    def _stage(self, nbytes):
        import torch
        if self._host is None or self._host.numel() < nbytes:
            cap = max(nbytes, 1 << 16)
            self._host = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._staged = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        return self._host, self._staged

    def decode_into(self, store_data, files, dest):
        import torch
        from . import _marshal
        if (not torch.is_tensor(store_data) or store_data.device != self.dev or store_data.dtype != torch.uint8 or store_data.dim() != 4
                or store_data.shape[3] != 4 or not store_data.is_contiguous()):
            raise ValueError(f"PngDecoder.decode_into: a contiguous uint8 [F,H,W,4] tensor on {self.dev} expected")
        files, dest = list(files), [int(d) for d in dest]
        if len(files) != len(dest):
            raise ValueError(f"PngDecoder.decode_into: {len(files)} files and {len(dest)} destinations")
        F, H, W = (int(n) for n in store_data.shape[:3])
        failed = []
        for b0 in range(0, len(files), self.max_streams):
            names, rows, parts, at = [], [], [], 0
            for f, d in zip(files[b0:b0 + self.max_streams], dest[b0:b0 + self.max_streams]):
                if isinstance(f, (bytes, bytearray, memoryview)):
                    name, data = f"<file {len(names) + b0}>", bytes(f)
                else:
                    name = str(f)
                    with open(f, "rb") as fh:
                        data = fh.read()
                try:
                    w, h, ch, stream = parse_png(data, self.verify_crc)
                except ValueError as e:
                    raise ValueError(f"{name}: {e}") from None
                names.append(name)
                rows.append((at, len(stream), w, h, ch, d))
                parts.append(stream)
                at += len(stream)
            n = len(rows)
            host, staged = self._stage(at + n * _lib.UNPNG_TABLE_COLS * 8)
            # one pinned buffer, one upload: the table's bytes, then the streams
            table = np.asarray(rows, dtype=np.int64).reshape(n, _lib.UNPNG_TABLE_COLS)
            tb = table.size * 8
            view = host.numpy()
            view[:tb] = table.view(np.uint8).reshape(-1)
            view[tb:tb + at] = np.frombuffer(b"".join(parts), np.uint8)
            with torch.cuda.device(self.dev):
                staged[:tb + at].copy_(host[:tb + at], non_blocking=True)
                self.uploads += 1
                _marshal.unpng_decode(n, staged[tb:tb + max(at, 1)], staged[:tb].view(torch.int64), self._ws, store_data, self.status,
                                      torch.cuda.current_stream(self.dev))
                self.launches += 2
                status = self.status[:n].cpu().tolist()
            failed += [(name, s) for name, s in zip(names, status) if s != OK]
        if failed:
            raise ValueError("PngDecoder: " + "; ".join(f"{name}: SG_UNPNG_{STATUS[s] if 0 <= s < len(STATUS) else s} ({s})" for name, s in failed))
        return len(files)
