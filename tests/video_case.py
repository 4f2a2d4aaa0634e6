"""What the host and the GPU tests of sings_amd/video.py share: the list of frames that exercise the coder, a JPEG marker walker and
a RIFF walker.  The walkers are written here, against the formats, and name nothing of the code under test."""
import struct

import numpy as np


# ---- the frames.  name -> (uint8 [H,W,3] frame, quality, restart_interval | None)
def _noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _cosine(W, H):
    """One high frequency along x only: most coefficients of a block are zero, one far down the zig-zag order is not."""
    x = np.arange(W, dtype=np.float64)
    row = 128.0 + 120.0 * np.cos((2.0 * (x % 8) + 1.0) * 7.0 * np.pi / 16.0)
    return np.repeat(np.repeat(np.rint(row).astype(np.uint8)[None, :, None], H, 0), 3, 2)


def _checkerboard(W, H):
    by, bx = np.mgrid[0:H, 0:W] // 8
    return np.repeat((((by + bx) & 1) * 255).astype(np.uint8)[..., None], 3, 2)


def avatar_like(W, H, seed=5):
    """A textured ellipse (the "avatar") on a flat white background."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    inside = ((x - W / 2) / (W * 0.22)) ** 2 + ((y - H / 2) / (H * 0.42)) ** 2 < 1.0
    body = np.stack([120 + 60 * np.sin(x / 5.0) + rng.normal(0, 6, (H, W)), 90 + 50 * np.cos(y / 7.0) + rng.normal(0, 6, (H, W)),
                     80 + 40 * np.sin((x + y) / 9.0) + rng.normal(0, 6, (H, W))], -1)
    return np.where(inside[..., None], np.clip(body, 0, 255), 255.0).astype(np.uint8)


def gradient(W, H):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1), 255.0 * (x + y) / max(W + H - 2, 1)], -1).astype(np.uint8)


def cases():
    return {
        "8x8": (_noise(8, 8, 1), 90, None),
        "16x8": (_noise(16, 8, 2), 90, None),
        "13x21_edges": (_noise(13, 21, 3), 75, None),
        "96x80_rows": (avatar_like(96, 80), 90, None),           # 10 segments of 12 MCUs: the RST numbering wraps
        "96x80_ri5": (avatar_like(96, 80, 6), 90, 5),            # 24 segments of 5 MCUs
        "96x80_ri7": (gradient(96, 80), 50, 7),                  # 120 = 17 * 7 + 1: a last segment of one MCU
        "constant": (np.full((24, 40, 3), 77, dtype=np.uint8), 90, None),
        "checkerboard_q100": (_checkerboard(32, 16), 100, 4),    # DC differences of category 11 inside a segment
        "noise_q100": (_noise(64, 48, 4), 100, None),            # long codes, byte stuffing
        "noise_q100_ri48": (_noise(64, 48, 4), 100, 48),         # one segment of 144 coefficient blocks: more than 64, a partial last 64
        "cosine_q10": (_cosine(32, 16), 10, None),               # runs of 16 zeros and more: ZRL
        "one_segment": (_noise(40, 24, 8), 60, 65535),           # a restart interval beyond the MCU count
        "152x112_ri1": (avatar_like(152, 112), 90, 1),           # 19 x 14 = 266 segments: more than 256, the scan's second round
    }


def grouped(names, K):
    """Groups of at most K case names whose frames share size, quality and restart interval (one launch each)."""
    c = cases()
    groups = {}
    for n in names:
        f, q, ri = c[n]
        groups.setdefault((f.shape, q, ri), []).append(n)
    out = []
    for key, ns in groups.items():
        for i in range(0, len(ns), K):
            out.append(ns[i:i + K])
    return out


# ---- JPEG
SOI, EOI, APP0, DQT, SOF0, DHT, DRI, SOS = 0xD8, 0xD9, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA


def walk_jpeg(data):
    """-> dict(order=[markers of the header], segments={marker: [payloads]}, entropy=bytes between SOS and EOI (RST markers
    included), rst=[numbers of the RST markers in order], stuffed=count of FF 00 pairs).  Asserts the framing: SOI first, EOI last,
    nothing but 00 or an RST behind an FF of the entropy data."""
    assert data[:2] == bytes((0xFF, SOI)), "SOI first"
    assert data[-2:] == bytes((0xFF, EOI)), "EOI last"
    order, segments = [SOI], {}
    pos = 2
    while True:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        order.append(m)
        segments.setdefault(m, []).append(data[pos + 4:pos + 2 + n])
        pos += 2 + n
        if m == SOS:
            break
    entropy = data[pos:-2]
    rst, stuffed, pieces, start = [], 0, [], 0
    i = 0
    while i < len(entropy):
        if entropy[i] == 0xFF:
            assert i + 1 < len(entropy), "an FF at the end of the entropy data"
            nxt = entropy[i + 1]
            if nxt == 0x00:
                stuffed += 1
            else:
                assert 0xD0 <= nxt <= 0xD7, f"FF {nxt:02X} inside the entropy data"
                rst.append(nxt - 0xD0)
                pieces.append(entropy[start:i])
                start = i + 2
            i += 2
        else:
            i += 1
    pieces.append(entropy[start:])
    return dict(order=order, segments=segments, entropy=entropy, rst=rst, stuffed=stuffed, pieces=pieces)


HEADER_ORDER = [SOI, APP0, DQT, DQT, SOF0, DHT, DHT, DHT, DHT, DRI, SOS]


def check_stream(data, W, H, ri):
    """The segment order, the SOF0 dimensions, the DRI value and the restart markers of one stream; -> walk_jpeg's dict."""
    w = walk_jpeg(data)
    assert w["order"] == HEADER_ORDER, [hex(m) for m in w["order"]]
    seg = w["segments"]
    assert seg[APP0][0] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert [p[0] for p in seg[DQT]] == [0, 1] and all(len(p) == 65 for p in seg[DQT])
    sof = seg[SOF0][0]
    assert sof[0] == 8 and struct.unpack(">HH", sof[1:5]) == (H, W) and sof[5] == 3
    assert sof[6:] == bytes((1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1))
    assert [p[0] for p in seg[DHT]] == [0x00, 0x10, 0x01, 0x11]
    assert struct.unpack(">H", seg[DRI][0])[0] == ri
    assert seg[SOS][0] == bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))
    nmcu = ((W + 7) // 8) * ((H + 7) // 8)
    nseg = (nmcu + ri - 1) // ri
    assert w["rst"] == [i % 8 for i in range(nseg - 1)], (w["rst"], nseg)
    assert all(len(p) > 0 for p in w["pieces"])
    return w


# ---- RIFF
def walk_riff(data):
    """An AVI file -> dict(avih=, strh=, strf= payloads, frames=[payload of every 00dc chunk], offsets=[offset of each chunk from the
    'movi' fourcc], padded=[chunk had a pad byte], idx1=[(id, flags, offset, size)], movi_at=file offset of the 'movi' fourcc)."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8, "the RIFF size covers the file"
    out = dict(frames=[], offsets=[], padded=[], idx1=[])

    def chunks(lo, hi):
        pos = lo
        while pos < hi:
            tag, n = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
            yield tag, pos, n
            pos += 8 + n + (n & 1)
        assert pos == hi, (pos, hi)

    def walk(lo, hi, inside):
        for tag, pos, n in chunks(lo, hi):
            if tag == b"LIST":
                kind = data[pos + 8:pos + 12]
                if kind == b"movi":
                    out["movi_at"] = pos + 8
                walk(pos + 12, pos + 8 + n, inside + [kind])
            elif tag == b"00dc":
                assert inside[-1] == b"movi"
                out["frames"].append(data[pos + 8:pos + 8 + n])
                out["offsets"].append(pos - out["movi_at"])
                out["padded"].append(bool(n & 1))
                if n & 1:
                    assert data[pos + 8 + n] == 0
            elif tag == b"idx1":
                assert not inside
                out["idx1"] = [struct.unpack("<4sIII", data[pos + 8 + 16 * i:pos + 24 + 16 * i]) for i in range(n // 16)]
            else:
                assert tag in (b"avih", b"strh", b"strf"), tag
                assert inside == ([b"hdrl"] if tag == b"avih" else [b"hdrl", b"strl"]), (tag, inside)
                out[tag.decode()] = data[pos + 8:pos + 8 + n]
    walk(12, len(data), [])
    return out
