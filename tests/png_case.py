"""The frames the PNG tests encode (tests/test_png_host.py on the CPU, tests/test_gpu_png.py against the device), and the twin's
streams of them, computed once per process.

A case is (name, frames uint8 [k,H,W,3], filter, rows_per_segment, bgr).  The sizes are the smallest at which the encoder takes another
path: one pixel; scanlines of 64, 67 and 256 bytes (a round of the deflate pass is 64 bytes); 200 x 40 in segments of 7 rows, which
leaves a short last segment and cuts the run of black rows at the top across a segment boundary; 5 x 260 in segments of one row, more
segments than the 256 threads of the offset scan take in one round.
"""
import numpy as np

RUN_LENGTHS = (1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 263, 517, 518)
NOISE = (0, 2, 6, 12, 24)            # amplitudes at which the twin's log shows table 1, 1, 2, 3 and 4 (and 0 in the short segment)


def body(H, W, amp, seed, top_black=0):
    """A synthetic avatar: a smooth body with uniform noise of +-amp on a black background; the first ``top_black`` rows black."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 60 * np.sin(x / 17.0 + y / 23.0), 100 + 80 * np.cos(x / 29.0), 90 + 0.5 * x + 0.3 * y], -1)
    img = base + (rng.integers(-amp, amp + 1, size=(H, W, 3)) if amp else 0)
    m = ((x - W / 2) ** 2 / (W / 3) ** 2 + (y - H / 2) ** 2 / (H / 2.2) ** 2) < 1
    out = np.clip(np.where(m[..., None], img, 0), 0, 255).astype(np.uint8)
    out[:top_black] = 0
    return out


def runs_frame():
    """One scanline under filter "none" whose bytes are runs of RUN_LENGTHS (values 10, 20, 10, ...: the filter byte 0 joins none)."""
    data = np.concatenate([np.full(n, 10 + 10 * (i % 2), dtype=np.uint8) for i, n in enumerate(RUN_LENGTHS)])
    assert data.size % 3 == 0
    return data.reshape(1, 1, data.size // 3, 3)


def cases():
    rng = np.random.default_rng(7)
    out = [
        ("1x1", np.array([[[[200, 3, 77]]]], dtype=np.uint8), "adaptive", None, False),
        ("21x13", np.stack([body(13, 21, a, 1) for a in (0, 6)]), "adaptive", None, False),
        ("22x9", np.stack([body(9, 22, a, 2) for a in (2, 24)]), "adaptive", None, False),
        ("85x7", np.stack([body(7, 85, a, 3) for a in (0, 12, 24)]), "adaptive", None, False),
        ("200x40", np.stack([body(40, 200, a, 4, top_black=10) for a in NOISE]), "adaptive", 7, False),
        ("200x40-flat", np.stack([np.full((40, 200, 3), 255, dtype=np.uint8), np.zeros((40, 200, 3), dtype=np.uint8)]), "adaptive", 7, False),
        ("200x40-random", rng.integers(0, 256, size=(1, 40, 200, 3), dtype=np.uint8), "adaptive", 7, False),
        ("200x40-bgr", body(40, 200, 6, 5)[None], "adaptive", 7, True),
        ("runs", runs_frame(), "none", None, False),
        ("black-85x7", np.zeros((1, 7, 85, 3), dtype=np.uint8), "none", None, False),
        ("5x260", np.stack([body(260, 5, a, 9) for a in (0, 24)]), "adaptive", 1, False),      # 260 segments: the scan's second round
    ]
    for f in ("none", "sub", "up", "average", "paeth"):
        out.append((f"22x9-{f}", body(9, 22, 6, 6)[None], f, None, False))
        out.append((f"200x40-{f}", body(40, 200, 6, 4, top_black=10)[None], f, 7, f == "paeth"))
    return out


CASES = cases()
NOISY = "200x40"                     # the case every candidate is forced on in the host tests
_TWIN = {}


def twin(name, force=-1):
    """(streams, log) of case ``name`` by ``png_encode_host``; computed once."""
    if (name, force) not in _TWIN:
        from sings_amd import png
        _, frames, filter, rps, bgr = next(c for c in CASES if c[0] == name)
        log = {}
        _TWIN[name, force] = (png.png_encode_host(frames, filter=filter, rows_per_segment=rps, bgr=bgr, force=force, log=log), log)
    return _TWIN[name, force]
