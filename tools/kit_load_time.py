"""Times the way from a training kit on disk to a FrameStore on the GPU box:  python tools/kit_load_time.py [--reps N] [--out FILE]

Synthetic kits, written once into a temporary directory: 80 frames of 512 x 896 and 300 frames of 1920 x 1080, a noisy body on black
with its mask, in two forms --

    pil_l1       PIL at ``compress_level=1``: zlib's level-1 streams, PIL's per-row choice of filter (rows of every type: the decoder
                 walks chains of Up / Average / Paeth rows)
    sub_rle      what cv2 writes and the shipped kit holds: every row of filter type Sub, zlib level 1 with Z_RLE, IDAT chunks of 8 KiB
                 (every row on its own: the decoder's row-parallel path)

The arms, each a block that starts and ends in a device synchronise, timed by the host clock; all of them end with the same bytes in a
``FrameStore`` (checked once):

    load_kit         ``kit.load_kit(root, "train+val")``: files read, chunks walked, streams uploaded, two launches per batch
    read_and_parse   the host's share of that alone: every file read and ``parse_png`` (CRC-32 checked)
    serial           the reference's loop: a decode per file on the host (cv2 where it imports, else PIL), then ``FrameStore(rgb, mask)``
    pool16           the same decodes in a pool of 16 threads

The arms ALTERNATE block by block after a warm-up; medians over ``--reps`` (>= 5) blocks with min and max; a difference counts as
resolved only when the two arms' [min, max] ranges do not overlap.  Writes profiles/kit_load_time.json (``--out``).

``--trace-workload``: no timing -- three ``load_kit`` of the ``--trace-form`` kit at 512 x 896 (``--trace-size 1``: 1920 x 1080), for a
kernel trace in a run of its own (``rocprofv3 --kernel-trace --stats -- python tools/kit_load_time.py --trace-workload``): the two
sg_unpng_* kernels per batch."""
import argparse
import json
import os
import shutil
import struct
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import video_time as vt                                           # noqa: E402

SIZES = ((512, 896, 80), (1920, 1080, 300))                       # W, H, frames
FORMS = ("pil_l1", "sub_rle")
THREADS = 16


_BASE = {}


def body(H, W, f):
    """A synthetic frame: a smooth body with noise of +-3 on black, shifted from frame to frame, and its mask."""
    if (H, W) not in _BASE:
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        base = np.stack([128 + 60 * np.sin(x / 17.0 + y / 23.0), 100 + 80 * np.cos(x / 29.0), 90 + 40 * np.sin(y / 31.0)], -1)
        _BASE[H, W] = (base.astype(np.int16), x, ((y - H / 2) / (H / 2.2)) ** 2)
    base, x, yy = _BASE[H, W]
    rng = np.random.default_rng(f)
    m = ((x - (W / 2 + W / 10 * np.sin(f / 7.0))) / (W / 3.5)) ** 2 + yy < 1
    img = np.clip(base + rng.integers(-3, 4, size=(H, W, 3), dtype=np.int16), 0, 255).astype(np.uint8) * m[..., None]
    return img, np.where(m, 255, 0).astype(np.uint8)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def sub_rle_png(a):
    """uint8 [H,W] or [H,W,3] -> a PNG as cv2 writes it: filter Sub on every row, level 1 with Z_RLE, IDAT chunks of 8192 bytes."""
    a = a[..., None] if a.ndim == 2 else a
    H, W, ch = a.shape
    x = a.reshape(H, W * ch)
    lines = np.empty((H, 1 + W * ch), np.uint8)
    lines[:, 0] = 1
    lines[:, 1:] = x
    lines[:, 1 + ch:] -= x[:, :-ch]
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    stream = c.compress(lines.tobytes()) + c.flush()
    idat = b"".join(_chunk(b"IDAT", stream[i:i + 8192]) for i in range(0, len(stream), 8192))
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if ch == 1 else 2, 0, 0, 0)) + idat
            + _chunk(b"IEND", b""))


def write_kit(root, W, H, frames, form):
    from PIL import Image
    for d in ("images", "masks", "score_demo_video"):
        os.makedirs(os.path.join(root, d))

    body(H, W, 0)                                                 # (the shared arrays, before the threads)

    def one(f):
        img, mask = body(H, W, f)
        for d, a in (("images", img), ("masks", mask)):
            path = os.path.join(root, d, f"{f:06d}.png")
            if form == "pil_l1":
                Image.fromarray(a).save(path, compress_level=1)
            else:
                with open(path, "wb") as fh:
                    fh.write(sub_rle_png(a))
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(one, range(frames)))
    K = np.array([[5000.0, 0, W / 2], [0, 5000.0, H / 2], [0, 0, 1]])
    np.savez(os.path.join(root, "score_demo_video", "cameras.npz"), intrinsic=K, extrinsic=np.eye(4), height=np.int64(H), width=np.int64(W))
    z = lambda *s: np.zeros(s, np.float32)
    np.savez(os.path.join(root, "score_demo_video", "poses_optimized.npz"), betas=z(16), global_orient=z(frames, 3), body_pose=z(frames, 69),
             transl=z(frames, 3))


def host_decoder():
    """(name, path -> array): cv2.imread where cv2 imports (the reference's call), else PIL."""
    try:
        import cv2
        return "cv2", lambda p, grey: cv2.imread(p, cv2.IMREAD_GRAYSCALE) if grey else np.ascontiguousarray(cv2.imread(p)[..., :3][..., ::-1])
    except ImportError:
        from PIL import Image
        return "PIL", lambda p, grey: np.asarray(Image.open(p))


def measure(dev, root, W, H, frames, form, reps, trace):
    from sings_amd import kit as KIT
    from sings_amd import unpng
    from sings_amd.frame_feed import FrameStore
    images = sorted(os.path.join(root, "images", n) for n in os.listdir(os.path.join(root, "images")))
    masks = sorted(os.path.join(root, "masks", n) for n in os.listdir(os.path.join(root, "masks")))
    device_route = lambda: KIT.load_kit(root, "train+val", dev).store
    if trace:
        for _ in range(3):
            device_route()
        torch.cuda.synchronize()
        return {"trace_workload": {"loads": 3, "form": form, "W": W, "H": H, "frames": frames}}
    name, decode = host_decoder()

    def host_route(pool):
        run = (lambda fn, xs: list(pool.map(fn, xs))) if pool else (lambda fn, xs: [fn(x) for x in xs])
        rgb = run(lambda p: decode(p, False), images)
        mask = run(lambda p: decode(p, True), masks)
        return FrameStore(np.stack(rgb), np.stack(mask), dev)

    def read_and_parse():
        n = 0
        for p in images + masks:
            with open(p, "rb") as fh:
                n += len(unpng.parse_png(fh.read())[3])
        return n
    pool = ThreadPoolExecutor(THREADS)
    want = host_route(pool).data
    assert torch.equal(device_route().data, want), "the device's store is not the host decoder's"
    del want
    types = np.zeros(5, np.int64)
    with open(images[0], "rb") as fh:
        w, h, ch, stream = unpng.parse_png(fh.read())
    types += np.bincount(np.frombuffer(zlib.decompress(stream), np.uint8).reshape(h, -1)[:, 0], minlength=5)
    arms = {"load_kit": device_route, "read_and_parse": read_and_parse, "serial": lambda: host_route(None), "pool16": lambda: host_route(pool)}
    res = vt.alternate(arms, reps, warmup=1)
    pool.shutdown()
    for k in arms:
        res[k]["ms_per_frame"] = res[k]["median_ms"] / frames
    res["serial_over_load_kit"] = vt.verdict(res, "load_kit", "serial")
    res["pool16_over_load_kit"] = vt.verdict(res, "load_kit", "pool16")
    res["load_kit_over_read_and_parse"] = vt.verdict(res, "read_and_parse", "load_kit")
    return {"W": W, "H": H, "frames": frames, "form": form, "host_decoder": name, "threads": THREADS,
            "file_bytes": {"images": sum(os.path.getsize(p) for p in images), "masks": sum(os.path.getsize(p) for p in masks)},
            "stream_bytes": read_and_parse(), "store_bytes": frames * H * W * 4, "filter_types_first_image": types.tolist(),
            "device_store_equals_host_decoders": True, "times": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--trace-size", type=int, default=0, choices=range(len(SIZES)))
    ap.add_argument("--trace-form", default="sub_rle", choices=FORMS)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(range(len(SIZES))), help="indices into SIZES")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kit_load_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "kit_load_time.py needs the GPU"
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp(prefix="kit_load_time_")
    try:
        if a.trace_workload:
            W, H, frames = SIZES[a.trace_size]
            write_kit(os.path.join(tmp, "kit"), W, H, frames, a.trace_form)
            print(json.dumps(measure(dev, os.path.join(tmp, "kit"), W, H, frames, a.trace_form, a.reps, True)))
            return
        out = {"reps": a.reps, "device_name": torch.cuda.get_device_name(0), "kits": []}
        for i in a.sizes:
            W, H, frames = SIZES[i]
            for form in FORMS:
                root = os.path.join(tmp, f"kit_{W}x{H}_{form}")
                write_kit(root, W, H, frames, form)
                out["kits"].append(measure(dev, root, W, H, frames, form, a.reps, False))
                shutil.rmtree(root)
                print(json.dumps(out["kits"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:                              # one line per kit
            short = lambda x: (round(x, 3) if isinstance(x, float) else {k: short(v) for k, v in x.items()} if isinstance(x, dict) else
                               [short(v) for v in x] if isinstance(x, list) else x)
            kits = ",\n  ".join(json.dumps(short(k)) for k in out.pop("kits"))
            fh.write(json.dumps(out)[:-1] + ', "kits": [\n  ' + kits + "\n]}\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
