"""Times the way from rendered frames to lossless files on the GPU box:  python tools/png_time.py [--reps N] [--frames F] [--out FILE]

One avatar of 150 000 Gaussians (J = 24; ``scene.avatar_scene``) at 512 x 896 and at 1920 x 1080, F = 32 frames with their own poses,
K = 8 frames per launch.  The arms, each a block that starts and ends in a device synchronise, timed by the host clock:

    render_rgb8          ``animate_chunk(out="rgb8")``: the frames as bytes on the device, nothing leaves it (the floor of every route)
    encode_launches      20 ``PngEncoder.encode`` of one rendered batch of 8, back to back: the four launches alone
    encode_to_host       ``PngEncoder.encode_to_host`` of that batch: the launches, the read of the sizes, the read of the used bytes
    animate_to_frames    ``png.animate_to_frames`` of the F frames, end to end, into numbered files in a temporary directory
    rgb8_host_png        the route the tree offered before: ``out="rgb8"``, one copy to the host per frame, PIL PNG per frame to a file
                         (``run_outputs._write_png``, the default writer), at PIL's default compression
    rgb8_host_png_l1     the same with ``compress_level=1``

The arms ALTERNATE block by block after a warm-up; medians over ``--reps`` (>= 5) blocks with min and max; a difference counts as
resolved only when the two arms' [min, max] ranges do not overlap.  Also written: bytes per frame of every form (raw, PIL default, PIL
level 1, device), the candidates the device's segments took (read from the numpy twin's log of the first frame), and that the
device's streams are the twin's for the first batch's first frame.  Writes profiles/png_time.json (``--out``).

``--trace-workload``: no timing -- 20 encodes of one rendered batch at 512 x 896 (``--trace-size 1``: at 1920 x 1080), for a kernel
trace (``rocprofv3 --kernel-trace --stats -- python tools/png_time.py --trace-workload``): the four sg_png_* kernels per batch of 8
frames."""
import argparse
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import video_time as vt                                           # noqa: E402

SIZES = ((512, 896), (1920, 1080))
K = 8


def measure(dev, W, H, F, gaussians, reps, trace):
    from PIL import Image
    from sings_amd import png as P
    from sings_amd import rasterizer as rz
    from sings_amd.posed import FrameAnimator, animate_chunk
    vt.W, vt.H = W, H                                             # (``vt.build`` makes the scene at the module's size)
    args, kw = vt.build(dev, F, gaussians)
    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    animator = FrameAnimator(args[0], streams=2)
    kw = dict(kw, animator=animator, frames_per_launch=K)
    render = lambda out: [x for _, x in animate_chunk(*args, out=out, **kw)]
    rgb8 = torch.stack(render("rgb8"))
    assert bool((rgb8 != 255).any()), "the avatar is in view"
    batch = rgb8[:K].contiguous()
    enc = P.PngEncoder(W, H, K, dev)
    streams = enc.encode_to_host(batch)
    if trace:
        for _ in range(20):
            enc.encode(batch)
        torch.cuda.synchronize()
        return {"trace_workload": {"encodes": 20, "K": K, "bytes": [len(s) for s in streams]}}
    log = {}
    twin = P.png_encode_host(batch[:1].cpu().numpy(), log=log)
    assert streams[:1] == twin, "the device's stream is not the twin's"
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(streams[1]))), batch[1].cpu().numpy()), "lossless"
    tmp = tempfile.mkdtemp(prefix="png_time_")

    def back_to_back():
        for _ in range(20):
            enc.encode(batch)

    def host_route(**save):
        n = 0
        for f, u8 in animate_chunk(*args, out="rgb8", **kw):
            path = os.path.join(tmp, f"h{f:05d}.png")
            Image.fromarray(u8.cpu().numpy()).save(path, **save)  # (one copy per frame)
            n += os.path.getsize(path)
        return n

    def device_route():
        P.animate_to_frames(tmp, *args, pattern="d{:05d}.png", **kw)
        return sum(os.path.getsize(os.path.join(tmp, f"d{f:05d}.png")) for f in range(F))

    arms = {"render_rgb8": lambda: render("rgb8"),
            "encode_launches": back_to_back,
            "encode_to_host": lambda: enc.encode_to_host(batch),
            "animate_to_frames": device_route,
            "rgb8_host_png": lambda: host_route(),
            "rgb8_host_png_l1": lambda: host_route(compress_level=1)}
    per = {"render_rgb8": F, "encode_launches": 20 * K, "encode_to_host": K, "animate_to_frames": F, "rgb8_host_png": F, "rgb8_host_png_l1": F}
    sizes = {"raw": W * H * 3, "device_png": device_route() / F, "pil_png": host_route() / F, "pil_png_l1": host_route(compress_level=1) / F}
    for k in ("raw", "pil_png", "pil_png_l1"):
        sizes[f"device_png_over_{k}"] = sizes["device_png"] / sizes[k]
    out = {"W": W, "H": H, "frames": F, "K": K, "P": gaussians, "rows_per_segment": enc.rows_per_segment, "segments": enc.layout["segments"],
           "ws_bytes": enc.layout["ws_bytes"], "device_stream_equals_twin": True, "bytes_per_frame": sizes,
           "candidates_first_frame": np.bincount(log["candidates"], minlength=P.TABLES + 1).tolist(),
           "filters_first_frame": np.bincount(log["filters"], minlength=5).tolist()}
    res = vt.alternate(arms, reps)
    for k in arms:
        res[k]["per"] = per[k]
        res[k]["ms_per_frame"] = res[k]["median_ms"] / per[k]
        res[k]["ms_per_frame_min_max"] = [res[k]["min"] / per[k], res[k]["max"] / per[k]]
    for slow in ("rgb8_host_png", "rgb8_host_png_l1"):
        res[f"{slow}_over_animate_to_frames"] = vt.verdict(res, "animate_to_frames", slow)
    res["encode_to_host_over_encode_launches"] = vt.verdict(res, "encode_launches", "encode_to_host", 20 * K, K)
    res["animate_to_frames_over_render_rgb8"] = vt.verdict(res, "render_rgb8", "animate_to_frames")
    out["times"] = res
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--gaussians", type=int, default=vt.N)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--trace-size", type=int, default=0, choices=range(len(SIZES)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "png_time.py needs the GPU"
    dev = torch.device("cuda:0")
    if a.trace_workload:
        print(json.dumps(measure(dev, *SIZES[a.trace_size], a.frames, a.gaussians, a.reps, True)))
        return
    out = {"reps": a.reps, "device_name": torch.cuda.get_device_name(0),
           "sizes": [measure(dev, W, H, a.frames, a.gaussians, a.reps, False) for W, H in SIZES]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
