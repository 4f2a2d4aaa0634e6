"""Times the way from rendered frames to a file on the GPU box:  python tools/video_time.py [--reps N] [--frames F] [--out FILE]

One avatar of 150 000 Gaussians (J = 24; ``scene.avatar_scene``) at 512 x 896, F = 32 frames with their own poses, K = 8 frames per
launch, JPEG quality 90.  The arms, each a block that starts and ends in a device synchronise, timed by the host clock:

    render_bgr8          ``animate_chunk(out="bgr8")``: the frames as bytes on the device, nothing leaves it (the floor of every route)
    encode_launches      20 ``JpegEncoder.encode`` of one rendered batch of 8, back to back: the four launches alone
    encode_to_host       ``JpegEncoder.encode_to_host`` of that batch: the launches, the read of the sizes, the read of the used bytes
    animate_to_video     ``video.animate_to_video`` of the F frames, end to end, into a Motion-JPEG AVI in a temporary directory
    bgr8_host_png        the route the tree offered before: ``out="bgr8"``, one copy to the host per frame, PIL PNG per frame to a file
                         (``run_outputs._write_png``, the default writer)
    bgr8_host_pil_jpeg   the same route with PIL's JPEG at the same quality, subsampling off

The arms ALTERNATE block by block after a warm-up; medians over ``--reps`` (>= 5) blocks with min and max; a difference counts as
resolved only when the two arms' [min, max] ranges do not overlap.  Also written: bytes per frame of every form (raw, PNG, PIL JPEG,
device JPEG), and that the device's streams of the timed frames are the numpy twin's for the first batch.  Writes
profiles/video_time.json (``--out``).

``--trace-workload``: no timing -- 20 encodes of one rendered batch, for a kernel trace (``rocprofv3 --kernel-trace --stats -- python
tools/video_time.py --trace-workload``): the four sg_jpeg_* kernels per batch of 8 frames."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

W, H, N, J, K, QUALITY = 512, 896, 150000, 24, 8, 90


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def alternate(arms, reps, warmup=2):
    """{name: fn} -> {name: {median_ms, min, max}}: every arm warmed up, then ``reps`` rounds of one block per arm, in turn."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn)[0])
    return {k: {"median_ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}


def verdict(res, fast, slow, per_fast=1.0, per_slow=1.0):
    """The ratio of the medians (each divided by its frames) and whether the blocks' spread resolves which is faster."""
    f = {k: res[fast][k] / per_fast for k in ("median_ms", "min", "max")}
    s = {k: res[slow][k] / per_slow for k in ("median_ms", "min", "max")}
    return {"ratio": s["median_ms"] / f["median_ms"], "resolved": bool(f["max"] < s["min"] or s["max"] < f["min"]),
            "faster": fast if f["median_ms"] < s["median_ms"] else slow}


def build(dev, F, n=N):
    from sings_amd.body import joint_transforms
    from sings_amd.scene import avatar_scene
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s = avatar_scene(N=n, J=J, W=W, H=H, seed=4)
    rs = np.random.RandomState(40)
    jr = t(s["joints_rest"])
    canon = dict(xyz_canon=t(s["xyz_canon"]), rotmat_canon=None, scales=t(s["scales"]), opacity=t(s["opacities"]), shs=t(s["shs"]),
                 lbs_weights=t(s["lbs_weights"]), active_sh_degree=0)
    cam = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in s["cam"].items()}
    cam.update(image_width=W, image_height=H)
    poses = t(rs.normal(0, 0.2, (F, 3 * J)).astype(np.float32))
    transl = t((s["transl"][None] + rs.normal(0, 0.03, (F, 3))).astype(np.float32))
    A_cano = joint_transforms(torch.zeros(3 * J, device=dev), jr, tuple(s["parents"]))
    args = (canon, poses, jr, A_cano, cam, torch.ones(3, device=dev))
    return args, dict(transl=transl, parents=tuple(s["parents"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--gaussians", type=int, default=N)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "video_time.py needs the GPU"
    from PIL import Image
    from sings_amd import rasterizer as rz
    from sings_amd import video as V
    from sings_amd.posed import FrameAnimator, animate_chunk
    dev = torch.device("cuda:0")
    F = a.frames
    args, kw = build(dev, F, a.gaussians)
    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    animator = FrameAnimator(args[0], streams=2)
    kw = dict(kw, animator=animator, frames_per_launch=K)
    render = lambda out: [x for _, x in animate_chunk(*args, out=out, **kw)]
    rgb8 = torch.stack(render("rgb8"))
    assert bool((rgb8 != 255).any()), "the avatar is in view"
    batch = rgb8[:K].contiguous()
    enc = V.JpegEncoder(W, H, K, dev, quality=QUALITY)
    streams = enc.encode_to_host(batch)
    if a.trace_workload:
        for _ in range(20):
            enc.encode(batch)
        torch.cuda.synchronize()
        print(json.dumps({"trace_workload": {"encodes": 20, "K": K, "bytes": [len(s) for s in streams]}}))
        return
    twin = V.jpeg_encode_host(batch[:2].cpu().numpy(), QUALITY)
    tmp = tempfile.mkdtemp(prefix="video_time_")

    def back_to_back():
        for _ in range(20):
            enc.encode(batch)

    def host_route(fmt):
        n = 0
        for f, u8 in animate_chunk(*args, out="bgr8", **kw):
            arr = u8.cpu().numpy()[..., ::-1]                     # (one copy per frame; RGB for the writer)
            path = os.path.join(tmp, f"{f:05d}.{fmt}")
            if fmt == "png":
                Image.fromarray(arr).save(path)
            else:
                Image.fromarray(arr).save(path, "JPEG", quality=QUALITY, subsampling=0)
            n += os.path.getsize(path)
        return n

    arms = {"render_bgr8": lambda: render("bgr8"),
            "encode_launches": back_to_back,
            "encode_to_host": lambda: enc.encode_to_host(batch),
            "animate_to_video": lambda: V.animate_to_video(os.path.join(tmp, "anim.avi"), *args, fps=20, quality=QUALITY, **kw),
            "bgr8_host_png": lambda: host_route("png"),
            "bgr8_host_pil_jpeg": lambda: host_route("jpg")}
    per = {"render_bgr8": F, "encode_launches": 20 * K, "encode_to_host": K, "animate_to_video": F, "bgr8_host_png": F,
           "bgr8_host_pil_jpeg": F}
    all_streams = render("jpeg")
    png_bytes, pil_jpeg_bytes = host_route("png"), host_route("jpg")
    psnr = lambda x, y: float(10 * np.log10(255.0 ** 2 / max(np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2), 1e-12)))
    first = rgb8[0].cpu().numpy()
    pil = io.BytesIO()
    Image.fromarray(first).save(pil, "JPEG", quality=QUALITY, subsampling=0)
    out = {"reps": a.reps, "frames": F, "P": a.gaussians, "W": W, "H": H, "K": K, "quality": QUALITY,
           "device_name": torch.cuda.get_device_name(0),
           "device_streams_equal_twin": bool(streams[:2] == twin),
           "bytes_per_frame": {"raw": W * H * 3, "device_jpeg": sum(len(s) for s in all_streams) / F, "png": png_bytes / F,
                               "pil_jpeg": pil_jpeg_bytes / F},
           "psnr_first_frame_db": {"device_jpeg": psnr(np.asarray(Image.open(io.BytesIO(all_streams[0]))), first),
                                   "pil_jpeg": psnr(np.asarray(Image.open(io.BytesIO(pil.getvalue()))), first)}}
    out["bytes_per_frame"]["raw_over_device_jpeg"] = out["bytes_per_frame"]["raw"] / out["bytes_per_frame"]["device_jpeg"]
    assert out["device_streams_equal_twin"], "the device's streams are not the twin's"
    res = alternate(arms, a.reps)
    for k in arms:
        res[k]["per"] = per[k]
        res[k]["ms_per_frame"] = res[k]["median_ms"] / per[k]
        res[k]["ms_per_frame_min_max"] = [res[k]["min"] / per[k], res[k]["max"] / per[k]]
    for slow in ("bgr8_host_png", "bgr8_host_pil_jpeg"):
        res[f"{slow}_over_animate_to_video"] = verdict(res, "animate_to_video", slow)
    res["encode_to_host_over_encode_launches"] = verdict(res, "encode_launches", "encode_to_host", 20 * K, K)
    res["animate_to_video_over_render_bgr8"] = verdict(res, "render_bgr8", "animate_to_video")
    out["times"] = res
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
