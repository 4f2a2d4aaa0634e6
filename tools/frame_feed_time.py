"""Times the frame feed on the GPU box:  python tools/frame_feed_time.py [--reps N] [--calls K] [--steps S] [--out FILE]

At 512 x 896 and at 1920 x 1080, F = 300 frames of random bytes, one frame per step:

    feed          ``FrameFeed.draw()``: the launch pair between two HIP events, blocks of ``--calls`` calls, ``--reps`` blocks; the median
                  per call and the spread (min .. max) of the blocks.  Also the pair replayed from a HIP graph.
    copies        what the pair replaces in ``AvatarTrainer._step``: ``gt.copy_`` and ``mask.copy_`` from an fp32 cache (16 cached
                  frames, visited in turn: the copies' cost does not depend on F) plus the copy of the index, timed the same way.
    rebuild       a draw that has to rebuild the epoch's order (the held epoch set to -1 in front of every call, by a device-side
                  fill inside the timed region: the "held" row does the same fill on another tensor and keeps the epoch, so it
                  rebuilds once per F draws only) at F = 300 and at F = 16384.
    memory        ``FrameStore.nbytes`` next to the fp32 cache's 16 B per pixel.
    the step      the captured training step (150 000 Gaussians, 512 x 896, fused optimiser, learned poses of F = 300 frames):
                  ``step_next()`` against ``step_frames(i, gt, mask)`` fed from an fp32 cache on the device.  Wall clock per step over
                  blocks of ``--steps`` steps; the two trainers are built twice each, in alternation.  A difference is resolved when
                  the medians differ by more than the blocks' spread.

Back-to-back calls are bound by the host's enqueue and a replay by the graph launch, not by the kernels: their own time comes from a
kernel trace of ``--trace`` (200 draws at each size, then 20 forced rebuilds at F = 300 and at F = 16384), in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o feed -- python3 tools/frame_feed_time.py --trace

Writes profiles/frame_feed_time.json (``--out``)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from sings_amd import grad_arena, overflow                        # noqa: E402
from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField      # noqa: E402
from sings_amd.frame_feed import MAX_FRAMES, FrameFeed, FrameStore                  # noqa: E402
from sings_amd.pose import PoseTable                              # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings   # noqa: E402
from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm     # noqa: E402
from sings_amd.scene import avatar_scene                          # noqa: E402
from sings_amd.train_loop import AvatarTrainer                    # noqa: E402
from sings_amd.train_step import AvatarStep                       # noqa: E402

LRS = {"xyz": 3.2e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3, "global_orient": 1e-4, "body_pose": 1e-4}
F_FRAMES, CACHED = 300, 16
SIZES = ((512, 896), (1920, 1080))


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def verdict(a, b):
    """a against b (per-call ms of alternating blocks): resolved when the medians differ by more than the larger spread."""
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = statistics.median(b) - statistics.median(a)
    return {"difference_ms": diff, "spread_ms": spread, "resolved": abs(diff) > spread}


def event_block(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def wall_block(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def random_store(F, H, W, dev):
    g = torch.Generator(dev).manual_seed(1)
    data = torch.randint(0, 256, (F, H, W, 4), dtype=torch.uint8, device=dev, generator=g)
    return FrameStore(data[..., :3], data[..., 3], device=dev)


def build_trainer(dev, with_feed):
    """The bench's training workload (benchkit/leg_train.py) with learned poses of 300 frames; -> (trainer, step(i))."""
    s = avatar_scene(N=150000, J=52)
    W, H = s["W"], s["H"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cam = s["cam"]
    store = random_store(F_FRAMES, H, W, dev)
    feed = FrameFeed(store, seed=3) if with_feed else None
    consts = dict(bg=feed.bg if with_feed else t(s["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]),
                  campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    poses72 = np.load(os.path.join(ROOT, "tests", "golden", "lbs_golden.npz"))["amass_poses_72"].astype(np.float32)
    poses72[:, :3] = 0
    poses72 = np.tile(poses72, (-(-F_FRAMES // poses72.shape[0]), 1))[:F_FRAMES]
    torch.manual_seed(0)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [64, 64, 64], 'multires': [1, 2, 4]}
    tri = HexPlaneField(cfg, bounds=1.2, device=dev, feature_minor=True)
    geo = GeometryDecoder(96).to(dev); app = AppearanceDecoder(96).to(dev)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-5.3); geo.scales[2].weight.mul_(0.1)
        geo.xyz_offsets.weight.mul_(0.01); geo.xyz_offsets.bias.zero_()
    mod = AvatarStep(t(s["xyz_canon"]), t(s["lbs_weights"]), tri, geo, app, l2_norm=L2Norm(), gaussian_connect=GaussiansEdgeLoss(),
                     gaussian_connect_w=1.0, defer_regulariser_join=True).to(dev)
    table = PoseTable.from_axis_angle(t(poses72[:, :3]), t(poses72[:, 3:]), t(np.tile(s["transl"].reshape(1, 3), (F_FRAMES, 1))),
                                      t(s["joints_rest"]), parents=tuple(int(p) for p in s["parents"]), body="smplh")
    tr = AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(s["smpl_scale"]), use_graph=True, sh_degree=0, max_sh_degree=0,
                       optimizer="fused", poses=table, frames=feed)
    if with_feed:
        return tr, (lambda i: tr.step_next())
    gts, masks = store.frames(list(range(CACHED)))                # (the fp32 cache the parent's loop reads; 16 frames of it)
    return tr, (lambda i: tr.step_frames((7 * i) % F_FRAMES, gts[i % CACHED], masks[i % CACHED]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--trace", action="store_true", help="only draws and forced rebuilds, for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_feed_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "frame_feed_time.py needs the GPU"
    dev = torch.device("cuda:0")

    def rebuild_feed(F):
        feed = FrameFeed(random_store(F, 2, 2, dev), seed=3)
        held, dummy = feed.state[2:3], torch.zeros(1, dtype=torch.int64, device=dev)
        return feed, (lambda i: (held.fill_(-1), feed.draw())), (lambda i: (dummy.fill_(-1), feed.draw()))
    if a.trace:
        for W, H in SIZES:
            feed = FrameFeed(random_store(F_FRAMES, H, W, dev), seed=3)
            for _ in range(200):
                feed.draw()
            torch.cuda.synchronize()
        for F in (F_FRAMES, MAX_FRAMES):
            feed, forced, _ = rebuild_feed(F)
            for i in range(20):
                forced(i)
            torch.cuda.synchronize()
        return
    out = {"frames": F_FRAMES, "reps": a.reps, "calls_per_block": a.calls, "steps_per_block": a.steps,
           "device_name": torch.cuda.get_device_name(0), "sizes": {}, "rebuild": {}}
    for W, H in SIZES:
        store = random_store(F_FRAMES, H, W, dev)
        feed = FrameFeed(store, seed=3)
        gts, masks = store.frames(list(range(CACHED)))
        s_gt, s_mask, s_idx = torch.empty_like(gts[0]), torch.empty_like(masks[0]), torch.zeros(1, dtype=torch.int32, device=dev)
        host_idx = [torch.tensor([i], dtype=torch.int32) for i in range(CACHED)]
        draw = lambda i: feed.draw()
        copies = lambda i: (s_idx.copy_(host_idx[i % CACHED]), s_gt.copy_(gts[i % CACHED]), s_mask.copy_(masks[i % CACHED]))
        draw(0); copies(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            draw(0)
        res = {"feed_events": [], "feed_graph_events": [], "copies_events": [], "feed_wall": [], "copies_wall": []}
        for r in range(a.reps + 2):
            row = (event_block(draw, a.calls), event_block(lambda i: g.replay(), a.calls), event_block(copies, a.calls),
                   wall_block(draw, a.calls), wall_block(copies, a.calls))
            if r >= 2:
                for k, v in zip(res, row):
                    res[k].append(v)
        out["sizes"][f"{W}x{H}"] = {"store_nbytes": store.nbytes, "fp32_cache_nbytes": 16 * F_FRAMES * H * W,
                                    "bytes_per_pixel": store.nbytes / (F_FRAMES * H * W),
                                    **{k + "_ms": stats(v) for k, v in res.items()},
                                    "copies_against_feed": verdict(res["feed_events"], res["copies_events"])}
        del store, feed, gts, masks, g
    for F in (F_FRAMES, MAX_FRAMES):
        feed, forced, held = rebuild_feed(F)
        forced(0)
        res = {"rebuild_events": [], "held_events": []}
        for r in range(a.reps + 2):
            row = (event_block(forced, 50), event_block(held, 50))
            if r >= 2:
                for k, v in zip(res, row):
                    res[k].append(v)
        out["rebuild"][str(F)] = {**{k + "_ms": stats(v) for k, v in res.items()},
                                  "rebuild_against_held": verdict(res["held_events"], res["rebuild_events"])}

    # ---- the captured step, fed either way: one trainer at a time (they share the module-level gradient arena)
    if not a.skip_step:
        steps = {"step_next": [], "step_frames_fp32_cache": []}
        try:
            for _ in range(2):
                for k in steps:
                    tr, step = build_trainer(dev, k == "step_next")
                    for i in range(6):                            # sizing steps, the capture, replays
                        step(i)
                    assert tr.captured is not None
                    steps[k] += [wall_block(step, a.steps) for _ in range(a.reps)]
                    del tr, step
                    overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
                    grad_arena.set_gradient_arena(None, None)
            out["captured_step_wall_ms"] = {k: stats(x) for k, x in steps.items()}
            out["captured_step_frames_against_next"] = verdict(steps["step_next"], steps["step_frames_fp32_cache"])
        finally:
            overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
            grad_arena.set_gradient_arena(None, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
