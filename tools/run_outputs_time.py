"""Times a run's pictures on the GPU box:  python tools/run_outputs_time.py [--reps N] [--out FILE] [--skip-trainer]

    the sheet launch     ``sheets.image_sheets`` (csrc/sg_sheet.hip) against the torch-op chain it replaces, at 512 x 896 and 256 x 256:
                         K = 8 validation pairs (``validate.comparison_grid`` + quantise + permute, per frame, against ONE
                         ``run_outputs.validation_grids`` launch) and the progress sheet of four images (a zero grid, four slice copies,
                         quantise, permute, against one pair-form launch).  The inputs rotate over a pool larger than the Infinity Cache.
                         The launch's byte floor is 15 B per tile pixel + 3 B per border pixel; the fraction of this run's copy rate
                         (``benchkit.roofline.measure_copy_peak``) it reaches is reported.
    the turntable        ``canonical.render_canonical`` at the reference's size -- 60 orbit cameras, 512 x 512, the bench's
                         ``avatar_scene(150 000, J=52)`` -- posed once and rendered 8 cameras per launch, against the per-frame path it
                         replaces: 60 ``get_render_pkg_fused`` calls on the same cameras, each frame quantised by its own launch.  Both
                         in ms per turntable and in images per second; "render only" leaves the quantisation out of both arms.
    a run                ``trainer.run`` over two ``viz_interval``s (tests/test_gpu_frame_feed_train.py's trainer: 4 000 Gaussians, 128 x 224,
                         graph on) with and without ``set_outputs``, the writer stubbed out: the device and copy cost of an output event
                         (60 turntable frames at 512 x 512, the training picture, the splat file's host work, progress sheets).

Every timed block starts and ends in a device synchronise and is bracketed by HIP events; warm-up first; the two arms of a comparison
ALTERNATE block by block; medians over ``--reps`` (>= 5) blocks with min and max, and a difference counts as resolved only when the two
arms' [min, max] ranges do not overlap.  Writes profiles/run_outputs_time.json (``--out``)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from sings_amd import canonical as cn                             # noqa: E402
from sings_amd.run_outputs import RunOutputs, validation_grids    # noqa: E402
from sings_amd.sheets import image_sheets, sheet_geometry         # noqa: E402

SIZES = ((512, 896), (256, 256))
POOL_BYTES = 600e6


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), res


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


def verdict(res, fast, slow):
    """The ratio of the medians and whether the blocks' spread resolves it."""
    f, s = res[fast], res[slow]
    return {"ratio": s["median_ms"] / f["median_ms"], "resolved": bool(f["max"] < s["min"] or s["max"] < f["min"]),
            "faster": fast if f["median_ms"] < s["median_ms"] else slow}


def torch_validation_grids(gt, pred):
    from sings_amd.validate import comparison_grid
    out = []
    for k in range(gt.shape[0]):
        grid = comparison_grid(gt[k], pred[k])
        out.append((grid * 255 + 0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous())
    return out


def torch_progress_sheet(imgs):
    """make_grid(nrow=4, pad_value=0) of four [3,H,W] images by geometry, then save_image's bytes."""
    H, W = int(imgs.shape[-2]), int(imgs.shape[-1])
    Hs, Ws, _, _ = sheet_geometry(4, H, W, 4, 2)
    grid = torch.zeros((3, Hs, Ws), dtype=imgs.dtype, device=imgs.device)
    for t in range(4):
        grid[:, 2:2 + H, 2 + t * (W + 2):2 + t * (W + 2) + W] = imgs[t]
    return (grid * 255 + 0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def torch_frames(x):
    """save_image's bytes of [K,3,H,W] frames: quantise, permute to HWC."""
    return (x * 255 + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def sheet_times(dev, W, H, reps, copy_gbs):
    hw = H * W
    sets = max(2, int(POOL_BYTES // (2 * 8 * 12 * hw)))             # sets of 8 pairs in the pool
    g = torch.Generator(device=dev).manual_seed(W + H)
    gt = torch.rand((sets, 8, 3, H, W), device=dev, generator=g)
    pred = gt + 0.1 * torch.randn((sets, 8, 3, H, W), device=dev, generator=g)
    out = {"pool_sets": sets}
    # the two agree before anything is timed
    a, b = validation_grids(gt[0], pred[0]), torch.stack(torch_validation_grids(gt[0], pred[0]))
    out["validation_bytes_that_differ"] = int((a != b).sum())
    half, full = pred[0, 0:4:2], pred[0, 1:4:2]
    a = image_sheets(half.contiguous(), full.contiguous(), nrow=4, padding=2, pad_value=0.0, quant="round")[0]
    out["progress_bytes_that_differ"] = int((a != torch_progress_sheet(pred[0, :4])).sum())
    passes = max(1, 400 // sets)                                    # (about 400 launches per timed block)
    out["passes_per_block"] = passes
    sweep = lambda fn, n: (lambda: [fn(i % n) for i in range(n * passes)])

    def per_launch(res, n, floor, what):
        for k in ("device", "torch"):
            res[k]["us_per_" + what] = res[k]["median_ms"] * 1e3 / (n * passes)
            res[k]["us_min"], res[k]["us_max"] = res[k]["min"] * 1e3 / (n * passes), res[k]["max"] * 1e3 / (n * passes)
        res["device"]["byte_floor_per_launch"] = floor
        res["device"]["GBs"] = floor / (res["device"]["us_per_" + what] * 1e-6) / 1e9
        res["device"]["fraction_of_copy_rate"] = res["device"]["GBs"] / copy_gbs
        res["torch_over_device"] = verdict(res, "device", "torch")
        return res

    res = alternate({"device": sweep(lambda i: validation_grids(gt[i], pred[i]), sets),
                     "torch": sweep(lambda i: torch_validation_grids(gt[i], pred[i]), sets)}, reps)
    Hs, Ws, _, _ = sheet_geometry(2, H, W, 2, 2)
    out["validation_K8"] = per_launch(res, sets, 8 * (2 * hw * 12 + Hs * Ws * 3), "8_pairs")
    fours = pred.reshape(sets * 2, 4, 3, H, W)
    halves, fulls = fours[:, 0::2].contiguous(), fours[:, 1::2].contiguous()
    n = int(fours.shape[0])
    res = alternate({"device": sweep(lambda i: image_sheets(halves[i], fulls[i], nrow=4, padding=2, pad_value=0.0, quant="round"), n),
                     "torch": sweep(lambda i: torch_progress_sheet(fours[i]), n)}, reps)
    Hs, Ws, _, _ = sheet_geometry(4, H, W, 4, 2)
    out["progress_sheet"] = per_launch(res, n, 4 * hw * 12 + Hs * Ws * 3, "sheet")
    # eight frames, one tile per sheet, no padding (a turntable launch's frames): every thread takes the 16-byte loads
    a, b = image_sheets(gt[0], tiles_per_sheet=1, padding=0, quant="round"), torch_frames(gt[0])
    out["frames_bytes_that_differ"] = int((a != b).sum())
    res = alternate({"device": sweep(lambda i: image_sheets(gt[i], tiles_per_sheet=1, padding=0, quant="round"), sets),
                     "torch": sweep(lambda i: torch_frames(gt[i]), sets)}, reps)
    out["frames_K8"] = per_launch(res, sets, 8 * hw * 15, "8_frames")
    return out


def turntable_times(dev, reps, nframes=60, size=512, N=150000, J=52):
    from sings_amd import rasterizer as rz
    from sings_amd.body import joint_transforms
    from sings_amd.camera import get_rotating_camera
    from sings_amd.renderer import get_render_pkg_fused
    from sings_amd.scene import avatar_scene
    s = avatar_scene(N=N, J=J, W=size, H=size, seed=4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    canon = dict(xyz_canon=t(s["xyz_canon"]), rotmat_canon=None, scales=t(s["scales"]), opacity=t(s["opacities"]), shs=t(s["shs"]),
                 lbs_weights=t(s["lbs_weights"]), active_sh_degree=0)
    pose = np.zeros(J * 3, np.float32); pose[3:72] = cn.predefined_pose("da_pose").numpy()
    A = joint_transforms(t(pose), t(s["joints_rest"]), tuple(s["parents"]))
    bg = torch.ones(3, device=dev)
    cams = get_rotating_camera(img_size=size, device=dev, nframes=nframes)
    posed = cn.pose_once(canon, A, cams[0], bg)
    orbit = cn.OrbitRenderer(posed, size, size, int(canon["shs"].shape[1]), K=8, device=dev)

    def orbit_frames():
        return [u8 for _, u8 in cn.render_canonical_chunks(canon, A, bg, cameras=cams, renderer=orbit)]

    def orbit_render():
        p = cn.pose_once(canon, A, cams[0], bg)
        return [raw for _, _, raw in orbit.chunks(p, cams, bg)]

    def fused_render():
        with torch.no_grad():
            return [get_render_pkg_fused(c, canon, A, bg)["render_raw"] for c in cams]

    def fused_frames():
        return [image_sheets(raw, tiles_per_sheet=1, padding=0, quant="round")[0] for raw in fused_render()]

    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    a, b = torch.cat(orbit_frames()), torch.stack(fused_frames())
    out = {"nframes": nframes, "size": size, "N": N, "J": J, "K": 8, "bytes_that_differ_from_the_fused_loop": int((a != b).sum()),
           "largest_byte_difference": int((a.int() - b.int()).abs().max()), "bytes": int(a.numel()),
           "not_background": bool((a != 255).any()), "pair_capacity": orbit.cap, "launches_per_turntable": -(-nframes // 8),
           "redone_launches": orbit.redone}
    res = alternate({"pose_once_K8": orbit_frames, "per_frame_fused": fused_frames}, reps)
    for k in res:
        res[k]["images_per_s"] = nframes / (res[k]["median_ms"] * 1e-3)
    res["per_frame_over_pose_once"] = verdict(res, "pose_once_K8", "per_frame_fused")
    out["frames"] = res
    res = alternate({"pose_once_K8": orbit_render, "per_frame_fused": fused_render}, reps)
    for k in res:
        res[k]["images_per_s"] = nframes / (res[k]["median_ms"] * 1e-3)
    res["per_frame_over_pose_once"] = verdict(res, "pose_once_K8", "per_frame_fused")
    out["render_only"] = res
    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    return out


def trainer_times(dev, reps, viz_interval=10):
    """Fresh trainers per block (a run moves the parameters on): ``2 * viz_interval + 1`` steps, iterations 0 .. 2 viz_interval, so three
    output events with outputs.  The first block of each arm, which also pays the graph capture, is the warm-up."""
    from sings_amd import frame_feed as ff
    from test_gpu_frame_feed_train import SEED, STILL_LRS, _feed_trainer, _quantised, _reset
    from test_gpu_pose_train import _pose_scene
    sc = _pose_scene()
    rgb_u8, mask_u8 = _quantised(sc, dev)
    _reset()
    store = ff.FrameStore(rgb_u8, mask_u8, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A = cn.static_A("da_pose", t(sc["joints"]), torch.inverse(t(sc["post"])), sc["parents"])
    steps, sink, logdir = 2 * viz_interval + 1, [], tempfile.mkdtemp()       # (directories only: the writer is a stub)

    def block(with_outputs):
        tr = _feed_trainer(sc, dev, "fused", True, ff.FrameFeed(store, seed=SEED), lrs=STILL_LRS)
        if with_outputs:
            tr.set_outputs(RunOutputs(logdir, A, torch.ones(3, device=dev), viz_interval=viz_interval,
                                      progress_interval=viz_interval, save_ply=False, write=lambda path, array: sink.append(array.nbytes)))
        ms, _ = timed(lambda: tr.run(steps))
        _reset()
        return ms

    ms = {True: [], False: []}
    for rep in range(reps + 1):
        for w in (False, True):
            m = block(w)
            if rep:
                ms[w].append(m)
    res = {("with_outputs" if w else "plain"): {"median_ms": statistics.median(v), "min": min(v), "max": max(v)} for w, v in ms.items()}
    events = 3
    res["ms_per_output_event"] = (res["with_outputs"]["median_ms"] - res["plain"]["median_ms"]) / events
    res["outputs_over_plain"] = verdict(res, "plain", "with_outputs")
    res.update(steps=steps, viz_interval=viz_interval, output_events=events, gaussians=int(sc["xyz"].shape[0]),
               host_bytes_per_event=sum(sink) // max(1, (reps + 1) * events), save_ply=False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "run_outputs_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "run_outputs_time.py needs the GPU"
    from benchkit.roofline import measure_copy_peak
    dev = torch.device("cuda:0")
    out = {"reps": a.reps, "device_name": torch.cuda.get_device_name(0), "copy_GBs": measure_copy_peak(dev)}
    for W, H in SIZES:
        out[f"sheets_{W}x{H}"] = sheet_times(dev, W, H, a.reps, out["copy_GBs"])
        torch.cuda.empty_cache()
    out["turntable"] = turntable_times(dev, a.reps)
    torch.cuda.empty_cache()
    if not a.skip_trainer:
        out["trainer"] = trainer_times(dev, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
