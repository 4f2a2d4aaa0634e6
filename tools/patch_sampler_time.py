"""Times the LPIPS patch sampler on the GPU box:  python tools/patch_sampler_time.py [--reps N] [--calls K] [--steps S] [--out FILE]

At 512 x 896 and at 1920 x 1080, n = 4, P = 128, a random mask of density 0.3:

    host          ``sings_amd.lpips.PatchSampler.origins`` (the mask copied to the host, ``np.where`` over every pixel) plus the upload
                  of its four corners: wall clock per call between two device synchronises -- the path a step had before.
    device        ``DevicePatchSampler.origins``: the launch pair between two HIP events, blocks of ``--calls`` calls, ``--reps`` blocks;
                  the median per call and the spread (min .. max) of the blocks.  Also the pair replayed from a HIP graph.
    the step      ``AvatarTrainer.step`` with the LPIPS term (150 000 Gaussians, 512 x 896, fused optimiser, captured), fed by each
                  sampler: ``lpips_sampler=`` (the draw inside the graph) against host corners passed as ``lpips_origins=`` (drawn from
                  the device mask, uploaded, copied in front of the replay).  Wall clock per step over blocks of ``--steps`` steps --
                  the host sampler's cost is host time, which events on the stream do not see; the two trainers are built twice each,
                  in alternation.  The difference is resolved when the medians differ by more than the blocks' spread.

Back-to-back calls are bound by the host's enqueue (a Python call and two launches) and a replay by the graph launch, not by the two
kernels: their own time comes from a kernel trace of ``--trace`` (200 draws at each size, nothing else), in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o sampler -- python3 tools/patch_sampler_time.py --trace

Writes profiles/patch_sampler_time.json (``--out``)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

import lpips_case as lc                                           # noqa: E402
from sings_amd import grad_arena, overflow                        # noqa: E402
from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField      # noqa: E402
from sings_amd.lpips import LPIPS, PatchSampler                   # noqa: E402
from sings_amd.patch_sampler import DevicePatchSampler            # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings   # noqa: E402
from sings_amd.scene import avatar_scene                          # noqa: E402
from sings_amd.train_loop import AvatarTrainer                    # noqa: E402
from sings_amd.train_step import AvatarStep                       # noqa: E402

LRS = {"xyz": 3.2e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}
N_PATCH, PATCH, RATIO, DENSITY = 4, 128, 0.9, 0.3


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
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def wall_block(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def build_trainer(dev, device_sampler):
    s = avatar_scene()
    W, H = s["W"], s["H"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cam = s["cam"]
    consts = dict(bg=t(s["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    torch.manual_seed(0)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [64, 64, 64], 'multires': [1, 2, 4]}
    tri = HexPlaneField(cfg, bounds=1.2, device=dev, feature_minor=True)
    geo = GeometryDecoder(96).to(dev); app = AppearanceDecoder(96).to(dev)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-5.3); geo.scales[2].weight.mul_(0.1)
        geo.xyz_offsets.weight.mul_(0.01); geo.xyz_offsets.bias.zero_()
    wt = lc.make_weights(0)
    lp = LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"], device=dev)
    mod = AvatarStep(t(s["xyz_canon"]), t(s["lbs_weights"]), tri, geo, app, lpips=lp, lpips_w=1.0, lpips_patch_size=PATCH).to(dev)
    A = torch.eye(4, device=dev).repeat(52, 1, 1).contiguous()
    gt = torch.rand((3, H, W), device=dev)
    mask = (torch.rand((H, W), device=dev, generator=torch.Generator(dev).manual_seed(1)) < DENSITY).float()
    sampler = DevicePatchSampler(N_PATCH, PATCH, RATIO, seed=3, device=dev) if device_sampler else None
    tr = AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), use_graph=True,
                       sh_degree=0, max_sh_degree=0, optimizer="fused", lpips_sampler=sampler)
    if device_sampler:
        return tr, (lambda: tr.step(A, gt, mask))
    host = PatchSampler(N_PATCH, PATCH, RATIO)
    return tr, (lambda: tr.step(A, gt, mask, lpips_origins=torch.from_numpy(host.origins(mask))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--trace", action="store_true", help="only 200 draws at each size, for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_sampler_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "patch_sampler_time.py needs the GPU"
    dev = torch.device("cuda:0")
    if a.trace:
        for W, H in ((512, 896), (1920, 1080)):
            mask = (torch.rand((H, W), device=dev, generator=torch.Generator(dev).manual_seed(1)) < DENSITY).float()
            devs = DevicePatchSampler(N_PATCH, PATCH, RATIO, seed=3, device=dev)
            for _ in range(200):
                devs.origins(mask)
            torch.cuda.synchronize()
        return
    out = {"n": N_PATCH, "patch_size": PATCH, "ratio_mask": RATIO, "mask_density": DENSITY, "reps": a.reps, "calls_per_block": a.calls,
           "steps_per_block": a.steps, "device_name": torch.cuda.get_device_name(0), "sizes": {}}
    np.random.seed(0)
    for W, H in ((512, 896), (1920, 1080)):
        mask = (torch.rand((H, W), device=dev, generator=torch.Generator(dev).manual_seed(1)) < DENSITY).float()
        host, devs = PatchSampler(N_PATCH, PATCH, RATIO), DevicePatchSampler(N_PATCH, PATCH, RATIO, seed=3, device=dev)
        upload = lambda: torch.from_numpy(host.origins(mask)).to(dev)
        draw = lambda: devs.origins(mask)
        draw(); upload()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            draw()
        res = {"host_wall": [], "device_events": [], "device_graph_events": [], "device_wall": []}
        for r in range(a.reps + 2):
            row = (wall_block(upload, 10), event_block(draw, a.calls), event_block(g.replay, a.calls), wall_block(draw, a.calls))
            if r >= 2:
                for k, v in zip(res, row):
                    res[k].append(v)
        out["sizes"][f"{W}x{H}"] = {"mask_bytes": 4 * W * H, "chunks": -(-(H - PATCH) * (W - PATCH) // 4096),
                                    **{k + "_ms": stats(v) for k, v in res.items()},
                                    "device_against_host": verdict(res["device_events"], res["host_wall"])}

    # ---- the captured step with the term, fed by each sampler: one trainer at a time (they share the module-level gradient arena)
    if not a.skip_step:
        steps = {"device_sampler": [], "host_sampler": []}
        try:
            for _ in range(2):
                for k in steps:
                    tr, step = build_trainer(dev, k == "device_sampler")
                    for _ in range(6):                            # sizing steps, the capture, replays
                        step()
                    assert tr.captured is not None
                    steps[k] += [wall_block(step, a.steps) for _ in range(a.reps)]
                    del tr, step
                    overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
                    grad_arena.set_gradient_arena(None, None)
            out["captured_step_wall_ms"] = {k: stats(x) for k, x in steps.items()}
            out["captured_step_host_against_device"] = verdict(steps["device_sampler"], steps["host_sampler"])
        finally:
            overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
            grad_arena.set_gradient_arena(None, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
