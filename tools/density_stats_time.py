"""Times the densification statistics on the GPU box:  python tools/density_stats_time.py [--reps N] [--calls K] [--steps S] [--out FILE]

At N = 150 000 and 102 146 Gaussians, K = 1 and 8 frames per step, about two thirds of the rows visible per frame:

    launch        ``sings_amd.density.densify_stats`` (one launch, gate open; gate closed) against the torch chain of
                  ``AvatarStep.add_densification_stats`` on the same tensors: back-to-back calls between two HIP events, blocks of
                  ``--calls`` calls, ``--reps`` blocks in alternation; the median per call and the spread (min .. max) of the blocks.
    the step      the captured training step (the bench's avatar, fused optimiser, learned poses of 300 frames, ``step_frames`` with K
                  frames) under three settings of ONE trainer, captured again at every switch: the torch statistics (``stats_gate``
                  None, as the parent commit's step), the fused launch with the gate open, and with the gate closed.  Wall clock per
                  step over blocks of ``--steps`` steps, ``--reps`` blocks per setting and round, two rounds in alternation.  A
                  difference is resolved when the medians differ by more than the blocks' spread.

Back-to-back calls are bound by the host's enqueue, not by the kernels: the kernels' own time comes from a kernel trace of ``--trace``
(200 calls of each kind at each size), in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o density -- python3 tools/density_stats_time.py --trace

Writes profiles/density_stats_time.json (``--out``)."""
import argparse
import json
import math
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from sings_amd import grad_arena, overflow                        # noqa: E402
from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField      # noqa: E402
from sings_amd.density import densify_stats                       # noqa: E402
from sings_amd.pose import PoseTable                              # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings   # noqa: E402
from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm     # noqa: E402
from sings_amd.scene import avatar_scene                          # noqa: E402
from sings_amd.train_loop import AvatarTrainer                    # noqa: E402
from sings_amd.train_step import AvatarStep                       # noqa: E402

LRS = {"xyz": 3.2e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3, "global_orient": 1e-4, "body_pose": 1e-4}
F_FRAMES = 300
SIZES = (150000, 102146)
FRAMES = (1, 8)
SETTINGS = ("torch", "fused_open", "fused_closed")


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


def launch_case(N, K, dev):
    """-> {name: fn(i)} over one set of tensors: the fused launch (gate open / closed / none) and the module's torch chain."""
    g = torch.Generator(dev).manual_seed(N + K)
    grad = torch.randn((K, N, 3), device=dev, generator=g) * 1e-3
    radii = torch.randint(1, 200, (K, N), device=dev, generator=g, dtype=torch.int32)
    radii[torch.rand((K, N), device=dev, generator=g) < 1 / 3] = 0
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    holder = types.SimpleNamespace(xyz_gradient_accum=z(N, 1), denom=z(N, 1), max_radii2D=z(N), stats_gate=None)
    extras = {"viewspace_points": types.SimpleNamespace(grad=grad), "radii": radii}
    opened, closed = torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    fused = lambda gate: (lambda i: densify_stats(grad, radii, holder.xyz_gradient_accum, holder.denom, holder.max_radii2D, gate=gate))
    return {"torch_chain": lambda i: AvatarStep.add_densification_stats(holder, extras), "fused_open": fused(opened),
            "fused_closed": fused(closed), "fused_no_gate": fused(None)}


def build_trainer(dev, N, K):
    """The bench's training workload (benchkit/leg_train.py) with learned poses of 300 frames, K frames per step; -> (trainer, step(i))."""
    s = avatar_scene(N=N, J=52)
    W, H = s["W"], s["H"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cam = s["cam"]
    consts = dict(bg=t(s["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

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
                       optimizer="fused", poses=table)
    g = torch.Generator(dev).manual_seed(2)
    gt = torch.rand((K, 3, H, W), device=dev, generator=g)
    mask = torch.rand((K, H, W), device=dev, generator=g)
    if K == 1:
        return tr, (lambda i: tr.step_frames((7 * i) % F_FRAMES, gt[0], mask[0]))
    return tr, (lambda i: tr.step_frames([(7 * i + k) % F_FRAMES for k in range(K)], gt, mask))


def warm_up(tr, step, n=6):
    """Sizing steps (the first time), the capture, replays.  The capture runs the body three more times than the sizing steps did; on
    noise frames the pair count can outgrow their hint meanwhile -- the library then doubles the hint and says so: capture once more."""
    for attempt in range(2):
        try:
            for i in range(n):
                step(i)
            return
        except RuntimeError as e:
            if attempt or "more than its capacity" not in str(e):
                raise
            tr.captured = None


def set_statistics(tr, setting, gates):
    """The module's opt-in, by hand (no schedule: the gate's word stays what it is set to here); the graph is captured again."""
    tr.m.stats_gate = None if setting == "torch" else gates[setting]
    tr.captured = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--trace", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_stats_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "density_stats_time.py needs the GPU"
    dev = torch.device("cuda:0")
    if a.trace:
        for N in SIZES:
            for K in FRAMES:
                for name, fn in launch_case(N, K, dev).items():
                    for i in range(200):
                        fn(i)
                    torch.cuda.synchronize()
        return
    out = {"reps": a.reps, "calls_per_block": a.calls, "steps_per_block": a.steps, "device_name": torch.cuda.get_device_name(0),
           "launch": {}, "captured_step": {}}
    for N in SIZES:
        for K in FRAMES:
            fns = launch_case(N, K, dev)
            res = {k: [] for k in fns}
            for r in range(a.reps + 2):
                row = [event_block(fn, a.calls) for fn in fns.values()]
                if r >= 2:
                    for k, v in zip(res, row):
                        res[k].append(v)
            out["launch"][f"N{N}_K{K}"] = {**{k + "_ms": stats(v) for k, v in res.items()},
                                          "chain_against_fused_open": verdict(res["fused_open"], res["torch_chain"]),
                                          "open_against_closed": verdict(res["fused_closed"], res["fused_open"])}
    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    dump()                                                        # (the launches' numbers are kept whatever the step half does)
    # ---- the captured step under the three settings: one trainer per (N, K), the settings in alternation
    if not a.skip_step:
        gates = {"fused_open": torch.ones(1, dtype=torch.int32, device=dev), "fused_closed": torch.zeros(1, dtype=torch.int32, device=dev)}
        try:
            for N in SIZES:
                for K in FRAMES:
                    tr, step = build_trainer(dev, N, K)
                    ms = {k: [] for k in SETTINGS}
                    for _ in range(2):
                        for k in SETTINGS:
                            set_statistics(tr, k, gates)
                            warm_up(tr, step)
                            assert tr.captured is not None
                            ms[k] += [wall_block(step, a.steps) for _ in range(a.reps)]
                    out["captured_step"][f"N{N}_K{K}"] = {
                        **{k + "_wall_ms": stats(v) for k, v in ms.items()},
                        "torch_against_fused_open": verdict(ms["fused_open"], ms["torch"]),
                        "torch_against_fused_closed": verdict(ms["fused_closed"], ms["torch"]),
                        "open_against_closed": verdict(ms["fused_closed"], ms["fused_open"])}
                    del tr, step
                    overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
                    grad_arena.set_gradient_arena(None, None)
        finally:
            overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
            grad_arena.set_gradient_arena(None, None)
    dump()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
