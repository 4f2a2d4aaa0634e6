"""Times the optimiser step of the training loop on the GPU box:  python tools/optim_time.py [--reps N] [--steps K] [--out FILE]

At the sizes of ``bench.py --workload train`` (150 k anchors, tri-plane 32 x (64, 128, 256)^2 x 3 feature-minor, decoders 96-128-128 /
96-64-64, L2Norm + Gaussian edge regularisers), medians of ``--reps`` repetitions after warm-up:

  (a) ``torch.optim.Adam.step()`` alone (what ``AvatarTrainer`` calls by default): host wall time per call (ends in a device
      synchronise) and GPU time (HIP events around the call)
  (b) ``FusedAdam.step()`` alone, the same two figures
  (c) ``AvatarTrainer.step`` end to end, torch + graph against fused + graph: blocks of ``--steps`` steps, the two alternating
  (d) the Adam kernel alone (32 launches between two events): its 28 B per element over its time, as a fraction of the float4-copy
      rate ``sg_copy_probe`` gives in the same run (bytes = read + written on both sides)

Writes profiles/optim_time.json (``--out``)."""
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

from benchkit.roofline import measure_copy_peak                  # noqa: E402
from sings_amd import _marshal, overflow                         # noqa: E402
from sings_amd.body import joint_transforms                      # noqa: E402
from sings_amd.decode import (AppearanceDecoder, GeometryDecoder, HexPlaneField, overlap_weight_grads,   # noqa: E402
                              prepare_triplane_backward_early, set_gradient_arena)
from sings_amd.rasterizer import GaussianRasterizationSettings   # noqa: E402
from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm     # noqa: E402
from sings_amd.scene import avatar_scene                         # noqa: E402
from sings_amd.train_loop import AvatarTrainer                   # noqa: E402
from sings_amd.train_step import AvatarStep                      # noqa: E402

LRS = {"xyz": 3.2e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}        # defaults/config.py:62-84


def build(dev, N, optimizer, use_graph):
    """The bench's training workload (benchkit/leg_train.py) behind an AvatarTrainer."""
    s = avatar_scene(N=N, J=52)
    W, H, J = s["W"], s["H"], s["J"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cam = s["cam"]
    consts = dict(bg=t(s["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    poses72 = np.load(os.path.join(ROOT, "tests", "golden", "lbs_golden.npz"))["amass_poses_72"]
    F = poses72.shape[0]
    poses = np.zeros((F, J * 3), np.float32); poses[:, :72] = poses72; poses[:, :3] = 0
    jr = t(s["joints_rest"])
    A_all = torch.stack([joint_transforms(t(poses[f]), jr, tuple(s["parents"])) for f in range(F)]).reshape(F, J, 4, 4).contiguous()
    torch.manual_seed(0)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [64, 64, 64], 'multires': [1, 2, 4]}
    tri = HexPlaneField(cfg, bounds=1.2, device=dev, feature_minor=True)
    geo = GeometryDecoder(96).to(dev); app = AppearanceDecoder(96).to(dev)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-5.3); geo.scales[2].weight.mul_(0.1)
        geo.xyz_offsets.weight.mul_(0.01); geo.xyz_offsets.bias.zero_()
    mod = AvatarStep(t(s["xyz_canon"]), t(s["lbs_weights"]), tri, geo, app, l2_norm=L2Norm(), gaussian_connect=GaussiansEdgeLoss(),
                     gaussian_connect_w=1.0, defer_regulariser_join=True).to(dev)
    gt = torch.rand((3, H, W), device=dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    mask = ((((xx - W / 2) / (W / 4)) ** 2 + ((yy - H / 2) / (H / 2.2)) ** 2) < 1).float().contiguous()
    tr = AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), use_graph=use_graph,
                       sh_degree=0, max_sh_degree=0, optimizer=optimizer)
    return tr, A_all, gt, mask


def call_times(fn, reps, warmup=5):
    """-> (median host wall ms per call, ending in a synchronise; median GPU ms between HIP events around the call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, gpu = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3); gpu.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(gpu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--gaussians", type=int, default=150000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_time.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    assert torch.cuda.is_available(), "optim_time.py needs the GPU"
    dev = torch.device("cuda:0")
    out = {"gaussians": a.gaussians, "reps": a.reps, "steps_per_block": a.steps, "device": torch.cuda.get_device_name(0)}
    out["copy_GBs"] = measure_copy_peak(dev)

    # ---- (c) end to end, first: the two trainers alternate in blocks (the torch trainer registers no arena, the fused one's stays)
    overlap_weight_grads(True); prepare_triplane_backward_early(True)          # (the bench's defaults)
    trainers = {}
    for name in ("torch_graph", "fused_graph"):
        trainers[name], A_all, gt, mask = build(dev, a.gaussians, "fused" if name.startswith("fused") else "torch", True)
    for i in range(8):                                            # sizing steps, the capture, replays
        for tr in trainers.values():
            tr.step(A_all[i % A_all.shape[0]], gt, mask)
    torch.cuda.synchronize()
    assert all(tr.captured is not None for tr in trainers.values())
    nparam = sum(p.numel() for p in trainers["fused_graph"].params)
    out["trainable_parameters"] = nparam
    blocks = {k: [] for k in trainers}
    F = A_all.shape[0]
    for rep in range(a.reps + 2):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                tr.step(A_all[(rep * a.steps + i) % F], gt, mask)
            torch.cuda.synchronize()
            if rep >= 2:
                blocks[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    for name, v in blocks.items():
        out[f"step_ms_{name}"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    overflow.check_deferred_overflow(dev)                         # (raises if a timed step overflowed the pair capacity)
    out["step_fused_over_torch"] = out["step_ms_fused_graph"]["median"] / out["step_ms_torch_graph"]["median"]

    # ---- (a) torch.optim.Adam.step() alone, on the torch trainer's parameters and the gradients of its last step
    tt = trainers["torch_graph"]
    wall, gpu = call_times(tt.opt.step, a.reps)
    out["torch_adam_step"] = {"wall_ms": wall, "gpu_ms": gpu}
    # ---- (b) FusedAdam.step() alone, on the fused trainer's
    tf = trainers["fused_graph"]
    wall, gpu = call_times(tf.opt.step, a.reps)
    out["fused_adam_step"] = {"wall_ms": wall, "gpu_ms": gpu}
    # ---- (d) the kernel alone: 32 launches between two events
    opt = tf.opt
    launch = lambda: _marshal.adam_step(opt.segments, opt.chunks, opt.hyper, opt.grad_flat, opt.exp_avg, opt.exp_avg_sq)
    ks = []
    for rep in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(32):
            launch()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ks.append(e0.elapsed_time(e1) / 32)
    kms = statistics.median(ks)
    gbs = 28.0 * nparam / (kms * 1e-3) / 1e9
    out["adam_kernel"] = {"ms": kms, "bytes": 28 * nparam, "GBs": gbs, "fraction_of_copy_rate": gbs / out["copy_GBs"],
                          "segments": int(opt.segments.shape[0]), "chunks": int(opt.chunks.shape[0])}
    overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
    set_gradient_arena(None, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
