"""Cost of the depth / alpha maps on the GPU box: python tools/aux_time.py [--reps N]

One view forward + backward, timed with device events, without and with the maps:
 * the drop-in op at cfg3 (200 k Gaussians, 1920 x 1080, SH degree 3): GaussianRasterizer.forward vs .forward_aux;
 * the skinned op at the cfg4 avatar (150 k, 512 x 896, SH degree 0): rasterize_skinned_gaussians with return_aux False / True.
The aux legs put a loss on colour, depth and alpha (so the backward runs the AUX kernels).  Prints ms per view and the ratio."""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sings_amd.body import joint_transforms  # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402
from sings_amd.scene import avatar_scene, synthetic_scene  # noqa: E402
from sings_amd.skinned import rasterize_skinned_gaussians  # noqa: E402


def _time(step, reps, warmup=5):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); step(); b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def drop_in(dev, reps):
    s = synthetic_scene(200000, 1920, 1080, 3, 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs = GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]), scale_modifier=1.0,
        viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]), sh_degree=3, campos=t(s["campos"]), prefiltered=False,
        debug=False)
    r = GaussianRasterizer(rs)
    x = {k: t(s[k]).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    m2 = torch.zeros_like(x["means3D"], requires_grad=True)
    dL, gD, gA = t(s["dL_dimage"]), torch.randn(1, s["H"], s["W"], device=dev), torch.randn(1, s["H"], s["W"], device=dev)

    def plain():
        c, _ = r(means2D=m2, **x)
        (c * dL).sum().backward()

    def aux():
        c, _, d, a = r.forward_aux(means2D=m2, **x)
        ((c * dL).sum() + (d * gD).sum() + (a * gA).sum()).backward()
    return _time(plain, reps), _time(aux, reps)


def skinned(dev, reps):
    s = avatar_scene(N=150000, J=52)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = s["cam"]
    rs = GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5),
        bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]), projmatrix=t(cam["full_proj_transform"]),
        sh_degree=0, campos=t(cam["camera_center"]), prefiltered=False, debug=False)
    J = s["J"]
    A = joint_transforms(torch.zeros(J * 3, device=dev), t(s["joints_rest"]), tuple(s["parents"])).detach().requires_grad_(True)
    xyz, sc, op = t(s["xyz_canon"]).requires_grad_(True), t(s["scales"]).requires_grad_(True), t(s["opacities"]).requires_grad_(True)
    sh = t(s["shs"]).requires_grad_(True)
    w, tr, ss = t(s["lbs_weights"]), t(s["transl"]).requires_grad_(True), t(s["smpl_scale"])
    dL, gD, gA = t(s["dL_dimage"]), torch.randn(1, s["H"], s["W"], device=dev), torch.randn(1, s["H"], s["W"], device=dev)

    def plain():
        c, _ = rasterize_skinned_gaussians(xyz, None, sc, op, sh, w, A, rs, smpl_scale=ss, transl=tr)
        (c * dL).sum().backward()

    def aux():
        c, _, d, a = rasterize_skinned_gaussians(xyz, None, sc, op, sh, w, A, rs, smpl_scale=ss, transl=tr, return_aux=True)
        ((c * dL).sum() + (d * gD).sum() + (a * gA).sum()).backward()
    return _time(plain, reps), _time(aux, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, fn in (("drop-in cfg3 200k 1920x1080 deg3", drop_in), ("skinned cfg4 avatar 150k 512x896", skinned)):
        p, a = fn(dev, args.reps)
        print(f"{name}: fwd+bwd plain {p:.3f} ms, with depth/alpha {a:.3f} ms, ratio {a / p:.3f}", flush=True)


if __name__ == "__main__":
    main()
