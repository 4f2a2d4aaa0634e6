"""Cost of the depth / alpha maps on the K-frame path, on the GPU box: python tools/aux_frames_time.py [--reps N] [--K 8]

The cfg4 avatar (150 k Gaussians, 512 x 896, SH degree 0, J = 52) as ONE K-frame launch per direction, forward + backward timed with
device events: rasterize_skinned_frames with return_aux False (loss on colour) and True (loss on colour, depth and alpha: the
backward runs the AUX kernels).  The two legs alternate rep by rep in one process (same clocks, same caches); prints the median ms
per launch and per frame and the ratio."""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sings_amd.body import joint_transforms  # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings  # noqa: E402
from sings_amd.scene import avatar_scene  # noqa: E402
from sings_amd.skinned import rasterize_skinned_frames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--K", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = args.K
    s = avatar_scene(N=150000, J=52)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = s["cam"]
    rs = GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5),
        bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]), projmatrix=t(cam["full_proj_transform"]),
        sh_degree=0, campos=t(cam["camera_center"]), prefiltered=False, debug=False)
    J = s["J"]
    g = np.random.RandomState(7)
    A = torch.stack([joint_transforms(t(g.normal(0, 0.15, J * 3).astype(np.float32)), t(s["joints_rest"]), tuple(s["parents"]))
                     .reshape(J, 16) for _ in range(K)]).contiguous().requires_grad_(True)
    tr = t((s["transl"][None] + g.normal(0, 0.02, (K, 3))).astype(np.float32)).requires_grad_(True)
    xyz, sc, op = t(s["xyz_canon"]).requires_grad_(True), t(s["scales"]).requires_grad_(True), t(s["opacities"]).requires_grad_(True)
    sh = t(s["shs"]).requires_grad_(True)
    w, ss = t(s["lbs_weights"]), t(s["smpl_scale"])
    H, W = s["H"], s["W"]
    dL = torch.randn(K, 3, H, W, device=dev)
    gD, gA = torch.randn(K, 1, H, W, device=dev), torch.randn(K, 1, H, W, device=dev)

    def plain():
        c, _ = rasterize_skinned_frames(xyz, None, sc, op, sh, w, A, rs, smpl_scale=ss, transl=tr)
        (c * dL).sum().backward()

    def aux():
        c, _, d, a = rasterize_skinned_frames(xyz, None, sc, op, sh, w, A, rs, smpl_scale=ss, transl=tr, return_aux=True)
        ((c * dL).sum() + (d * gD).sum() + (a * gA).sum()).backward()

    for _ in range(5):
        plain(); aux()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
          for k in ("plain", "aux")}
    for i in range(args.reps):                     # alternate the two legs
        for k, fn in (("plain", plain), ("aux", aux)):
            a, b = ev[k][i]
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    med = {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}
    print(f"skinned cfg4 avatar 150k 512x896 K={K} one launch: fwd+bwd plain {med['plain']:.3f} ms ({med['plain'] / K:.3f} per frame), "
          f"with depth/alpha {med['aux']:.3f} ms ({med['aux'] / K:.3f} per frame), ratio {med['aux'] / med['plain']:.3f}", flush=True)


if __name__ == "__main__":
    main()
