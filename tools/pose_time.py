"""Times the learned-pose path on the GPU box:  python tools/pose_time.py [--reps N] [--steps K] [--out FILE]

  (a) the two launches alone (``sg_pose_transforms`` / ``_backward``, F = 80 rows): 32 launches between two HIP events, for
      K in {1, 16} frames and J in {24, 52} joints
  (b) the complete captured training step (fused Adam inside the graph) at the sizes of ``bench.py --workload train`` (150 k anchors,
      J = 52), one frame per step, three trainers taking turns in blocks of ``--steps`` steps:
        fixed     ``AvatarTrainer(poses=None).step(A)``: the step as it was before poses could be learned (that code path is unchanged)
        fused     ``AvatarTrainer(poses=PoseTable).step_frames(f)``: one launch each way
        composed  the same tables through the stand-alone wrappers: ``index_select`` on the device index, ``rotation_6d_to_axis_angle``
                  twice, ``joint_transforms_hip`` (what (c) of the issue asks for)
      medians over ``--reps`` blocks, the spread (min, max) of each, and the differences

Writes profiles/pose_time.json (``--out``)."""
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

from sings_amd import _lib, overflow                              # noqa: E402
from sings_amd import rotations as R                              # noqa: E402
from sings_amd._marshal import _ptr, _stream                      # noqa: E402
from sings_amd.body import joint_transforms, joint_transforms_hip  # noqa: E402
from sings_amd.decode import (AppearanceDecoder, GeometryDecoder, HexPlaneField, overlap_weight_grads,   # noqa: E402
                              prepare_triplane_backward_early, set_gradient_arena)
from sings_amd.pose import NB, PoseTable                          # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings   # noqa: E402
from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm     # noqa: E402
from sings_amd.scene import avatar_scene, body_tree              # noqa: E402
from sings_amd.train_loop import AvatarTrainer                   # noqa: E402
from sings_amd.train_step import AvatarStep                      # noqa: E402

LRS = {"xyz": 3.2e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}        # defaults/config.py:62-84
POSE_LRS = dict(LRS, global_orient=1e-4, body_pose=1e-4)                             # lr.smpl_pose


class ComposedPoses(torch.nn.Module):
    """``PoseTable``'s interface over the stand-alone wrappers: the path a user could build before ``sg_pose_transforms`` existed."""

    def __init__(self, table):
        super().__init__()
        self.global_orient = torch.nn.Parameter(table.global_orient.detach().clone())
        self.body_pose = torch.nn.Parameter(table.body_pose.detach().clone())
        self.transl, self.joints_rest, self.post, self.tail_pose = table.transl, table.joints_rest, table.post, table.tail_pose
        self.parents, self.NBu = tuple(int(p) for p in table.parents.cpu()), table.NBu

    def forward(self, idx):
        K = int(idx.shape[0])
        i = idx.long()
        go = R.rotation_6d_to_axis_angle(self.global_orient.index_select(0, i))
        bp = R.rotation_6d_to_axis_angle(self.body_pose.index_select(0, i).reshape(K, NB, 6)[:, :self.NBu].contiguous())
        aa = torch.cat([go[:, None], bp] + ([self.tail_pose[None].expand(K, -1, -1)] if self.tail_pose.numel() else []), 1)
        return joint_transforms_hip(aa.contiguous(), self.joints_rest, self.parents, post=self.post), self.transl.index_select(0, i)


def build(dev, N, poses_kind):
    """The bench's training workload (benchkit/leg_train.py) behind an AvatarTrainer; ``poses_kind``: None, "fused" or "composed"."""
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
    poses72 = np.load(os.path.join(ROOT, "tests", "golden", "lbs_golden.npz"))["amass_poses_72"].astype(np.float32)
    F = poses72.shape[0]
    poses72[:, :3] = 0
    poses = np.zeros((F, J * 3), np.float32); poses[:, :66] = poses72[:, :66]        # (the 52-joint layout drives 21 body joints)
    jr = t(s["joints_rest"])
    parents = tuple(int(p) for p in s["parents"])
    A_all = torch.stack([joint_transforms(t(poses[f]), jr, parents) for f in range(F)]).reshape(F, J, 4, 4).contiguous()
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
    table = None
    if poses_kind is not None:
        table = PoseTable.from_axis_angle(t(poses72[:, :3]), t(poses72[:, 3:]), t(np.tile(s["transl"].reshape(1, 3), (F, 1))), jr,
                                          parents=parents, body="smplh")
        if poses_kind == "composed":
            table = ComposedPoses(table)
    tr = AvatarTrainer(mod, settings, consts["bg"], POSE_LRS if table is not None else LRS, smpl_scale=t(s["smpl_scale"]),
                       transl=t(s["transl"]), use_graph=True, sh_degree=0, max_sh_degree=0, optimizer="fused", poses=table)
    return tr, A_all, gt, mask, F


def launches_alone(dev, K, J, reps):
    """-> (forward us, backward us) per launch: medians over ``reps`` groups of 32 launches between two events."""
    lib = _lib.load()
    F, nbu = 80, {24: 23, 52: 21}[J]
    g = torch.Generator(device="cpu").manual_seed(K * 100 + J)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    go, bp, transl = rnd(F, 6), rnd(F, NB * 6), rnd(F, 3)
    tail = torch.zeros(max(J - 1 - nbu, 0), 3, device=dev)
    rest, parents = body_tree(J)
    joints, par = torch.from_numpy(np.asarray(rest, np.float32)).to(dev), torch.tensor([int(p) for p in parents], dtype=torch.int32, device=dev)
    post = torch.eye(4, device=dev).repeat(J, 1, 1) + 0.01 * rnd(J, 4, 4)
    idx = (torch.arange(K, dtype=torch.int32) * 5 % F).to(dev)
    A, aa, rows = torch.empty(K, J, 16, device=dev), torch.empty(K, J, 3, device=dev), torch.empty(K, 3, device=dev)
    dA, d_rows = rnd(K, J, 16), rnd(K, 3)
    d_go, d_bp, d_t = torch.empty_like(go), torch.empty_like(bp), torch.empty_like(transl)
    st = _stream(dev)
    fwd = lambda: _lib.check(lib.sg_pose_transforms(K, F, J, nbu, _ptr(idx), _ptr(go), _ptr(bp), _ptr(tail), _ptr(transl), _ptr(joints), _ptr(par),
                                                    _ptr(post), _ptr(A), _ptr(aa), _ptr(rows), st), "pose transforms")
    bwd = lambda: _lib.check(lib.sg_pose_transforms_backward(K, F, J, nbu, _ptr(idx), _ptr(go), _ptr(bp), _ptr(aa), _ptr(joints), _ptr(par),
                                                             _ptr(post), _ptr(dA), _ptr(d_rows), _ptr(d_go), _ptr(d_bp), _ptr(d_t), st),
                             "pose transforms backward")
    out = []
    for fn in (fwd, bwd):
        ts = []
        for rep in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(32):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ts.append(e0.elapsed_time(e1) / 32 * 1e3)
        out.append(statistics.median(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--gaussians", type=int, default=150000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "pose_time.py needs the GPU"
    dev = torch.device("cuda:0")
    out = {"gaussians": a.gaussians, "reps": a.reps, "steps_per_block": a.steps, "device": torch.cuda.get_device_name(0)}

    # ---- (a) the two launches alone
    out["launch_us"] = {}
    for J in (24, 52):
        for K in (1, 16):
            f, b = launches_alone(dev, K, J, 20)
            out["launch_us"][f"J{J}_K{K}"] = {"forward": f, "backward": b}

    # ---- (b), (c) the captured step: each trainer is built, sized and captured in turn (one gradient arena is registered at a time; a
    # captured graph holds its own arena's addresses), then the three replay in alternating blocks
    overlap_weight_grads(True); prepare_triplane_backward_early(True)          # (the bench's defaults)
    trainers, steppers = {}, {}
    for name, kind in (("fixed", None), ("fused", "fused"), ("composed", "composed")):
        tr, A_all, gt, mask, F = build(dev, a.gaussians, kind)
        trainers[name] = tr
        steppers[name] = ((lambda i, tr=tr, A_all=A_all, gt=gt, mask=mask, F=F: tr.step(A_all[i % F], gt, mask)) if kind is None else
                          (lambda i, tr=tr, gt=gt, mask=mask, F=F: tr.step_frames(i % F, gt, mask)))
        for i in range(8):                                        # sizing steps, the capture, replays
            steppers[name](i)
        torch.cuda.synchronize()
        assert tr.captured is not None
    blocks = {k: [] for k in trainers}
    for rep in range(a.reps + 2):
        for name, step in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                step(rep * a.steps + i)
            torch.cuda.synchronize()
            if rep >= 2:
                blocks[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    for name, v in blocks.items():
        out[f"step_ms_{name}"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "blocks": v}
    overflow.check_deferred_overflow(dev)                         # (raises if a timed step overflowed the pair capacity)
    med = lambda k: out[f"step_ms_{k}"]["median"]
    out["added_ms_fused_over_fixed"] = med("fused") - med("fixed")
    out["added_ms_composed_over_fixed"] = med("composed") - med("fixed")
    out["fused_minus_composed_ms"] = med("fused") - med("composed")
    out["spread_ms"] = max(out[f"step_ms_{k}"]["max"] - out[f"step_ms_{k}"]["min"] for k in trainers)
    overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
    set_gradient_arena(None, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
