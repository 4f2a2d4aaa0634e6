"""Generates tests/golden/pose_golden.npz by IMPORTING the reference's own Python (read-only at /root/reference) in the build
container, the way gen_lbs_golden.py does.  The reference source never ships; only these vectors do.

    python tests/golden/gen_pose_golden.py

Inputs    the 80 frames of examples/training_kits/f_2/score_demo_video/poses_optimized.npz, converted with the reference's
          axis_angle_to_rotation_6d (create_global_orient / create_body_pose); a copy pushed off the manifold by + 0.02 N(0,1) (what
          the rows look like after Adam steps); four rows that are exactly the identity (1,0,0,0,1,0) in every joint; rest joints of
          oracle.lbs_oracle.synthetic_body_model for J = 24 and a 52-joint tree, a random rigid `post` per joint; 30 constant tail
          rows for the 52-joint layout.  The 24-joint layout sees all 164 rows, the 52-joint one every second kit / perturbed row and
          the identity rows (84): the file stays well under 1 MB.
Outputs   the reference's fp32 axis-angle (rotation_6d_to_axis_angle) and A (vendored batch_rodrigues + batch_rigid_transform, @ post;
          its constant bottom row is not stored), and for the seeded dA of tests/pose_case.py the gradient of sum(A * dA) w.r.t. both
          tables from the same reference functions evaluated in fp64 (stored rounded to fp32: 6e-8 relative).
Asserted  in every row the two largest candidate magnitudes of matrix_to_quaternion differ by >= 1e-3 relative, so no test excludes a
          row (on failure: another perturbation seed, never an exclusion).
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sings.rec.utils.geometry import rotations as rot            # noqa: E402  (torch only)
from sings.rec.utils.body_model import smpl as vsmpl             # noqa: E402  (vendored SMPL math)

import pose_case as pc                                           # noqa: E402  (layouts, the seeded dA)
from oracle.lbs_oracle import synthetic_body_model               # noqa: E402  (inputs only)

PERTURB_SEED = 20
NB = pc.NB
out = {}
T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)

kit = np.load(os.path.join(REF, "examples/training_kits/f_2/score_demo_video/poses_optimized.npz"))
F = kit["global_orient"].shape[0]
assert F == 80 and kit["body_pose"].shape == (F, NB * 3)
go6 = rot.axis_angle_to_rotation_6d(T(kit["global_orient"])).numpy()
bp6 = rot.axis_angle_to_rotation_6d(T(kit["body_pose"]).reshape(F, NB, 3)).reshape(F, NB * 6).numpy()
rs = np.random.RandomState(PERTURB_SEED)
go6p = (go6 + 0.02 * rs.normal(0, 1, go6.shape)).astype(np.float32)
bp6p = (bp6 + 0.02 * rs.normal(0, 1, bp6.shape)).astype(np.float32)
n_id = 4
go_all = np.concatenate([go6, go6p, np.tile(pc.IDENTITY_6D, (n_id, 1))]).astype(np.float32)
bp_all = np.concatenate([bp6, bp6p, np.tile(pc.IDENTITY_6D, (n_id, NB))]).astype(np.float32)
out["global_orient"], out["body_pose"] = go_all, bp_all
out["kit_global_orient"], out["kit_body_pose"], out["kit_transl"], out["kit_betas"] = (
    kit["global_orient"], kit["body_pose"], kit["transl"], kit["betas"])

# ---- which quaternion candidate each row selects, and by what margin
d6 = np.concatenate([go_all[:2 * F].reshape(-1, 1, 6), bp_all[:2 * F].reshape(-1, NB, 6)], 1).reshape(-1, 6)
m = rot.rotation_6d_to_matrix(T(d6, torch.float64))
m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
q_abs = torch.sqrt(torch.clamp(torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1), min=0))
top = torch.sort(q_abs, -1, descending=True).values
gap = ((top[:, 0] - top[:, 1]) / top[:, 0]).min().item()
counts = np.bincount(q_abs.argmax(-1).numpy(), minlength=4)
print(f"candidates selected over {d6.shape[0] // 2} kit + {d6.shape[0] // 2} perturbed joints: {counts.tolist()}; smallest relative gap "
      f"between the two largest: {gap:.2e}")
assert gap >= 1e-3, "two candidates within 1e-3: choose another PERTURB_SEED (do not exclude rows)"
out["candidate_counts"], out["candidate_min_gap"] = counts.astype(np.int64), np.float64(gap)

# ---- d aa.sum() / d d6 at the exact identity (finite: (0,-1,1,0,0,-1))
x = T(pc.IDENTITY_6D[None]).requires_grad_(True)
rot.rotation_6d_to_axis_angle(x).sum().backward()
out["identity_daa_dd6"] = x.grad.numpy()[0]
assert np.isfinite(out["identity_daa_dd6"]).all()


def reference_A(go, bp, joints, parents, post, body, tail, dtype):
    J, nbu = pc.LAYOUT[body]
    R = go.shape[0]
    aa_go = rot.rotation_6d_to_axis_angle(go.reshape(-1, 6)).reshape(R, 3)
    aa_bp = rot.rotation_6d_to_axis_angle(bp.reshape(-1, 6)).reshape(R, NB * 3)[:, :nbu * 3]          # SMPL-H: body_pose[:63]
    full = torch.cat([aa_go, aa_bp] + ([tail.reshape(1, -1).expand(R, -1)] if tail is not None else []), 1)
    rm = vsmpl.batch_rodrigues(full.reshape(-1, 3), dtype=dtype).view(R, J, 3, 3)
    _, A = vsmpl.batch_rigid_transform(rm, joints[None].expand(R, -1, -1), parents, dtype=dtype)
    return A @ post[None], full.reshape(R, J, 3)


for body in ("smpl", "smplh"):
    J, nbu = pc.LAYOUT[body]
    bm = synthetic_body_model(seed=3 if body == "smpl" else 4, J=J)
    joints = (bm["J_regressor"] @ bm["v_template"]).astype(np.float32)
    parents = torch.from_numpy(bm["parents"])
    rsb = np.random.RandomState(77 + J)
    post = np.tile(np.eye(4, dtype=np.float32), (J, 1, 1))
    post[:, :3, :3] = vsmpl.batch_rodrigues(T(rsb.normal(0, 0.5, (J, 3)))).numpy()
    post[:, :3, 3] = rsb.normal(0, 0.1, (J, 3))
    tail = rsb.normal(0, 0.1, (J - 1 - nbu, 3)).astype(np.float32) if J - 1 - nbu else None
    rows = np.arange(go_all.shape[0]) if body == "smpl" else np.concatenate(
        [np.arange(0, F, 2), np.arange(F, 2 * F, 2), np.arange(2 * F, 2 * F + n_id)])
    go, bp = go_all[rows], bp_all[rows]
    with torch.no_grad():
        A32, aa32 = reference_A(T(go), T(bp), T(joints), parents, T(post), body, None if tail is None else T(tail), torch.float32)
    assert torch.equal(A32[:, :, 3], T(post)[None, :, 3].expand(len(rows), -1, -1)), "bottom row of A is post's"
    dA = pc.upstream(body, len(rows))
    g64, b64 = T(go, torch.float64).requires_grad_(True), T(bp, torch.float64).requires_grad_(True)
    D = torch.float64
    A64, _ = reference_A(g64, b64, T(joints, D), parents, T(post, D), body, None if tail is None else T(tail, D), D)
    (A64 * T(dA, D)).sum().backward()
    assert torch.isfinite(g64.grad).all() and torch.isfinite(b64.grad).all()
    # the reference's own fp32 against its fp64: the scale of the tests' bounds
    err_A = (A32.double() - A64.detach()).abs().max().item()
    g32, b32 = T(go).requires_grad_(True), T(bp).requires_grad_(True)
    A32g, _ = reference_A(g32, b32, T(joints), parents, T(post), body, None if tail is None else T(tail), torch.float32)
    (A32g * T(dA)).sum().backward()
    ratio = 0.0
    for a, b in ((g32.grad, g64.grad), (b32.grad, b64.grad)):
        ratio = max(ratio, ((a.double() - b).abs() / (3e-5 * b.abs() + 3e-6 * b.abs().max())).max().item())
    print(f"{body}: {len(rows)} rows; reference fp32 vs fp64: A {err_A:.2e}, table gradients at {ratio:.2f} of the tests' bound")
    out[f"{body}_rows"] = rows.astype(np.int64)
    out[f"{body}_joints"], out[f"{body}_parents"], out[f"{body}_post"] = joints, bm["parents"].astype(np.int32), post
    if tail is not None:
        out[f"{body}_tail"] = tail
    out[f"{body}_aa"] = aa32.numpy()
    out[f"{body}_A34"] = A32[:, :, :3].numpy().copy()
    out[f"{body}_d_global_orient"] = g64.grad.numpy().astype(np.float32)
    out[f"{body}_d_body_pose"] = b64.grad.numpy().astype(np.float32)

path = os.path.join(ROOT, "tests", "golden", "pose_golden.npz")
np.savez_compressed(path, **out)
print(f"wrote {path}: {os.path.getsize(path)} bytes")
