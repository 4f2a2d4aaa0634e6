"""The learned-pose path (sings_amd/pose.py, sg_pose_transforms) restated on the CPU with torch autograd over the oracle helpers, generic
in dtype, and what its tests share: the layouts, the golden file's keys, the seeded upstream gradient.

    row of the 6-D tables -> rotation_6d_to_axis_angle per joint (oracle/rotations_oracle.py)
                          -> batch_rodrigues, batch_rigid_transform (oracle/lbs_oracle.py) -> A = G - pad(G J) -> @ post
"""
import os

import numpy as np
import torch

from oracle import lbs_oracle as lo
from oracle import rotations_oracle as rot

NB = 23
LAYOUT = {"smpl": (24, 23), "smplh": (52, 21)}              # body -> (J, body joints of the row the chain uses)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_golden.npz")
IDENTITY_6D = np.array([1, 0, 0, 0, 1, 0], np.float32)
DA_SEED = {"smpl": 4101, "smplh": 4102}


def upstream(body, rows):
    """The seeded dL/dA [rows,J,4,4] of the golden gradients (regenerated, not stored: numpy's RandomState is stable)."""
    J = LAYOUT[body][0]
    return np.random.RandomState(DA_SEED[body]).normal(0, 1, (rows, J, 4, 4)).astype(np.float32)


def axis_angle_rows(global_orient, body_pose, body="smpl", tail_pose=None):
    """Tables' rows [R,6], [R,138] -> the chain's axis-angle pose [R,J,3] (the row's first NBu body joints, then the constant tail)."""
    J, nbu = LAYOUT[body]
    R = global_orient.shape[0]
    d6 = torch.cat([global_orient.reshape(R, 1, 6), body_pose.reshape(R, NB, 6)[:, :nbu]], 1)
    aa = rot.rotation_6d_to_axis_angle(d6)
    if J - 1 - nbu:
        tail = torch.zeros(J - 1 - nbu, 3, dtype=aa.dtype) if tail_pose is None else tail_pose.to(aa.dtype)
        aa = torch.cat([aa, tail[None].expand(R, -1, -1)], 1)
    return aa


def pose_to_A(global_orient, body_pose, joints_rest, parents, post=None, body="smpl", tail_pose=None):
    """-> (A [R,J,4,4], axis-angle [R,J,3]); differentiable w.r.t. the two tables, in the dtype of the inputs."""
    J = LAYOUT[body][0]
    R = global_orient.shape[0]
    aa = axis_angle_rows(global_orient, body_pose, body, tail_pose)
    rm = lo.batch_rodrigues(aa.reshape(-1, 3)).reshape(R, J, 3, 3)
    _, A = lo.batch_rigid_transform(rm, joints_rest[None].expand(R, -1, -1).contiguous(), [int(p) for p in parents])
    if post is not None:
        A = A @ post[None]
    return A, aa


def table_gradients(global_orient, body_pose, dA, joints_rest, parents, post=None, body="smpl", tail_pose=None, dtype=torch.float64):
    """d sum(A * dA) / d (global_orient, body_pose), every row on its own, evaluated in ``dtype``; numpy in, numpy (``dtype``) out."""
    T = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)
    go, bp = T(global_orient).requires_grad_(True), T(body_pose).requires_grad_(True)
    A, _ = pose_to_A(go, bp, T(joints_rest), parents, T(post), body, T(tail_pose))
    (A * T(dA)).sum().backward()
    return go.grad.numpy(), bp.grad.numpy()
