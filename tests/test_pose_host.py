"""Host side of the learned-pose path (no GPU): the two entry points are in the prototype table under ABI 8, ``PoseTable`` validates its
inputs and refuses host tensors, ``AvatarTrainer`` refuses pose groups without a table, and the CPU restatement the GPU tests compare
against (tests/pose_case.py, over the oracle helpers) reproduces the reference's golden values and fp64 gradients."""
import numpy as np
import pytest
import torch

import pose_case as pc


def test_entry_points_are_declared_under_abi_8():
    from sings_amd import _lib
    assert _lib.ABI_VERSION == 8
    assert _lib._PROTOTYPES["sg_pose_transforms"] == "i: i4 p12"
    assert _lib._PROTOTYPES["sg_pose_transforms_backward"] == "i: i4 p13"
    lib = _lib.load()
    assert lib.sg_abi_version() == 8 and _lib.POSE_NB == pc.NB
    # bad arguments are refused before anything is launched or dereferenced
    import ctypes as C
    fake = C.c_void_p(0x1000)
    for K, F, J, nbu in ((0, 8, 24, 23), (1, 0, 24, 23), (1, 8, 65, 23), (1, 8, 24, 24), (1, 8, 23, 23)):
        rc = lib.sg_pose_transforms(K, F, J, nbu, fake, fake, fake, None, None, fake, fake, None, fake, fake, None, None)
        assert rc != 0 and b"sg_pose_transforms: bad argument" in lib.sg_last_error()
    assert lib.sg_pose_transforms(1, 8, 52, 21, fake, fake, fake, None, None, fake, fake, None, fake, fake, None, None) != 0      # no tail
    assert lib.sg_pose_transforms(1, 8, 24, 23, fake, fake, fake, None, fake, fake, fake, None, fake, fake, None, None) != 0      # transl alone
    assert lib.sg_pose_transforms_backward(1, 8, 24, 23, fake, fake, fake, fake, fake, fake, None, fake, fake, fake, fake, None, None) != 0


def _inputs(F=5, J=24):
    rs = np.random.RandomState(0)
    f = lambda *s: torch.from_numpy(rs.normal(0, 0.2, s).astype(np.float32))
    return dict(global_orient=f(F, 3), body_pose=f(F, 69), transl=f(F, 3), joints_rest=f(J, 3), A_t2cano=torch.eye(4).repeat(J, 1, 1))


def test_from_axis_angle_validates_shapes():
    from sings_amd.pose import PoseTable
    ok = _inputs()
    with pytest.raises(ValueError, match="body_pose"):
        PoseTable.from_axis_angle(**dict(ok, body_pose=torch.zeros(4, 69)))                       # F mismatch
    with pytest.raises(ValueError, match="transl"):
        PoseTable.from_axis_angle(**dict(ok, transl=torch.zeros(6, 3)))
    with pytest.raises(ValueError, match="'smpl' or 'smplh'"):
        PoseTable.from_axis_angle(**ok, body="smplx")
    with pytest.raises(ValueError, match="joints_rest"):
        PoseTable.from_axis_angle(**ok, body="smplh")                                             # 24 joints for the 52-joint layout
    h = _inputs(J=52)
    parents52 = (-1,) + tuple(range(51))
    with pytest.raises(ValueError, match="tail_pose must have 30 rows"):
        PoseTable.from_axis_angle(**h, parents=parents52, body="smplh", tail_pose=torch.zeros(29, 3))
    with pytest.raises(ValueError, match="tail_pose must have 0 rows"):
        PoseTable.from_axis_angle(**ok, tail_pose=torch.zeros(30, 3))
    with pytest.raises(ValueError, match="topological order"):
        PoseTable.from_axis_angle(**ok, parents=(-1, 0, 3, 1) + tuple(range(3, 23)))
    with pytest.raises(ValueError, match="parents must have 24 entries"):
        PoseTable.from_axis_angle(**ok, parents=parents52)


def test_host_tensors_are_refused():
    from sings_amd.pose import PoseTable
    ok = _inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PoseTable.from_axis_angle(**ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PoseTable(torch.zeros(5, 6), torch.zeros(5, 138), ok["transl"], ok["joints_rest"])
    with pytest.raises(ValueError, match=r"body_pose must be \[F,138\]"):
        PoseTable(torch.zeros(5, 6), torch.zeros(5, 69), ok["transl"], ok["joints_rest"])


def test_trainer_rejects_pose_groups_without_a_table():
    from sings_amd.train_loop import AvatarTrainer
    lrs = {"xyz": 1e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}
    for name in AvatarTrainer.POSE_GROUPS:
        with pytest.raises(ValueError, match="lrs for pose groups"):
            AvatarTrainer(None, None, None, dict(lrs, **{name: 1e-4}))
        with pytest.raises(ValueError, match="lr_schedules for pose groups"):
            AvatarTrainer(None, None, None, lrs, lr_schedules={name: lambda it: 1e-4})


@pytest.mark.parametrize("body", ["smpl", "smplh"])
def test_cpu_restatement_reproduces_the_golden(body):
    """tests/pose_case.py in fp32 against the reference's fp32 values (the GPU tests' bounds), in fp64 against its fp64 gradients."""
    G = np.load(pc.GOLDEN)
    rows = G[f"{body}_rows"]
    go, bp = G["global_orient"][rows], G["body_pose"][rows]
    tail = G[f"{body}_tail"] if f"{body}_tail" in G.files else None
    T = lambda a: None if a is None else torch.from_numpy(a)
    A, aa = pc.pose_to_A(T(go), T(bp), T(G[f"{body}_joints"]), G[f"{body}_parents"], T(G[f"{body}_post"]), body, T(tail))
    np.testing.assert_allclose(aa.numpy(), G[f"{body}_aa"], rtol=2e-6, atol=2e-6)
    assert np.abs(A.numpy()[:, :, :3] - G[f"{body}_A34"]).max() <= 3e-6
    dgo, dbp = pc.table_gradients(go, bp, pc.upstream(body, len(rows)), G[f"{body}_joints"], G[f"{body}_parents"], G[f"{body}_post"], body,
                                  tail)
    for a, b in ((dgo, G[f"{body}_d_global_orient"]), (dbp, G[f"{body}_d_body_pose"])):
        b = b.astype(np.float64)
        assert (np.abs(a - b) <= 3e-5 * np.abs(b) + 3e-6 * np.abs(b).max()).all()
    assert G["candidate_min_gap"] >= 1e-3 and (G["candidate_counts"] > 0).sum() >= 3
    np.testing.assert_array_equal(G["identity_daa_dd6"], np.array([0, -1, 1, 0, 0, -1], np.float32))
