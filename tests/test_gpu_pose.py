"""sings_amd.pose.PoseTable (sg_pose_transforms[_backward], csrc/sg_pose.hip) on the GPU against tests/golden/pose_golden.npz: the
reference's own fp32 axis-angle and A for the kit's 80 frames, a copy pushed off the rotation manifold and exact-identity rows, and
its fp64 gradients of both tables for a seeded dA (tests/golden/gen_pose_golden.py; no row is excluded: the generator asserts that
the quaternion candidates are never within 1e-3 of a tie).

Bounds: A atol 3e-6 (tests/test_gpu_lbs.py's bound for this chain; the reference's fp32 against its fp64 is 6.5e-7), axis-angle
rtol = atol = 2e-6 (tests/test_gpu_rotations.py), gradients |a - b| <= 3e-5 |b| + 3e-6 max|b| (tests/test_gpu_lbs.py; the reference's
fp32 autograd sits at 0.11 of it)."""
import os

import numpy as np
import pytest
import torch

import pose_case as pc

pytestmark = pytest.mark.gpu
G = np.load(pc.GOLDEN)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _table(body, dev, rows=None, transl=None, learn_transl=False):
    from sings_amd.pose import PoseTable
    rows = G[f"{body}_rows"] if rows is None else rows
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tail = t(G[f"{body}_tail"]) if f"{body}_tail" in G.files else None
    tr = np.zeros((len(rows), 3), np.float32) if transl is None else transl
    return PoseTable(t(G["global_orient"][rows]), t(G["body_pose"][rows]), t(tr), t(G[f"{body}_joints"]), t(G[f"{body}_post"]),
                     tuple(int(p) for p in G[f"{body}_parents"]), body, tail, learn_transl=learn_transl)


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _grads(pt, idx, dA, d_rows=None):
    for p in pt.parameters():
        p.grad = None
    A, rows = pt(idx)
    loss = (A * dA).sum()
    if d_rows is not None:
        loss = loss + (rows * d_rows).sum()
    loss.backward()
    return A.detach(), [p.grad.clone() for p in (pt.global_orient, pt.body_pose)] + ([pt.transl.grad.clone()] if d_rows is not None else [])


@pytest.mark.parametrize("body", ["smpl", "smplh"])
def test_forward_against_the_reference(body):
    dev = _dev()
    pt = _table(body, dev)
    R, J = len(G[f"{body}_rows"]), pc.LAYOUT[body][0]
    idx = torch.arange(R, dtype=torch.int32, device=dev)
    with torch.no_grad():
        A, rows = pt(idx)
    A, aa = A.cpu().numpy(), pt.last_axis_angle.cpu().numpy()
    assert A.shape == (R, J, 4, 4) and aa.shape == (R, J, 3) and rows.shape == (R, 3)
    err_A, err_aa = np.abs(A[:, :, :3] - G[f"{body}_A34"]).max(), np.abs(aa - G[f"{body}_aa"]).max()
    print(f"{body}: max |A - reference| {err_A:.2e}, max |axis-angle - reference| {err_aa:.2e}")
    assert err_A <= 3e-6
    np.testing.assert_allclose(aa, G[f"{body}_aa"], rtol=2e-6, atol=2e-6)
    assert np.array_equal(A[:, :, 3], np.broadcast_to(G[f"{body}_post"][None, :, 3], (R, J, 4)))
    assert np.isfinite(A).all() and np.isfinite(aa).all()
    # the exact-identity rows: zero axis-angle in the learned joints
    assert np.array_equal(aa[-4:, :pc.LAYOUT[body][1] + 1], np.zeros((4, pc.LAYOUT[body][1] + 1, 3), np.float32))


@pytest.mark.parametrize("body", ["smpl", "smplh"])
def test_backward_against_the_fp64_reference(body):
    dev = _dev()
    pt = _table(body, dev)
    R, nbu = len(G[f"{body}_rows"]), pc.LAYOUT[body][1]
    dA = torch.from_numpy(pc.upstream(body, R)).to(dev)
    _, (dgo, dbp) = _grads(pt, torch.arange(R, dtype=torch.int32, device=dev), dA)
    worst = 0.0
    for name, a, b in (("global_orient", dgo, G[f"{body}_d_global_orient"]), ("body_pose", dbp, G[f"{body}_d_body_pose"])):
        a, b = a.cpu().numpy().astype(np.float64), b.astype(np.float64)
        assert np.isfinite(a).all(), name
        ratio = np.abs(a - b) / (3e-5 * np.abs(b) + 3e-6 * np.abs(b).max())
        worst = max(worst, float(ratio.max()))
        print(f"{body} d_{name}: worst entry at {ratio.max():.3f} of the bound (row {np.unravel_index(ratio.argmax(), ratio.shape)[0]})")
        assert (ratio <= 1.0).all(), (name, float(ratio.max()))
    # body joints the layout does not drive (SMPL-H: 22 and 23 of the row) are exactly zero
    unused = dbp.reshape(R, pc.NB, 6)[:, nbu:]
    assert unused.numel() == R * (pc.NB - nbu) * 6 and not unused.any()
    # rows the step does not name are exactly zero, the named ones are what the full call gave
    some = torch.tensor([3, 40, R - 1], dtype=torch.int32, device=dev)
    _, (dgo_s, dbp_s) = _grads(pt, some, dA[some.long()])
    named = torch.zeros(R, dtype=torch.bool, device=dev); named[some.long()] = True
    assert not dgo_s[~named].any() and not dbp_s[~named].any()
    assert _bits_equal(dgo_s[named], dgo[named]) and _bits_equal(dbp_s[named], dbp[named])


def test_identity_rows_have_the_references_finite_gradient():
    """d aa.sum() / d d6 at (1,0,0,0,1,0) is (0,-1,1,0,0,-1) in the reference (the selected candidate's gradient through the series
    branch of quaternion_to_axis_angle).  Through the kernel: Rodrigues' derivative at 0 is the three generator matrices (times
    sin(t)/t at t = |1e-8|, 1 in fp32), so a dA of (R32 - R23 + R13 - R31 + R21 - R12) / 2 on a LEAF joint of a chain with zero
    rest joints and no `post` hands that joint's axis-angle the gradient (1,1,1)."""
    from sings_amd.pose import PoseTable
    dev = _dev()
    ident = torch.from_numpy(pc.IDENTITY_6D).to(dev)
    pt = PoseTable(ident[None].clone(), ident.repeat(1, pc.NB), torch.zeros(1, 3, device=dev), torch.zeros(24, 3, device=dev))
    A, _ = pt(0)
    assert torch.equal(pt.last_axis_angle, torch.zeros(1, 24, 3, device=dev))
    assert torch.equal(A, torch.eye(4, device=dev).expand(24, 4, 4))
    leaf = 23                                                            # (SMPL_PARENTS: nobody's parent)
    dA = torch.zeros(4, 4, device=dev)
    dA[2, 1], dA[1, 2], dA[0, 2], dA[2, 0], dA[1, 0], dA[0, 1] = 0.5, -0.5, 0.5, -0.5, 0.5, -0.5
    (A[leaf] * dA).sum().backward()
    assert torch.isfinite(pt.global_orient.grad).all() and torch.isfinite(pt.body_pose.grad).all()
    g = pt.body_pose.grad.reshape(pc.NB, 6)[leaf - 1].cpu().numpy()
    np.testing.assert_allclose(g, G["identity_daa_dd6"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("body", ["smpl", "smplh"])
def test_k_frames_equal_single_calls_bit_for_bit(body):
    dev = _dev()
    rs = np.random.RandomState(5)
    R = len(G[f"{body}_rows"])
    transl = rs.normal(0, 1, (R, 3)).astype(np.float32)
    pt = _table(body, dev, transl=transl, learn_transl=True)
    J = pc.LAYOUT[body][0]
    frames = [7, 2, 41, 80, R - 1, 0]
    K = len(frames)
    dA = torch.from_numpy(rs.normal(0, 1, (K, J, 4, 4)).astype(np.float32)).to(dev)
    d_rows = torch.from_numpy(rs.normal(0, 1, (K, 3)).astype(np.float32)).to(dev)
    idx = torch.tensor(frames, dtype=torch.int32, device=dev)
    A, gk = _grads(pt, idx, dA, d_rows)
    with torch.no_grad():
        _, rows = pt(idx)
    assert _bits_equal(rows, torch.from_numpy(transl[frames]).to(dev))
    singles = []
    for k, f in enumerate(frames):
        for p in pt.parameters():
            p.grad = None
        A1, row1 = pt(f)                                                 # an int: [J,4,4], [3]
        assert A1.shape == (J, 4, 4) and row1.shape == (3,)
        ((A1 * dA[k]).sum() + (row1 * d_rows[k]).sum()).backward()
        assert _bits_equal(A1.detach(), A[k]), f"frame {f}"
        singles.append([p.grad.clone() for p in (pt.global_orient, pt.body_pose, pt.transl)])
    for n in range(3):                                                   # distinct rows: the K-frame gradient is the single calls', row by row
        want = torch.zeros_like(gk[n])
        for k, f in enumerate(frames):
            assert not singles[k][n][torch.arange(R, device=dev) != f].any()
            want[f] = singles[k][n][f]
        assert _bits_equal(gk[n], want), ("global_orient", "body_pose", "transl")[n]
    # a row named twice: exactly the sum of the two single-call gradients, first position first
    dup = torch.tensor([frames[0], frames[1], frames[0]], dtype=torch.int32, device=dev)
    _, gd = _grads(pt, dup, dA[[0, 1, 2]], d_rows[[0, 1, 2]])
    for p in pt.parameters():
        p.grad = None
    A1, row1 = pt(frames[0])
    ((A1 * dA[2]).sum() + (row1 * d_rows[2]).sum()).backward()
    second = [p.grad.clone() for p in (pt.global_orient, pt.body_pose, pt.transl)]
    for n in range(3):
        want = torch.zeros_like(gd[n])
        want[frames[0]] = singles[0][n][frames[0]] + second[n][frames[0]]
        want[frames[1]] = singles[1][n][frames[1]]
        assert _bits_equal(gd[n], want), n
    # two runs: bitwise identical
    _, gd2 = _grads(pt, dup, dA[[0, 1, 2]], d_rows[[0, 1, 2]])
    A2, gk2 = _grads(pt, idx, dA, d_rows)
    assert _bits_equal(A2, A) and all(_bits_equal(a, b) for a, b in zip(gd + gk, gd2 + gk2))


@pytest.mark.parametrize("body", ["smpl", "smplh"])
def test_one_launch_equals_the_existing_pieces_bit_for_bit(body):
    """Against ``joint_transforms_hip(rotation_6d_to_axis_angle(row), joints_rest, post=...)`` composed from the stand-alone wrappers
    (four conversion launches and the chain, each way): the kernel calls the same device functions in the same order and the build
    forbids contraction, so values and gradients are bit-equal."""
    from sings_amd import rotations as Rt
    from sings_amd.body import joint_transforms_hip
    dev = _dev()
    pt = _table(body, dev)
    R, (J, nbu) = len(G[f"{body}_rows"]), pc.LAYOUT[body]
    dA = torch.from_numpy(pc.upstream(body, R)).to(dev)
    A, (dgo, dbp) = _grads(pt, torch.arange(R, dtype=torch.int32, device=dev), dA)
    go = pt.global_orient.detach().clone().requires_grad_(True)
    bp = pt.body_pose.detach().clone().requires_grad_(True)
    d6 = torch.cat([go.reshape(R, 1, 6), bp.reshape(R, pc.NB, 6)[:, :nbu]], 1)
    aa = Rt.rotation_6d_to_axis_angle(d6)
    if J - 1 - nbu:
        aa = torch.cat([aa, pt.tail_pose[None].expand(R, -1, -1)], 1)
    A_ref = joint_transforms_hip(aa.contiguous(), pt.joints_rest, tuple(int(p) for p in pt.parents.cpu()), post=pt.post)
    (A_ref * dA).sum().backward()
    assert _bits_equal(pt.last_axis_angle, aa.detach().contiguous())
    assert _bits_equal(A, A_ref.detach())
    assert _bits_equal(dgo, go.grad) and _bits_equal(dbp, bp.grad)


def test_frame_index_checks_and_clamp():
    dev = _dev()
    pt = _table("smpl", dev)
    R = len(G["smpl_rows"])
    with pytest.raises(IndexError):
        pt(R)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pt(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        pt(torch.zeros(2, dtype=torch.int64, device=dev))
    with torch.no_grad():                                                # a device index outside the table reads the nearest row
        A, _ = pt(torch.tensor([-5, R + 9], dtype=torch.int32, device=dev))
        B, _ = pt(torch.tensor([0, R - 1], dtype=torch.int32, device=dev))
    assert _bits_equal(A, B)


def test_save_kit_poses_round_trip(tmp_path):
    """Keys, shapes and dtypes of the kit's poses_optimized.npz; loading the file and converting again reproduces A within the forward
    test's bound (3e-6)."""
    from sings_amd.pose import PoseTable
    dev = _dev()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kit = {k: G["kit_" + k] for k in ("global_orient", "body_pose", "transl", "betas")}
    args = (t(G["smpl_joints"]), torch.inverse(t(G["smpl_post"])), tuple(int(p) for p in G["smpl_parents"]))
    pt = PoseTable.from_axis_angle(t(kit["global_orient"]), t(kit["body_pose"]), t(kit["transl"]), *args)
    with torch.no_grad():                                                # what a few Adam steps leave: rows off the manifold
        pt.global_orient.add_(0.02 * torch.randn_like(pt.global_orient)); pt.body_pose.add_(0.02 * torch.randn_like(pt.body_pose))
    path = str(tmp_path / "poses_refined.npz")
    pt.save_kit_poses(path, betas=kit["betas"])
    z = np.load(path)
    assert sorted(z.files) == sorted(kit)
    for k, v in kit.items():
        assert z[k].shape == v.shape and z[k].dtype == v.dtype, k
    assert np.array_equal(z["betas"], kit["betas"]) and np.array_equal(z["transl"], kit["transl"])
    for a, b in zip(pt.axis_angle(), (z["global_orient"], z["body_pose"], z["transl"])):
        assert np.array_equal(a, b)
    again = PoseTable.from_axis_angle(t(z["global_orient"]), t(z["body_pose"]), t(z["transl"]), *args)
    idx = torch.arange(80, dtype=torch.int32, device=dev)
    with torch.no_grad():
        A0, r0 = pt(idx)
        A1, r1 = again(idx)
    err = float((A0 - A1).abs().max())
    print(f"save_kit_poses round trip: max |A - A'| {err:.2e}")
    assert err <= 3e-6 and _bits_equal(r0, r1)
