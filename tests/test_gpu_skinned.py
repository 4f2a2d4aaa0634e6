"""GPU parity of the LBS-fused path (sg_skinned_forward/backward through the C ABI).

Oracle = oracle/lbs_oracle.py (pinned against the reference's lbs_extra / matrix_to_quaternion /
quaternion_multiply by tests/golden/lbs_golden.npz) composed with the rasterizer oracle.
 * posed means / quaternions / scales vs the torch restatement: fp32 tolerance (W.A is summed in joint
   order on the matrix cores, torch uses a BLAS order);
 * the fused image must be BIT-IDENTICAL to the plain HIP path fed with the fused kernel's own posed
   outputs (same projection code, nothing else may differ);
 * LBS^T: gradients w.r.t. canonical means / rotations / scales, the joint transforms A and transl
   vs torch autograd through the restatement, seeded with the rasterizer-oracle gradients.
"""
import numpy as np
import pytest
import torch

from oracle import lbs_oracle as lo
from oracle import raster_oracle as ro
from sings_amd.camera import make_camera

pytestmark = pytest.mark.gpu
BORDER = 2e-5


def _scene(N, J, seed, isotropic=False):
    rs = np.random.RandomState(seed)
    xyz = (rs.normal(0, 0.35, (N, 3)) * np.array([0.5, 1.0, 0.3])).astype(np.float32)
    A = np.tile(np.eye(4, dtype=np.float32), (J, 1, 1))
    for j in range(J):
        A[j, :3, :3] = lo.batch_rodrigues(torch.from_numpy(rs.normal(0, 0.3, (1, 3)).astype(np.float32))).numpy()[0]
        A[j, :3, 3] = rs.normal(0, 0.05, 3)
    w = rs.rand(N, J).astype(np.float32) ** 6
    w[w < 0.1] = 0
    w[np.arange(N), rs.randint(0, J, N)] += 0.3
    w /= w.sum(1, keepdims=True)
    Rc = None if isotropic else lo.rotation_6d_to_matrix(torch.from_numpy(rs.normal(size=(N, 6)).astype(np.float32))).numpy()
    scales = np.exp(rs.normal(-4.6, 0.4, (N, 3))).astype(np.float32)
    if isotropic:
        scales[:] = scales[:, :1]
    opac = rs.uniform(0.05, 0.95, (N, 1)).astype(np.float32)
    shs = np.concatenate([rs.normal(0, 1, (N, 1, 3)), rs.normal(0, 0.15, (N, 15, 3))], 1).astype(np.float32)
    cam = make_camera(np.eye(4, dtype=np.float32), 1500.0, 1500.0, 128, 112, 256, 224)
    return dict(N=N, J=J, xyz=xyz, A=A, w=w.astype(np.float32), Rc=Rc, scales=scales, opac=opac, shs=shs, cam=cam,
                smpl_scale=np.array([1.07], np.float32), transl=np.array([-0.04, 0.09, 4.0], np.float32),
                bg=np.array([1, 1, 1], np.float32), dL=rs.normal(0, 1, (3, 224, 256)).astype(np.float32))


def _settings(s, dev, deg=3):
    import math
    from sings_amd.rasterizer import GaussianRasterizationSettings
    c = s["cam"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return GaussianRasterizationSettings(
        image_height=c["image_height"], image_width=c["image_width"], tanfovx=math.tan(c["fovx"] * 0.5),
        tanfovy=math.tan(c["fovy"] * 0.5), bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(c["world_view_transform"]),
        projmatrix=t(c["full_proj_transform"]), sh_degree=deg, campos=t(c["camera_center"]), prefiltered=False,
        debug=False)


def _oracle_deform(s, ext=None, grad=False):
    T = lambda a: None if a is None else torch.from_numpy(a).clone().requires_grad_(grad)
    xyz, Rc, sc, A, tr = T(s["xyz"]), T(s["Rc"]), T(s["scales"]), T(s["A"]), T(s["transl"])
    Rc_use = Rc if Rc is not None else torch.eye(3)[None].repeat(s["N"], 1, 1)
    out = lo.deform_gaussians(xyz, Rc_use, sc, torch.from_numpy(s["w"]), A, smpl_scale=torch.from_numpy(s["smpl_scale"]),
                              transl=tr, ext_tfs=ext)
    return (xyz, Rc, sc, A, tr), out


@pytest.mark.parametrize("J,iso,seed", [(24, False, 1), (52, False, 2), (52, True, 3), (30, False, 4)])
def test_fused_forward(J, iso, seed):
    from sings_amd.skinned import rasterize_skinned_gaussians
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    s = _scene(6000, J, seed, isotropic=iso)
    rs = _settings(s, dev)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    color, radii, pxyz, pq, psc = rasterize_skinned_gaussians(
        t(s["xyz"]), t(s["Rc"]), t(s["scales"]), t(s["opac"]), t(s["shs"]), t(s["w"]), t(s["A"]), rs,
        smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), return_posed=True)
    _, (oxyz, oq, osc, _) = _oracle_deform(s)
    assert np.abs(pxyz.cpu().numpy() - oxyz.numpy()).max() < 2e-5          # |xyz| ~ 4 -> ~5 ulp
    assert np.abs(psc.cpu().numpy() - osc.numpy()).max() < 1e-8
    assert np.abs(pq.cpu().numpy() - oq.numpy()).max() < 2e-5
    assert int((radii > 0).sum()) > 0.5 * s["N"]
    # fused == plain path on the fused kernel's own posed outputs, bit for bit
    c2, r2 = GaussianRasterizer(rs)(means3D=pxyz, means2D=torch.zeros_like(pxyz), opacities=t(s["opac"]), shs=t(s["shs"]),
                                    scales=psc, rotations=pq)
    assert torch.equal(radii, r2) and torch.equal(color, c2)
    # and the image matches the rasterizer oracle on those posed values
    cam = s["cam"]
    import math
    o = ro.forward(pxyz.cpu().numpy(), s["opac"], cam["world_view_transform"], cam["full_proj_transform"],
                   cam["camera_center"], 256, 224, math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"],
                   scales=psc.cpu().numpy(), rotations=pq.cpu().numpy(), shs=s["shs"], sh_degree=3)
    assert np.array_equal(o["radii"], radii.cpu().numpy())
    strict = o["margin"] >= BORDER
    assert np.abs(color.cpu().numpy() - o["color"]).max(0)[strict].max() <= 1e-5


def test_fused_forward_ext_tfs():
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = torch.device("cuda:0")
    s = _scene(3000, 24, 7)
    rs = _settings(s, dev)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    ext = (torch.tensor([0.05, -0.1, 0.5]), lo.batch_rodrigues(torch.tensor([[0.2, 0.6, -0.3]]))[0], torch.tensor([1.2]))
    with torch.no_grad():
        color, radii, pxyz, pq, psc = rasterize_skinned_gaussians(
            t(s["xyz"]), t(s["Rc"]), t(s["scales"]), t(s["opac"]), t(s["shs"]), t(s["w"]), t(s["A"]), rs,
            smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), ext_tfs=tuple(x.to(dev) for x in ext), return_posed=True)
    _, (oxyz, oq, osc, _) = _oracle_deform(s, ext=ext)
    assert np.abs(pxyz.cpu().numpy() - oxyz.numpy()).max() < 3e-5
    assert np.abs(pq.cpu().numpy() - oq.numpy()).max() < 3e-5
    assert np.abs(psc.cpu().numpy() - osc.numpy()).max() < 1e-8
    assert (pq[:, 0] >= 0).all()              # quaternion_multiply standardises the real part


def _close(name, a, b, rtol=5e-4, atol_scale=5e-6):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    bound = rtol * np.abs(b) + atol_scale * (np.abs(b).max() + 1e-30)
    bad = np.abs(a - b) > bound
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} off, worst {np.abs(a - b).max():.3e} vs scale {np.abs(b).max():.3e}"


@pytest.mark.parametrize("J,iso,seed", [(24, False, 11), (52, False, 12), (52, True, 13)])
def test_fused_backward(J, iso, seed):
    import math
    from sings_amd.skinned import rasterize_skinned_gaussians, _RasterizeSkinnedGaussians
    dev = torch.device("cuda:0")
    s = _scene(5000, J, seed, isotropic=iso)
    rs = _settings(s, dev)
    req = lambda a: None if a is None else torch.from_numpy(a).to(dev).requires_grad_(True)
    t = lambda a: torch.from_numpy(a).to(dev)
    xyz, Rc, sc, op, sh, A, tr = req(s["xyz"]), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"]), req(s["A"]), req(s["transl"])
    m2d = torch.zeros(s["N"], 3, device=dev, requires_grad=True)      # per-call holder of the screen-space gradient
    color, radii, pxyz, pq, psc = rasterize_skinned_gaussians(xyz, Rc, sc, op, sh, t(s["w"]), A, rs, smpl_scale=t(s["smpl_scale"]),
                                                              transl=tr, return_posed=True, means2D=m2d)
    cam = s["cam"]
    o = ro.forward(pxyz.detach().cpu().numpy(), s["opac"], cam["world_view_transform"], cam["full_proj_transform"],
                   cam["camera_center"], 256, 224, math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"],
                   scales=psc.cpu().numpy(), rotations=pq.detach().cpu().numpy(), shs=s["shs"], sh_degree=3)
    dL = s["dL"].copy(); dL[:, o["margin"] < BORDER] = 0
    g = ro.backward(o, dL)
    # an extra loss directly on the posed means / quaternions exercises the upstream-gradient inputs
    wx = torch.from_numpy(np.random.RandomState(5).normal(size=(s["N"], 3)).astype(np.float32))
    wq = torch.from_numpy(np.random.RandomState(6).normal(size=(s["N"], 4)).astype(np.float32))
    loss = (color * t(dL)).sum() + (pxyz * wx.to(dev)).sum() + (pq * wq.to(dev)).sum()
    loss.backward()
    # reference: torch autograd through the restatement, seeded with the oracle's posed-space gradients
    (oxyz, oRc, osc, oA, otr), (pxyz_o, pq_o, psc_o, _) = _oracle_deform(s, grad=True)
    seeds = (pxyz_o * (torch.from_numpy(g["dL_dmeans3D"]) + wx)).sum() + (pq_o * (torch.from_numpy(g["dL_drots"]) + wq)).sum() \
        + (psc_o * torch.from_numpy(g["dL_dscales"])).sum()
    seeds.backward()
    _close("xyz_canon", xyz.grad.cpu().numpy(), oxyz.grad.numpy())
    _close("scales", sc.grad.cpu().numpy(), osc.grad.numpy())
    if not iso:
        _close("rotmat_canon", Rc.grad.cpu().numpy(), oRc.grad.numpy())
    _close("A", A.grad.cpu().numpy()[:, :3, :], oA.grad.numpy()[:, :3, :], rtol=2e-3, atol_scale=2e-4)
    assert np.abs(A.grad.cpu().numpy()[:, 3, :]).max() == 0
    _close("transl", tr.grad.cpu().numpy(), otr.grad.numpy(), rtol=2e-3, atol_scale=2e-4)
    _close("opacity", op.grad.cpu().numpy(), g["dL_dopacity"], rtol=2e-4, atol_scale=2e-6)
    _close("sh", sh.grad.cpu().numpy(), g["dL_dsh"], rtol=2e-4, atol_scale=2e-6)
    _close("viewspace", m2d.grad.cpu().numpy(), g["dL_dmean2D"], rtol=2e-4, atol_scale=2e-6)
    assert not hasattr(_RasterizeSkinnedGaussians, "last_viewspace_grad")      # the round-1 class attribute (last call wins) is gone


def test_fused_op_learns_the_long_rows_hint_and_reports_a_violation():
    """rasterize_skinned_gaussians in "sync" mode reads the count word's SG_COUNT_FLAG_HALF_LONG_ROWS bit; the next call of that
    (device, P, W, H) -- in any overflow mode -- passes SG_FLAG_LONG_ROWS (direct binning of the few-tile frame) and returns the same
    bits.  A violated hint: "sync" renders the frame again without it; "deferred" reports it from check_deferred_overflow()."""
    from sings_amd import overflow as ov, rasterizer as rz
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = torch.device("cuda:0")
    s = _scene(5000, 24, 11, isotropic=False)
    rs = _settings(s, dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    key = (dev.index, s["N"], 256, 224)
    rz.reset_overflow_state(dev)

    def frame(scale=1.0):
        req = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)
        xyz, Rc, sc, op, sh = req(s["xyz"] * np.float32(scale)), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"])
        color, radii = rasterize_skinned_gaussians(xyz, Rc, sc, op, sh, t(s["w"]), t(s["A"]), rs, smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]))
        color.backward(t(s["dL"]))
        return color.detach().clone(), [x.grad.clone() for x in (xyz, Rc, sc, op, sh)]
    c0, g0 = frame()
    assert ov._rows_ok.get(key) is True
    c1, g1 = frame()                                            # hinted
    assert torch.equal(c0, c1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    rz.set_deferred_overflow_check(True, device=dev)
    try:
        c2, g2 = frame()                                        # hinted, no host read
        assert rz.check_deferred_overflow(dev) is not None
        assert torch.equal(c0, c2) and all(torch.equal(a, b) for a, b in zip(g0, g2))
    finally:
        rz.set_overflow_check("sync")
    rz.reset_overflow_state(dev)


def test_avatar_shaped_scene_with_long_lists_against_the_oracle():
    """The geometry of the reference's workload, scaled down so that the oracle finishes in seconds: one narrow body far from
    a long-focal-length camera (fx = 5000 at 512 x 896 -> 937.5 at 96 x 128, z ~ 10 m), J = 52, anisotropic Gaussians a few
    millimetres across with high opacity.  All splats fall on a handful of tiles -- lists of several thousand entries (bucket
    sort, depth segments, checkpoints) whose pixels saturate after a fraction of the list (live-box culling, early exit).
    Image, and every gradient of the fused path including dL/dA and dL/dtransl, against the oracle."""
    import math
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = torch.device("cuda:0")
    N, J, Wd, Hd = 30000, 52, 96, 128
    s = _scene(N, J, 41)
    rs_ = np.random.RandomState(41)
    s["xyz"] = (rs_.normal(0, 1, (N, 3)) * np.array([0.05, 0.13, 0.04])).astype(np.float32)
    s["scales"] = np.exp(rs_.normal(-5.3, 0.3, (N, 3))).astype(np.float32)
    s["opac"] = rs_.uniform(0.3, 0.95, (N, 1)).astype(np.float32)
    s["A"][:, :3, 3] *= 0.2                                               # (joint offsets of centimetres: the body stays narrow)
    s["transl"] = np.array([-0.01, 0.02, 10.0], np.float32)
    s["cam"] = make_camera(np.eye(4, dtype=np.float32), 937.5, 937.5, Wd / 2, Hd / 2, Wd, Hd)
    s["dL"] = rs_.normal(0, 1, (3, Hd, Wd)).astype(np.float32)
    rs = _settings(s, dev)
    req = lambda a: None if a is None else torch.from_numpy(a).to(dev).requires_grad_(True)
    t = lambda a: torch.from_numpy(a).to(dev)
    xyz, Rc, sc, op, sh, A, tr = req(s["xyz"]), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"]), req(s["A"]), req(s["transl"])
    m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
    color, radii, pxyz, pq, psc = rasterize_skinned_gaussians(xyz, Rc, sc, op, sh, t(s["w"]), A, rs, smpl_scale=t(s["smpl_scale"]),
                                                              transl=tr, return_posed=True, means2D=m2d)
    cam = s["cam"]
    o = ro.forward(pxyz.detach().cpu().numpy(), s["opac"], cam["world_view_transform"], cam["full_proj_transform"],
                   cam["camera_center"], Wd, Hd, math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"],
                   scales=psc.cpu().numpy(), rotations=pq.detach().cpu().numpy(), shs=s["shs"], sh_degree=3)
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert tl.max() > 4096, tl.max()                                      # bucket-sorted lists, > 16 depth segments
    last = o["n_contrib"].reshape(Hd // 16, 16, Wd // 16, 16).transpose(0, 2, 1, 3).reshape(-1, 256)
    assert (np.median(last[tl > 4096], axis=1) < 0.5 * tl[tl > 4096]).all()   # ... whose typical pixel terminates long before the end
    assert tl.max() > 12288 and ((tl > 4096) & (tl <= 12288)).any()       # both long-list sort paths: in-LDS and multi-level
    assert np.array_equal(o["radii"], radii.cpu().numpy())
    strict = o["margin"] >= BORDER
    assert strict.mean() > 0.99
    assert np.abs(color.detach().cpu().numpy() - o["color"]).max(0)[strict].max() <= 2e-5
    dL = s["dL"].copy(); dL[:, ~strict] = 0
    g = ro.backward(o, dL)
    (color * t(dL)).sum().backward()
    (oxyz, oRc, osc, oA, otr), (pxyz_o, pq_o, psc_o, _) = _oracle_deform(s, grad=True)
    seeds = (pxyz_o * torch.from_numpy(g["dL_dmeans3D"])).sum() + (pq_o * torch.from_numpy(g["dL_drots"])).sum() \
        + (psc_o * torch.from_numpy(g["dL_dscales"])).sum()
    seeds.backward()
    # (segmented backward: the colour behind a segment comes from forward checkpoints -- a different fp32 rounding of the same
    #  quantity, see tests/test_gpu_raster.py::test_long_tile_lists_sort_paths)
    _close("xyz_canon", xyz.grad.cpu().numpy(), oxyz.grad.numpy(), rtol=1e-3, atol_scale=1e-5)
    _close("scales", sc.grad.cpu().numpy(), osc.grad.numpy(), rtol=1e-3, atol_scale=1e-5)
    _close("rotmat_canon", Rc.grad.cpu().numpy(), oRc.grad.numpy(), rtol=1e-3, atol_scale=1e-5)
    _close("A", A.grad.cpu().numpy()[:, :3, :], oA.grad.numpy()[:, :3, :], rtol=2e-3, atol_scale=2e-4)
    _close("transl", tr.grad.cpu().numpy(), otr.grad.numpy(), rtol=2e-3, atol_scale=2e-4)
    _close("opacity", op.grad.cpu().numpy(), g["dL_dopacity"], rtol=1e-3, atol_scale=1e-5)
    _close("sh", sh.grad.cpu().numpy(), g["dL_dsh"], rtol=1e-3, atol_scale=1e-5)
    _close("viewspace", m2d.grad.cpu().numpy(), g["dL_dmean2D"], rtol=1e-3, atol_scale=1e-5)


def test_fused_backward_deterministic_and_ext_refused():
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = torch.device("cuda:0")
    s = _scene(4000, 52, 21)
    rs = _settings(s, dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    outs = []
    for _ in range(2):
        req = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)
        xyz, Rc, sc, op, sh, A, tr = req(s["xyz"]), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"]), req(s["A"]), req(s["transl"])
        color, _ = rasterize_skinned_gaussians(xyz, Rc, sc, op, sh, t(s["w"]), A, rs, smpl_scale=t(s["smpl_scale"]), transl=tr)
        color.backward(t(s["dL"]))
        outs.append([x.grad.clone() for x in (xyz, Rc, sc, op, sh, A, tr)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    ext = (torch.zeros(3, device=dev), torch.eye(3, device=dev), torch.ones(1, device=dev))
    xyz = t(s["xyz"]).requires_grad_(True)
    color, _ = rasterize_skinned_gaussians(xyz, t(s["Rc"]), t(s["scales"]), t(s["opac"]), t(s["shs"]), t(s["w"]), t(s["A"]), rs,
                                           ext_tfs=ext)
    with pytest.raises(RuntimeError, match="forward-only"):
        color.sum().backward()


def test_cfg4_full_size_properties():
    """BASELINE configs[3] at full size (150 k canonical Gaussians, J = 52, 512x896, AMASS frame; longest tile list ~10^4:
    bucket sort, depth-segmented backward) through the pre-allocated engine: size-independent properties -- two runs bitwise
    identical (image, radii, every gradient incl. dL/dA), the backward linear in dL/dimage, the pair count within the capacity.
    (The same scene against the composed oracle: test_cfg4_full_size_against_the_oracle below.)"""
    import math, os
    from sings_amd.body import joint_transforms
    from sings_amd.engine import SkinnedEngine
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.scene import avatar_scene
    dev = torch.device("cuda:0")
    s = avatar_scene(N=150000, J=52)
    W, H, J, N = s["W"], s["H"], s["J"], 150000
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = s["cam"]
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=t(s["bg"]),
        scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]), projmatrix=t(cam["full_proj_transform"]), sh_degree=0,
        campos=t(cam["camera_center"]), prefiltered=False, debug=False)
    poses72 = np.load(os.path.join(os.path.dirname(__file__), "golden", "lbs_golden.npz"))["amass_poses_72"]
    pose = np.zeros(J * 3, np.float32); pose[:72] = poses72[17]; pose[:3] = 0
    A = joint_transforms(t(pose), t(s["joints_rest"]), tuple(s["parents"])).reshape(J, 16).contiguous()
    xyz, w, sc, op, sh = t(s["xyz_canon"]), t(s["lbs_weights"]), t(s["scales"]), t(s["opacities"]), t(s["shs"])
    eng = SkinnedEngine(N, J, W, H, sh.shape[1], dev, capacity_pairs=16 * N)
    eng.set_camera(rs)
    eng.set_frame(xyz, None, w, A, t(s["smpl_scale"]), t(s["transl"]))
    rng = np.random.RandomState(0)
    d1 = t(s["dL_dimage"]); d2 = t(rng.standard_normal(s["dL_dimage"].shape).astype(np.float32))

    def run(d):
        R = eng.forward(sh, op, sc, sync_num_rendered=True)
        eng.backward(sh, op, sc, d)
        torch.cuda.synchronize()
        return R, eng.color.clone(), eng.radii.clone(), eng.grad_flat.clone(), eng.d_A.clone(), eng.d_transl.clone()

    Ra, ca, ra, ga, dAa, dta = run(d1)
    Rb, cb, rb, gb, dAb, dtb = run(d1)
    assert Ra == Rb and 5e5 < Ra <= eng.cap
    assert torch.equal(ca, cb) and torch.equal(ra, rb) and torch.equal(ga, gb) and torch.equal(dAa, dAb) and torch.equal(dta, dtb)
    assert float((ra > 0).float().mean()) > 0.9 and float((ca - t(s["bg"])[:, None, None]).abs().max()) > 0.1
    _, _, _, g2, dA2, _ = run(d2)
    _, _, _, g12, dA12, _ = run(0.5 * d1 - 2.0 * d2)
    for a_, b_, c_, name in ((ga, g2, g12, "canonical-Gaussian gradients"), (dAa, dA2, dA12, "dL/dA")):
        ref = 0.5 * a_.double() - 2.0 * b_.double()
        err = (c_.double() - ref).abs().max().item(); scale = ref.abs().max().item()
        assert err <= 5e-5 * scale, (name, err, scale)


def _cfg4(dev, frame=17):
    """BASELINE configs[3] as bench.py --workload avatar builds it: avatar_scene(N = 150 000, J = 52), 512 x 896, fx = fy = 5000,
    AMASS frame `frame` of the committed 120 (global orientation zeroed: the body faces the camera)."""
    import math, os
    from sings_amd.body import joint_transforms
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.scene import avatar_scene
    s = avatar_scene(N=150000, J=52)
    J = s["J"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = s["cam"]
    rs = GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5),
        bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]), projmatrix=t(cam["full_proj_transform"]),
        sh_degree=0, campos=t(cam["camera_center"]), prefiltered=False, debug=False)
    poses72 = np.load(os.path.join(os.path.dirname(__file__), "golden", "lbs_golden.npz"))["amass_poses_72"]

    def A_of(f):
        pose = np.zeros(J * 3, np.float32); pose[:72] = poses72[f]; pose[:3] = 0
        return joint_transforms(t(pose), t(s["joints_rest"]), tuple(s["parents"])).reshape(J, 4, 4).contiguous()
    return s, rs, A_of


def _oracle_view(s, cam_args, pxyz, pq, psc, deg=0):
    import math
    cam = s["cam"]
    return ro.forward(pxyz, s["opacities"], cam["world_view_transform"], cam["full_proj_transform"], cam["camera_center"], s["W"], s["H"],
                      math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"], scales=psc, rotations=pq, shs=s["shs"],
                      sh_degree=deg)


def _posed_ulps(pxyz, pq, psc, oxyz, oq, osc):
    mag = np.abs(oxyz).max(1, keepdims=True)
    u_xyz = (np.abs(pxyz.astype(np.float64) - oxyz) / np.spacing(mag.astype(np.float32))).max()
    u_q = (np.abs(pq.astype(np.float64) - oq) / np.spacing(np.float32(1.0))).max()
    u_sc = (np.abs(psc.astype(np.float64) - osc) / np.spacing(np.abs(osc))).max()
    return float(u_xyz), float(u_q), float(u_sc)


def _oracle_lbs_gradients(s, A, g):
    """dL/d(canonical means, scales, A, transl) by autograd through oracle/lbs_oracle.py (pinned by the reference-generated
    lbs_golden.npz), seeded with the raster oracle's gradients w.r.t. the posed means / quaternions / scales."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone().requires_grad_(True)
    xyz, sc, A_, tr = T(s["xyz_canon"]), T(s["scales"]), T(A), T(s["transl"])
    eye = torch.eye(3)[None].repeat(s["N"], 1, 1)
    pxyz_o, pq_o, psc_o, _ = lo.deform_gaussians(xyz, eye, sc, torch.from_numpy(s["lbs_weights"]), A_,
                                                 smpl_scale=torch.from_numpy(s["smpl_scale"]), transl=tr)
    ((pxyz_o * torch.from_numpy(g["dL_dmeans3D"])).sum() + (pq_o * torch.from_numpy(g["dL_drots"])).sum()
     + (psc_o * torch.from_numpy(g["dL_dscales"])).sum()).backward()
    return xyz.grad.numpy(), sc.grad.numpy(), A_.grad.numpy(), tr.grad.numpy(), (pxyz_o.detach().numpy(), pq_o.detach().numpy(),
                                                                               psc_o.detach().numpy())


def test_cfg4_full_size_against_the_oracle():
    """BASELINE configs[3] AT FULL SIZE against the composed oracle (the CPU side needs ~4 s): the workload SinGS trains
    (human_complex.yaml:34-35, 95-96; the calls replaced are sings_hybrid.py:398-428 + gs_renderer_single.py:87-95).
     * posed means / quaternions / scales of the fused kernel vs oracle/lbs_oracle.py, in ulps (the seam between the two oracles);
     * the raster oracle on the kernel's own posed values: R, radii, rectangles, depth bits, upstream-format keys, the sorted
       lists (bucket-sorted: the longest has ~10^4 entries), ranges -- bit for bit; RGB <= 1e-5 off borderline pixels (those
       within the oracle's flip bound), final_T, n_contrib;
     * EVERY gradient of the fused op -- canonical means, scales, opacity, SH, the screen-space statistic, dL/dA and dL/dtransl --
       vs the raster oracle's explicit backward chained through the LBS oracle's autograd (four-workgroup composite of lists
       > 1024, sparse backward, record-valid bytes, segmented checkpoints: all at their production sizes)."""
    import test_gpu_raster as TR
    from sings_amd.inspect_ws import forward_with_state
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = torch.device("cuda:0")
    s, rs, A_of = _cfg4(dev)
    N = s["N"]
    A = A_of(17)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    req = lambda a: t(a).requires_grad_(True)
    xyz, sc, op, sh, tr = req(s["xyz_canon"]), req(s["scales"]), req(s["opacities"]), req(s["shs"]), req(s["transl"])
    A_g = A.clone().requires_grad_(True)
    m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
    color, radii, pxyz, pq, psc = rasterize_skinned_gaussians(xyz, None, sc, op, sh, t(s["lbs_weights"]), A_g, rs,
                                                              smpl_scale=t(s["smpl_scale"]), transl=tr, return_posed=True, means2D=m2d)
    c = lambda x: x.detach().cpu().numpy()
    o = _oracle_view(s, None, c(pxyz), c(pq), c(psc))
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert o["R"] > 5e5 and tl.max() > 8192, (o["R"], tl.max())
    # the plain path on the kernel's posed outputs exposes the workspaces: every integer of the binning, bit for bit
    st = forward_with_state(rs, pxyz.detach(), op.detach(), shs=sh.detach(), scales=psc.detach(), rotations=pq.detach(), capacity=8 * N)
    s_r = dict(s, H=s["H"], W=s["W"])
    TR._check_forward_state(s_r, st, o)
    assert torch.equal(st["color"], color.detach()) and torch.equal(st["radii"], radii)        # fused == plain, bit for bit
    TR._check_image(c(color), c(st["final_T"]), c(st["n_contrib"]), o)
    del st
    border = o["margin"] < BORDER
    dL = s["dL_dimage"].copy(); dL[:, border] = 0
    g = ro.backward(o, dL)
    (color * t(dL)).sum().backward()
    gx, gs, gA, gt, (oxyz, oq, osc) = _oracle_lbs_gradients(s, c(A), g)
    u = _posed_ulps(c(pxyz), c(pq), c(psc), oxyz, oq, osc)
    assert u[0] <= 2.0 and u[1] <= 8.0 and u[2] <= 1.0, u
    # (segmented backward: the colour behind a segment comes from forward checkpoints -- a different fp32 rounding of the same
    #  quantity; same tolerances as the scaled-down avatar scene above)
    _close("xyz_canon", c(xyz.grad), gx, rtol=1e-3, atol_scale=1e-5)
    _close("scales", c(sc.grad), gs, rtol=1e-3, atol_scale=1e-5)
    _close("A", c(A_g.grad)[:, :3, :], gA[:, :3, :], rtol=2e-3, atol_scale=2e-4)
    _close("transl", c(tr.grad), gt, rtol=2e-3, atol_scale=2e-4)
    _close("opacity", c(op.grad), g["dL_dopacity"], rtol=1e-3, atol_scale=1e-5)
    _close("sh", c(sh.grad), g["dL_dsh"], rtol=1e-3, atol_scale=1e-5)
    _close("viewspace", c(m2d.grad), g["dL_dmean2D"], rtol=1e-3, atol_scale=1e-5)


def test_cfg4_eight_frames_in_one_launch_against_the_oracle():
    """ONE K = 8 launch per kernel of the full-size avatar (sg_skinned_forward_frames / *_backward_*_frames: what bench.py
    --workload avatar and the chunked training step run) compared with the oracle DIRECTLY -- not through the chain "K-frame
    call == K single-frame calls == oracle" of tests/test_gpu_frames.py.  Every frame: posed values vs the LBS oracle in ulps,
    pair count and radii vs the raster oracle (bit for bit, on the launch's own posed outputs); frames 0 and 7: the image, dL/dA,
    dL/dtransl and the screen-space statistic; and the canonical-Gaussian gradient the launch leaves behind = the SUM over its
    eight frames of the oracle's gradients (raster oracle's explicit backward chained through the LBS oracle's autograd)."""
    from sings_amd.engine import SkinnedFramesEngine
    dev = torch.device("cuda:0")
    s, rs, A_of = _cfg4(dev)
    N, J, W, H, K = s["N"], s["J"], s["W"], s["H"], 8
    frames = [3, 17, 29, 41, 56, 70, 88, 101]
    A = torch.stack([A_of(f) for f in frames]).reshape(K, J, 16).contiguous()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs_ = np.random.RandomState(8)
    transl_n = (s["transl"][None] + rs_.normal(0, 0.02, (K, 3))).astype(np.float32)
    dL_n = rs_.normal(0, 1, (K, 3, H, W)).astype(np.float32)
    xyz, w, sc, op, sh = t(s["xyz_canon"]), t(s["lbs_weights"]), t(s["scales"]), t(s["opacities"]), t(s["shs"])
    eng = SkinnedFramesEngine(N, J, W, H, sh.shape[1], K, dev, 16 * N)
    eng.set_camera(rs)
    eng.set_frames(xyz, None, w, A, t(s["smpl_scale"]), t(transl_n))
    e = lambda *shp: torch.empty(shp, dtype=torch.float32, device=dev)
    posed = (e(K, N, 3), e(K, N, 4), e(K, N, 3))
    Rs = eng.forward(sh, op, sc, sync_num_rendered=True, posed_out=posed)
    assert max(Rs) <= eng.cap
    color = eng.color.cpu().numpy(); radii = eng.radii.cpu().numpy()
    pxyz, pq, psc = (x.cpu().numpy() for x in posed)
    sums = dict(xyz=0.0, sc=0.0, op=0.0, sh=0.0)
    per_frame = {}
    A_n = A.cpu().numpy().reshape(K, J, 4, 4)
    for f in range(K):
        sf = dict(s, transl=transl_n[f])
        o = _oracle_view(sf, None, pxyz[f], pq[f], psc[f])
        assert Rs[f] == o["R"] and np.array_equal(radii[f], o["radii"]), (f, Rs[f], o["R"])
        border = o["margin"] < BORDER
        dL_n[f][:, border] = 0
        g = ro.backward(o, dL_n[f])
        gx, gs, gA, gt, (oxyz, oq, osc) = _oracle_lbs_gradients(sf, A_n[f], g)
        u = _posed_ulps(pxyz[f], pq[f], psc[f], oxyz, oq, osc)
        assert u[0] <= 2.0 and u[1] <= 8.0 and u[2] <= 1.0, (f, u)
        sums["xyz"] = sums["xyz"] + gx.astype(np.float64); sums["sc"] = sums["sc"] + gs.astype(np.float64)
        sums["op"] = sums["op"] + g["dL_dopacity"].astype(np.float64); sums["sh"] = sums["sh"] + g["dL_dsh"].astype(np.float64)
        if f in (0, K - 1):
            per_frame[f] = (o, border, g, gA, gt)
    assert len(set(Rs)) > 1                                          # (the frames really differ)
    eng.backward(sh, op, sc, t(dL_n))
    torch.cuda.synchronize()
    for f, (o, border, g, gA, gt) in per_frame.items():
        diff = np.abs(color[f] - o["color"]).max(0)
        assert diff[~border].max() <= 1e-5, (f, diff[~border].max())
        over = diff[border] - (1e-5 + 1.001 * o["flip"][border])
        assert border.sum() == 0 or over.max() <= 0, (f, over.max())
        _close(f"A[{f}]", eng.d_A[f].cpu().numpy().reshape(J, 4, 4)[:, :3, :], gA[:, :3, :], rtol=2e-3, atol_scale=2e-4)
        _close(f"transl[{f}]", eng.d_transl[f].cpu().numpy(), gt, rtol=2e-3, atol_scale=2e-4)
        _close(f"viewspace[{f}]", eng.d_means2D[f].cpu().numpy(), g["dL_dmean2D"], rtol=1e-3, atol_scale=1e-5)
    _close("sum xyz_canon", eng.d_xyz.cpu().numpy(), sums["xyz"], rtol=1e-3, atol_scale=1e-5)
    _close("sum scales", eng.d_scales.cpu().numpy(), sums["sc"], rtol=1e-3, atol_scale=1e-5)
    _close("sum opacity", eng.d_opacity.cpu().numpy(), sums["op"], rtol=1e-3, atol_scale=1e-5)
    _close("sum sh", eng.d_sh.cpu().numpy(), sums["sh"], rtol=1e-3, atol_scale=1e-5)

def _avatar_shaped(N=30000, J=52, Wd=96, Hd=128, seed=41):
    """The scaled-down geometry of the reference's workload used by test_avatar_shaped_scene_with_long_lists_against_the_oracle."""
    s = _scene(N, J, seed)
    rs_ = np.random.RandomState(seed)
    s["xyz"] = (rs_.normal(0, 1, (N, 3)) * np.array([0.05, 0.13, 0.04])).astype(np.float32)
    s["scales"] = np.exp(rs_.normal(-5.3, 0.3, (N, 3))).astype(np.float32)
    s["opac"] = rs_.uniform(0.3, 0.95, (N, 1)).astype(np.float32)
    s["A"][:, :3, 3] *= 0.2
    s["transl"] = np.array([-0.01, 0.02, 10.0], np.float32)
    s["cam"] = make_camera(np.eye(4, dtype=np.float32), 937.5, 937.5, Wd / 2, Hd / 2, Wd, Hd)
    s["dL"] = rs_.normal(0, 1, (3, Hd, Wd)).astype(np.float32)
    return s


def seam_ulps(s, dev):
    """Posed means / quaternions / scales of the fused kernel against oracle/lbs_oracle.py, in ulps: a mean's error in units of
    the fp32 spacing at its point's largest coordinate magnitude (the blend T [v;1] + transl sums terms of that size), a
    quaternion's in units of the spacing at 1 (unit quaternions), a scale's at its own magnitude."""
    from sings_amd.skinned import rasterize_skinned_gaussians
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    Wd, Hd = int(s["cam"]["image_width"]), int(s["cam"]["image_height"])
    rs = _settings(s, dev)
    assert (rs.image_width, rs.image_height) == (Wd, Hd)
    with torch.no_grad():
        _, _, pxyz, pq, psc = rasterize_skinned_gaussians(
            t(s["xyz"]), t(s["Rc"]), t(s["scales"]), t(s["opac"]), t(s["shs"]), t(s["w"]), t(s["A"]), rs,
            smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), return_posed=True)
    _, (oxyz, oq, osc, _) = _oracle_deform(s)
    oxyz, oq, osc = oxyz.numpy(), oq.numpy(), osc.numpy()
    mag = np.abs(oxyz).max(1, keepdims=True)
    u_xyz = (np.abs(pxyz.cpu().numpy().astype(np.float64) - oxyz) / np.spacing(mag.astype(np.float32))).max()
    u_q = (np.abs(pq.cpu().numpy().astype(np.float64) - oq) / np.spacing(np.float32(1.0))).max()
    u_sc = (np.abs(psc.cpu().numpy().astype(np.float64) - osc) / np.spacing(np.abs(osc))).max()
    return float(u_xyz), float(u_q), float(u_sc)


@pytest.mark.parametrize("which", ["generic_J52", "generic_J24", "avatar_shaped_J52"])
def test_posed_values_seam_in_ulps(which):
    """The ONLY guard on the seam between the two oracles: test_fused_backward and the avatar-shaped scene feed the raster oracle
    the kernel's OWN posed outputs (MFMA k-ordered sums vs a BLAS order would otherwise flip tile rectangles), so what ties
    canonical -> posed to oracle/lbs_oracle.py (pinned by the reference-generated lbs_golden.npz) is this comparison.  Stated in
    ulps (see seam_ulps).  Observed on the MI355X (tests/tools/seam_ulps.py, J = 24 / 30 / 52 and the avatar-shaped scene): posed
    means 0 ulp, quaternions 1 ulp of 1.0, scales 0 ulp -- the oracle's matmul and the kernel's k-ordered MFMA chain agree to the
    last bit on these inputs; the bounds leave one BLAS re-association of headroom."""
    dev = torch.device("cuda:0")
    s = {"generic_J52": lambda: _scene(6000, 52, 2), "generic_J24": lambda: _scene(6000, 24, 1),
         "avatar_shaped_J52": lambda: _avatar_shaped()}[which]()
    u_xyz, u_q, u_sc = seam_ulps(s, dev)
    assert u_xyz <= 2.0, f"posed means off by {u_xyz:.1f} ulps"
    assert u_q <= 8.0, f"posed quaternions off by {u_q:.1f} ulps of 1.0"
    assert u_sc <= 1.0, f"posed scales off by {u_sc:.1f} ulps"
