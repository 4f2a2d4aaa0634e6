"""GPU parity of every projection path under general cameras (tests/camera_case.py): a rotated view off the origin, fx != fy, a
principal point off the image centre, and fov-clamped splats beyond the limit in x only, y only and both.

Every other GPU comparison with the oracle runs under the identity view (or the identity plus a shift), where each product with a
view-matrix entry is a product with 0 or 1: a transposed read of view[r + 4k], fx where fy belongs, x and y exchanged in the fov
clamp, an SH direction without the camera centre or a depth from the wrong column of the view pass there unnoticed.  Here the
drop-in rasterizer (forward state bit for bit, image, every gradient, the precomputed-input branch, the depth / alpha maps), the
fused skinned op (posed values, image, every gradient incl. dL/dA and dL/dtransl, its maps), the K-camera skinned launch, the
render glue and the SH colour are held against the oracle that tests/test_camera_general_host.py anchors under the same cameras.
Tolerances: those of tests/test_gpu_raster.py, test_gpu_skinned.py and test_gpu_aux_maps.py, unchanged.
"""
import functools
import math

import numpy as np
import pytest
import torch

import camera_case as cc
import test_gpu_aux_maps as TA
import test_gpu_raster as TR
import test_gpu_skinned as TS
from oracle import raster_oracle as ro

pytestmark = pytest.mark.gpu
BORDER = TR.BORDER
_id = lambda c: "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def _ref(case):
    """(scene, oracle forward) of a camera_case scene: computed once, shared, never modified."""
    s = cc.gpu_scene(*case)
    return s, TR._oracle(s)


def _leaves(s, dev):
    req = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True)
    m = req(s["means3D"])
    return dict(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=req(s["opacities"]), shs=req(s["shs"]),
                scales=req(s["scales"]), rotations=req(s["rotations"]))


@pytest.mark.parametrize("case", cc.FORWARD, ids=_id)
def test_drop_in_forward_state_and_image(case):
    """Per-Gaussian state (radii, depth bits, pixel centres, conics, colours, rectangles, SH clamp bits) bit for bit, R, ranges,
    sorted lists and keys equal, image by _check_image."""
    from sings_amd.inspect_ws import forward_with_state
    dev = TR._dev()
    s, o = _ref(case)
    t = lambda a: torch.from_numpy(a).to(dev)
    st = forward_with_state(TR._settings(s, dev, debug=True), t(s["means3D"]), t(s["opacities"]), shs=t(s["shs"]),
                            scales=t(s["scales"]), rotations=t(s["rotations"]))
    TR._check_forward_state(s, st, o)
    TR._check_image(st["color"].cpu().numpy(), st["final_T"].cpu().numpy(), st["n_contrib"].cpu().numpy(), o)


@pytest.mark.parametrize("case", cc.BACKWARD, ids=_id)
def test_drop_in_backward(case):
    """Every gradient of GaussianRasterizer against the oracle's explicit backward; the three fov-clamp groups once more on their
    own rows, so that their 120 rows are measured against their own scale and not the scene's."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = TR._dev()
    s, o = _ref(case)
    x = _leaves(s, dev)
    color, radii = GaussianRasterizer(TR._settings(s, dev))(**x)
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    border = o["margin"] < BORDER
    assert np.abs(color.detach().cpu().numpy() - o["color"]).max(0)[~border].max() <= TR.RGB_TOL
    dLn = s["dL_dimage"].copy(); dLn[:, border] = 0
    g = ro.backward(o, dLn)
    color.backward(torch.from_numpy(dLn).to(dev))
    pairs = (("means3D", x["means3D"], "dL_dmeans3D"), ("means2D", x["means2D"], "dL_dmean2D"), ("opacity", x["opacities"], "dL_dopacity"),
             ("sh", x["shs"], "dL_dsh"), ("scales", x["scales"], "dL_dscales"), ("rotations", x["rotations"], "dL_drots"))
    got = {name: ten.grad.cpu().numpy().reshape(g[key].shape) for name, ten, key in pairs}
    for name, _, key in pairs:
        TR._grad_close(name, got[name], g[key])
    for k, group in enumerate(("beyond x", "beyond y", "beyond both")):
        rows = (s["clamp_kind"] == k) & (o["radii"] > 0)
        assert rows.sum() >= 16 and np.abs(g["dL_dmeans3D"][rows]).max() > 0
        for name, _, key in pairs:
            TR._grad_close(f"{name} [{group}]", got[name][rows], g[key][rows])


def test_precomputed_colours_and_covariances_under_generic():
    """The colors_precomp and the cov3D_precomp branch (no SH, no scale / rotation chain: the covariance gradient comes straight
    out of the view-rotated Jacobian), forward and backward."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = TR._dev()
    s = cc.gpu_scene(*cc.PRECOMP[0])
    N = s["N"]
    colors = np.random.RandomState(0).uniform(0, 1, (N, 3)).astype(np.float32)
    o = TR._oracle(s, colors=colors)
    rs = TR._settings(s, dev)
    t = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)
    m, op, col, sc, rt = t(s["means3D"]), t(s["opacities"]), t(colors), t(s["scales"]), t(s["rotations"])
    m2 = torch.zeros_like(m, requires_grad=True)
    color, radii = GaussianRasterizer(rs)(means3D=m, means2D=m2, opacities=op, colors_precomp=col, scales=sc, rotations=rt)
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    border = o["margin"] < BORDER
    assert np.abs(color.detach().cpu().numpy() - o["color"]).max(0)[~border].max() <= TR.RGB_TOL
    dLn = s["dL_dimage"].copy(); dLn[:, border] = 0
    g = ro.backward(o, dLn)
    color.backward(torch.from_numpy(dLn).to(dev))
    for name, ten, key in (("colors", col, "dL_dcolor"), ("means3D", m, "dL_dmeans3D"), ("means2D", m2, "dL_dmean2D"),
                           ("opacity", op, "dL_dopacity"), ("scales", sc, "dL_dscales"), ("rotations", rt, "dL_drots")):
        TR._grad_close(name, ten.grad.cpu().numpy(), g[key])
    # cov3D_precomp: the oracle's own covariances in
    o2 = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                    s["tanfovy"], s["bg"], colors_precomp=colors, cov3D_precomp=o["cov3D"])
    border2 = o2["margin"] < BORDER
    dL2 = s["dL_dimage"].copy(); dL2[:, border2] = 0
    g2 = ro.backward(o2, dL2)
    cov = torch.from_numpy(o["cov3D"]).to(dev).requires_grad_(True)
    m_, op_, col_ = t(s["means3D"]), t(s["opacities"]), t(colors)
    color2, radii2 = GaussianRasterizer(rs)(means3D=m_, means2D=torch.zeros_like(m_, requires_grad=True), opacities=op_,
                                            colors_precomp=col_, cov3D_precomp=cov)
    np.testing.assert_array_equal(radii2.cpu().numpy(), o2["radii"])
    assert np.abs(color2.detach().cpu().numpy() - o2["color"]).max(0)[~border2].max() <= TR.RGB_TOL
    color2.backward(torch.from_numpy(dL2).to(dev))
    for name, ten, key in (("cov3D", cov, "dL_dcov3D"), ("means3D", m_, "dL_dmeans3D"), ("colors", col_, "dL_dcolor"),
                           ("opacity", op_, "dL_dopacity")):
        TR._grad_close(name + " (cov3D_precomp)", ten.grad.cpu().numpy(), g2[key])


# ---- the skinned paths -------------------------------------------------------------------------------------------------------------
def _to_world(cam, A, transl_view):
    """Joint transforms and translation that put the posed body where `transl_view` puts it in VIEW space: posed_world =
    R^T (posed_view - t), i.e. A' = diag(R^T, 1) A and transl' = R^T (transl_view - t) (the skinning weights sum to one)."""
    E = cam["extrinsic"]; R, t = E[:3, :3], E[:3, 3]
    A = np.asarray(A, np.float64).copy()
    A[..., :3, :] = R.T @ A[..., :3, :]
    return A.astype(np.float32), (R.T @ (np.asarray(transl_view, np.float64) - t)).astype(np.float32)


def _skinned_scene(name, N=3000, J=24, seed=51, W=256, H=224):
    s = TS._scene(N, J, seed)
    cam = cc.cameras(W, H)[name]
    s["A"], s["transl"] = _to_world(cam, s["A"], [-0.04, 0.09, 2.0])
    s.update(cam=cam, W=W, H=H)
    return s


def _skinned_oracle(s, pxyz, pq, psc, pair=False):
    cam = s["cam"]
    a = (pxyz, s["opac"], cam["world_view_transform"], cam["full_proj_transform"], cam["camera_center"], s["W"], s["H"],
         math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"])
    if pair:
        return TA._oracle_pair(*a, psc, pq, s["shs"], 3)
    return ro.forward(*a, scales=psc, rotations=pq, shs=s["shs"], sh_degree=3)


@pytest.mark.parametrize("name", ["generic", "roll", "offcentre"])
def test_fused_skinned_forward_and_backward(name):
    """rasterize_skinned_gaussians: posed values against the LBS oracle, fused == plain path on those values bit for bit, image
    against the raster oracle, and every gradient of test_gpu_skinned.py::test_fused_backward incl. dL/dA and dL/dtransl."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = TR._dev()
    s = _skinned_scene(name)
    N = s["N"]
    rs = TS._settings(s, dev)
    req = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)
    t = lambda a: torch.from_numpy(a).to(dev)
    xyz, Rc, sc, op, sh, A, tr = req(s["xyz"]), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"]), req(s["A"]), req(s["transl"])
    m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
    color, radii, pxyz, pq, psc = rasterize_skinned_gaussians(xyz, Rc, sc, op, sh, t(s["w"]), A, rs, smpl_scale=t(s["smpl_scale"]),
                                                              transl=tr, return_posed=True, means2D=m2d)
    c = lambda v: v.detach().cpu().numpy()
    _, (oxyz, oq, osc, _) = TS._oracle_deform(s)
    assert np.abs(c(pxyz) - oxyz.numpy()).max() < 2e-5
    assert np.abs(c(psc) - osc.numpy()).max() < 1e-8
    assert np.abs(c(pq) - oq.numpy()).max() < 2e-5
    assert int((radii > 0).sum()) > 0.5 * N
    with torch.no_grad():
        c2, r2 = GaussianRasterizer(rs)(means3D=pxyz.detach(), means2D=torch.zeros_like(pxyz), opacities=op.detach(), shs=sh.detach(),
                                        scales=psc.detach(), rotations=pq.detach())
    assert torch.equal(radii, r2) and torch.equal(color.detach(), c2)
    o = _skinned_oracle(s, c(pxyz), c(pq), c(psc))
    assert np.array_equal(o["radii"], c(radii))
    strict = o["margin"] >= BORDER
    assert strict.mean() > 0.99
    assert np.abs(c(color) - o["color"]).max(0)[strict].max() <= 1e-5
    dL = s["dL"].copy(); dL[:, ~strict] = 0
    g = ro.backward(o, dL)
    wx = torch.from_numpy(np.random.RandomState(5).normal(size=(N, 3)).astype(np.float32))
    wq = torch.from_numpy(np.random.RandomState(6).normal(size=(N, 4)).astype(np.float32))
    ((color * t(dL)).sum() + (pxyz * wx.to(dev)).sum() + (pq * wq.to(dev)).sum()).backward()
    (oxyz, oRc, osc, oA, otr), (pxyz_o, pq_o, psc_o, _) = TS._oracle_deform(s, grad=True)
    ((pxyz_o * (torch.from_numpy(g["dL_dmeans3D"]) + wx)).sum() + (pq_o * (torch.from_numpy(g["dL_drots"]) + wq)).sum()
     + (psc_o * torch.from_numpy(g["dL_dscales"])).sum()).backward()
    TS._close("xyz_canon", c(xyz.grad), oxyz.grad.numpy())
    TS._close("scales", c(sc.grad), osc.grad.numpy())
    TS._close("rotmat_canon", c(Rc.grad), oRc.grad.numpy())
    TS._close("A", c(A.grad)[:, :3, :], oA.grad.numpy()[:, :3, :], rtol=2e-3, atol_scale=2e-4)
    assert np.abs(c(A.grad)[:, 3, :]).max() == 0
    TS._close("transl", c(tr.grad), otr.grad.numpy(), rtol=2e-3, atol_scale=2e-4)
    TS._close("opacity", c(op.grad), g["dL_dopacity"], rtol=2e-4, atol_scale=2e-6)
    TS._close("sh", c(sh.grad), g["dL_dsh"], rtol=2e-4, atol_scale=2e-6)
    TS._close("viewspace", c(m2d.grad), g["dL_dmean2D"], rtol=2e-4, atol_scale=2e-6)


def test_k_camera_skinned_launch_sees_three_general_cameras():
    """SkinnedFramesEngine, K = 3, frames under the extrinsics of `yaw`, `generic` and `orbit3` (one intrinsic set per launch:
    generic's, fy = 1.2 fx), SH degree 3, 6-D canonical rotations: bit-equal to three SkinnedEngine calls chained with accumulate
    as in tests/test_gpu_frames.py -- and, directly, every frame's radii and image against the oracle on the launch's own posed
    values."""
    from sings_amd.body import joint_transforms
    from sings_amd.engine import SkinnedEngine, SkinnedFramesEngine
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.scene import avatar_scene
    dev = TR._dev()
    N, J, W, H, K = 4000, 52, 160, 288, 3
    base = cc.cameras(W, H)
    cams = [cc.retarget(base[n], base["generic"]) for n in ("yaw", "generic", "orbit3")]
    s = avatar_scene(N=N, J=J, W=W, H=H, seed=3, isotropic=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs = np.random.RandomState(3)
    jr = t(s["joints_rest"])
    A_np, tr_np = [], []
    for f in range(K):
        Af = joint_transforms(t(rs.normal(0, 0.2, J * 3).astype(np.float32)), jr, tuple(s["parents"])).reshape(J, 4, 4).cpu().numpy()
        a, tr = _to_world(cams[f], Af, np.array([-0.04, 0.09, 2.5]) + rs.normal(0, 0.03, 3))
        A_np.append(a.reshape(J, 16)); tr_np.append(tr)
    A, transl = t(np.stack(A_np)), t(np.stack(tr_np))
    view = np.stack([c["world_view_transform"] for c in cams]); proj = np.stack([c["full_proj_transform"] for c in cams])
    campos = np.stack([c["camera_center"] for c in cams])
    tx, ty = cams[0]["tanfovx"], cams[0]["tanfovy"]
    assert all(c["tanfovx"] == tx and c["tanfovy"] == ty for c in cams)

    def settings(vm, pm, cp):
        return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=tx, tanfovy=ty, bg=t(s["bg"]), scale_modifier=1.0,
                                             viewmatrix=vm, projmatrix=pm, sh_degree=3, campos=cp, prefiltered=False, debug=False)
    xyz, w, op, sh = t(s["xyz_canon"]), t(s["lbs_weights"]), t(s["opacities"]), t(s["shs"])
    sc = t(s["scales"] * np.float32(4.0))                             # (at this focal length: splats of a pixel or two)
    rot = t(rs.normal(size=(N, 6)).astype(np.float32))
    dL = t(rs.normal(0, 1, (K, 3, H, W)).astype(np.float32))
    cap = 24 * N
    ref = SkinnedEngine(N, J, W, H, 16, dev, cap, with_rot=True, rot_width=6)
    ref.throughput = True
    per_frame = []
    for f in range(K):
        ref.set_camera(settings(t(view[f]), t(proj[f]), t(campos[f])))
        ref.set_frame(xyz, rot, w, A[f], t(s["smpl_scale"]), transl[f])
        R = ref.forward(sh, op, sc, sync_num_rendered=True)
        assert 0 < R <= cap
        ref.backward(sh, op, sc, dL[f], accumulate=f > 0)
        torch.cuda.synchronize()
        per_frame.append([v.clone() for v in (ref.color, ref.radii, ref.d_means2D, ref.d_A, ref.d_transl)] + [R])
    ref_grad = ref.grad_flat.clone()
    eng = SkinnedFramesEngine(N, J, W, H, 16, K, dev, cap, with_rot=True, rot_width=6)
    eng.set_camera(settings(t(view), t(proj), t(campos)))
    eng.set_frames(xyz, rot, w, A, t(s["smpl_scale"]), transl)
    e = lambda *shp: torch.empty(shp, dtype=torch.float32, device=dev)
    posed = (e(K, N, 3), e(K, N, 4), e(K, N, 3))
    Rs = eng.forward(sh, op, sc, sync_num_rendered=True, posed_out=posed)
    eng.backward(sh, op, sc, dL)
    torch.cuda.synchronize()
    assert Rs == [p[5] for p in per_frame]
    for f in range(K):
        c, r, m2, dA, dt, _ = per_frame[f]
        assert torch.equal(eng.color[f], c), f"image of frame {f}"
        assert torch.equal(eng.radii[f], r) and torch.equal(eng.d_means2D[f], m2), f"radii / means2D of frame {f}"
        assert torch.equal(eng.d_A[f], dA) and torch.equal(eng.d_transl[f], dt), f"dL/dA, dL/dtransl of frame {f}"
    assert torch.equal(eng.grad_flat, ref_grad) and float(ref_grad.abs().max()) > 0
    pxyz, pq, psc = (v.cpu().numpy() for v in posed)
    color = eng.color.cpu().numpy(); radii = eng.radii.cpu().numpy()
    for f in range(K):
        o = ro.forward(pxyz[f], s["opacities"], view[f], proj[f], campos[f], W, H, tx, ty, s["bg"], scales=psc[f], rotations=pq[f],
                       shs=s["shs"], sh_degree=3)
        assert Rs[f] == o["R"] and np.array_equal(radii[f], o["radii"]), (f, Rs[f], o["R"])
        assert (o["radii"] > 0).mean() > 0.5, f
        strict = o["margin"] >= BORDER
        assert strict.mean() > 0.99 and np.abs(color[f] - o["color"]).max(0)[strict].max() <= 1e-5, f


# ---- depth and alpha maps ----------------------------------------------------------------------------------------------------------
def test_drop_in_depth_and_alpha_maps_under_generic():
    """rasterize_gaussians_aux: the depth map reads column 2 of the view (z = m2 x + m6 y + m10 z + m14) and chains dL/dz back
    through that row; under the identity view the row is (0, 0, 1)."""
    dev = TR._dev()
    s = cc.gpu_scene(*cc.AUX[0])
    o, oa = TA._oracle_scene(s)
    _, (color, radii, depth, alpha) = TA._run_aux(s, dev)
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    strict = TA._check_maps(o, oa, depth, alpha)
    TA._check_grads(s, dev, o, oa, strict, "cda", 134)


def test_skinned_depth_and_alpha_maps_under_generic():
    """tests/test_gpu_aux_maps.py::test_skinned_maps_and_gradients_against_the_oracle under `generic`, that file's tolerances."""
    from oracle import lbs_oracle as lo
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = TR._dev()
    s = _skinned_scene("generic", seed=52)
    N, Wd, Hd, cam = s["N"], s["W"], s["H"], s["cam"]
    req = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)
    t = lambda a: torch.from_numpy(a).to(dev)
    xyz, Rc, sc, op, sh, A, tr = req(s["xyz"]), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"]), req(s["A"]), req(s["transl"])
    m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
    color, radii, pxyz, pq, psc, depth, alpha = rasterize_skinned_gaussians(
        xyz, Rc, sc, op, sh, t(s["w"]), A, TA._skin_settings(s, dev), smpl_scale=t(s["smpl_scale"]), transl=tr, return_posed=True,
        means2D=m2d, return_aux=True)
    o, oa = _skinned_oracle(s, pxyz.detach().cpu().numpy(), pq.detach().cpu().numpy(), psc.cpu().numpy(), pair=True)
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    assert (o["radii"] > 0).mean() > 0.5
    strict = TA._check_maps(o, oa, depth, alpha)
    rng = np.random.RandomState(17)
    dLc = s["dL"].copy(); dLc[:, ~strict] = 0
    gD = rng.normal(0, 1, (Hd, Wd)).astype(np.float32); gD[~strict] = 0
    gA = rng.normal(0, 1, (Hd, Wd)).astype(np.float32); gA[~strict] = 0
    ((color * t(dLc)).sum() + (depth[0] * t(gD)).sum() + (alpha[0] * t(gA)).sum()).backward()
    ref = TA._reference_grads(o, oa, dLc, gD, gA, cam["world_view_transform"])
    T = lambda a: torch.from_numpy(a).clone().requires_grad_(True)
    oxyz, oRc, osc, oA, otr = T(s["xyz"]), T(s["Rc"]), T(s["scales"]), T(s["A"]), T(s["transl"])
    pxyz_o, pq_o, psc_o, _ = lo.deform_gaussians(oxyz, oRc, osc, torch.from_numpy(s["w"]), oA,
                                                 smpl_scale=torch.from_numpy(s["smpl_scale"]), transl=otr)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    ((pxyz_o * f(ref["means3D"])).sum() + (pq_o * f(ref["rotations"])).sum() + (psc_o * f(ref["scales"])).sum()).backward()
    TA._grad_close("xyz_canon", xyz.grad.cpu().numpy(), oxyz.grad.numpy(), atol=1e-5)
    TA._grad_close("rotmat_canon", Rc.grad.cpu().numpy(), oRc.grad.numpy(), atol=1e-5)
    TA._grad_close("scales", sc.grad.cpu().numpy(), osc.grad.numpy(), atol=1e-5)
    TA._grad_close("opacity", op.grad.cpu().numpy(), ref["opacities"])
    TA._grad_close("sh", sh.grad.cpu().numpy(), ref["shs"])
    TA._grad_close("viewspace", m2d.grad.cpu().numpy(), ref["means2D"])
    TA._grad_close("A", A.grad.cpu().numpy()[:, :3, :], oA.grad.numpy()[:, :3, :], rtol=2e-3, atol=2e-4)
    TA._grad_close("transl", tr.grad.cpu().numpy(), otr.grad.numpy(), rtol=2e-3, atol=2e-4)


# ---- the render glue ---------------------------------------------------------------------------------------------------------------
def _data(cam, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(fovx=cam["fovx"], fovy=cam["fovy"], image_height=cam["H"], image_width=cam["W"],
                world_view_transform=t(cam["world_view_transform"]), full_proj_transform=t(cam["full_proj_transform"]),
                camera_center=t(cam["camera_center"]))


def test_render_through_an_orbit_camera():
    """renderer.render() with the camera dict of an orbit view (what FrameAnimator and validate render through)."""
    from sings_amd.renderer import render
    dev = TR._dev()
    s, o = _ref(cc.RENDER[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with torch.no_grad():
        pkg = render(t(s["means3D"]), t(s["shs"]), t(s["opacities"]), t(s["scales"]), t(s["rotations"]), _data(s["cam"], dev),
                     bg_color=t(s["bg"]), active_sh_degree=s["sh_degree"])
    np.testing.assert_array_equal(pkg["radii"].cpu().numpy(), o["radii"])
    assert torch.equal(pkg["visibility_filter"], pkg["radii"] > 0)
    strict = o["margin"] >= BORDER
    assert np.abs(pkg["render_raw"].cpu().numpy() - o["color"]).max(0)[strict].max() <= 1e-5
    assert np.abs(pkg["render"].cpu().numpy() - np.clip(o["color"], 0, 1)).max(0)[strict].max() <= 1e-5


def test_k_path_of_the_renderer_stacks_two_orbit_cameras():
    """get_render_pkgs_fused with a LIST of camera dicts (one view matrix per frame stacked into a K-camera launch): orbit1 and
    orbit3 together, each frame's radii and image against the oracle on the posed values of the single-frame fused op."""
    from sings_amd.renderer import get_render_pkgs_fused
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = TR._dev()
    W, H = 256, 224
    s = TS._scene(3000, 24, 53)
    s["transl"] = np.array([0.02, -0.2, 0.05], np.float32)            # the orbit looks at the origin from 5 m
    s.update(W=W, H=H)
    base = cc.cameras(W, H)
    cams = [base["orbit1"], base["orbit3"]]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    canon = dict(xyz_canon=t(s["xyz"]), rotmat_canon=t(s["Rc"]), scales=t(s["scales"]), opacity=t(s["opac"]), shs=t(s["shs"]),
                 lbs_weights=t(s["w"]), active_sh_degree=3)
    A = t(np.stack([s["A"], s["A"]])); transl = t(np.stack([s["transl"], s["transl"]]))
    with torch.no_grad():
        pk = get_render_pkgs_fused([_data(c, dev) for c in cams], canon, A, t(s["bg"]), smpl_scale=t(s["smpl_scale"]), transl=transl)
        s["cam"] = cams[0]
        _, _, pxyz, pq, psc = rasterize_skinned_gaussians(canon["xyz_canon"], canon["rotmat_canon"], canon["scales"], canon["opacity"],
                                                          canon["shs"], canon["lbs_weights"], t(s["A"]), TS._settings(s, dev),
                                                          smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), return_posed=True)
    c = lambda v: v.cpu().numpy()
    images = []
    for f, cam in enumerate(cams):
        s["cam"] = cam
        o = _skinned_oracle(s, c(pxyz), c(pq), c(psc))
        assert np.array_equal(c(pk["radii"][f]), o["radii"]) and (o["radii"] > 0).mean() > 0.5, f
        strict = o["margin"] >= BORDER
        assert strict.mean() > 0.99 and np.abs(c(pk["render_raw"][f]) - o["color"]).max(0)[strict].max() <= 1e-5, f
        images.append(o["color"])
    assert np.abs(images[0] - images[1]).max() > 0.1                  # (the two views really differ)


# ---- SH colour with the camera off the origin --------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_colour_with_the_camera_centre_off_the_origin(deg):
    """tests/test_gpu_raster.py::test_sh_colour_against_the_reference_spherical_harmonics on the shifted groups: colours, clamp
    flags and dL/dsh of golden G9 when mean - campos, and neither the mean nor the view-space point, is the direction."""
    import sh_case
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from sings_amd.inspect_ws import forward_with_state
    dev = TR._dev()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    seen = 0
    for g in cc.shifted_sh_groups():
        rs = GaussianRasterizationSettings(image_height=sh_case.H, image_width=sh_case.W, tanfovx=sh_case.TANFOV, tanfovy=sh_case.TANFOV,
                                           bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=t(g["viewmatrix"]),
                                           projmatrix=t(g["projmatrix"]), sh_degree=deg, campos=t(g["campos"]), prefiltered=False,
                                           debug=False)
        st = forward_with_state(rs, t(g["means3D"]), t(g["opacities"]), shs=t(g["shs"]), scales=t(g["scales"]), rotations=t(g["rotations"]))
        assert bool((st["radii"] > 0).all())
        rgb, clamped = sh_case.expected_rgb(deg, g["idx"])
        got = st["rgb"].cpu().numpy()
        assert np.abs(got - rgb).max() <= 2e-6, np.abs(got - rgb).max()
        sure = np.abs(sh_case.G9[f"eval_deg{deg}"][g["idx"]] + 0.5) > 1e-5
        bits = st["clamp_bits"].cpu().numpy()
        got_clamped = np.stack([(bits >> c) & 1 for c in range(3)], 1).astype(bool)
        assert np.array_equal(got_clamped[sure], clamped[sure])
        seen += g["idx"].size
        if deg == 3:
            o = ro.forward(g["means3D"], g["opacities"], g["viewmatrix"], g["projmatrix"], g["campos"], sh_case.W, sh_case.H,
                           sh_case.TANFOV, sh_case.TANFOV, np.zeros(3, np.float32), scales=g["scales"], rotations=g["rotations"],
                           shs=g["shs"], sh_degree=deg)
            dL = np.random.RandomState(1).normal(0, 1, (3, sh_case.H, sh_case.W)).astype(np.float32)
            dL[:, o["margin"] < BORDER] = 0
            gr = ro.backward(o, dL)
            dcol = np.where(o["clamped"].astype(bool), 0.0, gr["dL_dcolor"])
            want = sh_case.G9["basis_deg3"][g["idx"]][:, :, None] * dcol[:, None, :]
            sh = t(g["shs"]).requires_grad_(True)
            m = t(g["means3D"])
            color, _ = GaussianRasterizer(rs)(means3D=m, means2D=torch.zeros_like(m), opacities=t(g["opacities"]), shs=sh,
                                              scales=t(g["scales"]), rotations=t(g["rotations"]))
            color.backward(t(dL))
            TR._grad_close("dL/dsh vs reference basis", sh.grad.cpu().numpy(), want, rtol=2e-4, atol=2e-6)
    assert seen == 512
