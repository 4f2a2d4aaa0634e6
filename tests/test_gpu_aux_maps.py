"""GPU parity of the depth and alpha maps (rasterize_gaussians_aux, rasterize_skinned_gaussians(return_aux=True)).

The reference is oracle/raster_aux.py: a composition of the existing raster oracle, two passes over the same Gaussians:
 * the colour pass with the scene's colours and background;
 * the aux pass with colors_precomp = (z, 1, 0) and background 0, whose channels 0 and 1 are depth and alpha.
Reference gradients: the colour pass's backward + the aux pass's backward seeded with (dL/ddepth, dL/dalpha, 0) + the aux pass's
dL/dcolour[:, 0] (= dL/dz) chained through the view row of z into the means (the posed means, then LBS, for the skinned op).
Pixels within 2e-5 of a hard threshold of the oracle are excluded from the comparisons and carry no gradient, as in
tests/test_gpu_raster.py.
"""
import math

import numpy as np
import pytest
import torch

from oracle import lbs_oracle as lo
from oracle.raster_aux import oracle_pair as _oracle_pair, reference_grads as _reference_grads
from sings_amd.camera import make_camera
from sings_amd.scene import synthetic_scene

pytestmark = pytest.mark.gpu
BORDER = 2e-5

# few tiles (<= 4096 tile counters: deep forward, sparse backward), then many tiles (plain forward, dense backward)
FEW = [(2000, 128, 128, 3, 1), (3000, 200, 136, 1, 11)]
MANY = [(40000, 1600, 1056, 1, 41)]


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _settings(s, dev):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
        scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]), sh_degree=s["sh_degree"],
        campos=t(s["campos"]), prefiltered=False, debug=False)


def _grad_close(name, a, b, rtol=1e-3, atol=6e-6):
    a = np.asarray(a, np.float64).reshape(np.shape(b)); b = np.asarray(b, np.float64)
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b)
    bad = err > rtol * np.abs(b) + atol * scale
    assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} off; worst abs {err.max():.3e} (scale {scale:.3e})"


def _scene(N, W, H, deg, seed, opacity_scale=1.0):
    s = synthetic_scene(N, W, H, deg, seed)
    s["opacities"] = (s["opacities"] * opacity_scale).astype(np.float32)
    return s


def _oracle_scene(s):
    return _oracle_pair(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                        s["tanfovy"], s["bg"], s["scales"], s["rotations"], s["shs"], s["sh_degree"])


def _inputs(s, dev):
    req = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True)
    m = req(s["means3D"])
    return dict(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=req(s["opacities"]), shs=req(s["shs"]),
                scales=req(s["scales"]), rotations=req(s["rotations"]))


def _run_aux(s, dev, x=None):
    from diff_gaussian_rasterization import GaussianRasterizer
    x = x or _inputs(s, dev)
    return x, GaussianRasterizer(_settings(s, dev)).forward_aux(**x)


def _check_maps(o, oa, depth, alpha):
    strict = o["margin"] >= BORDER
    assert strict.mean() > 0.99
    a = alpha.detach().cpu().numpy()[0]; d = depth.detach().cpu().numpy()[0]
    vis = o["radii"] > 0
    zmax = np.abs(o["depths"][vis]).max()
    assert np.abs(a - oa["color"][1])[strict].max() <= 1e-5
    assert np.abs(d - oa["color"][0])[strict].max() <= 1e-5 * zmax
    # the alpha map is the composite's own 1 - T_final
    assert np.abs(a - (1.0 - o["final_T"].reshape(a.shape)))[strict].max() <= 1e-5
    return strict


def _loss_maps(s, strict, rng, which):
    H, W = s["H"], s["W"]
    dLc = s["dL_dimage"].copy() if "c" in which else np.zeros((3, H, W), np.float32)
    gD = rng.normal(0, 1, (H, W)).astype(np.float32) if "d" in which else np.zeros((H, W), np.float32)
    gA = rng.normal(0, 1, (H, W)).astype(np.float32) if "a" in which else np.zeros((H, W), np.float32)
    dLc[:, ~strict] = 0; gD[~strict] = 0; gA[~strict] = 0
    return dLc, gD, gA


def _check_grads(s, dev, o, oa, strict, which, seed):
    x, (color, radii, depth, alpha) = _run_aux(s, dev)
    dLc, gD, gA = _loss_maps(s, strict, np.random.RandomState(seed), which)
    t = lambda a: torch.from_numpy(a).to(dev)
    loss = (color * t(dLc)).sum() + (depth[0] * t(gD)).sum() + (alpha[0] * t(gA)).sum()
    loss.backward()
    ref = _reference_grads(o, oa, dLc, gD, gA, s["viewmatrix"])
    for name in ("means3D", "means2D", "opacities", "scales", "rotations", "shs"):
        _grad_close(name, x[name].grad.cpu().numpy(), ref[name])


@pytest.mark.parametrize("N,W,H,deg,seed", FEW + MANY)
def test_maps_and_gradients_against_the_oracle(N, W, H, deg, seed):
    dev = _dev()
    s = _scene(N, W, H, deg, seed)
    o, oa = _oracle_scene(s)
    _, (color, radii, depth, alpha) = _run_aux(s, dev)
    assert tuple(depth.shape) == (1, H, W) and tuple(alpha.shape) == (1, H, W)
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    strict = _check_maps(o, oa, depth, alpha)
    _check_grads(s, dev, o, oa, strict, "cda", seed + 100)


@pytest.mark.parametrize("which", ["d", "a"])
@pytest.mark.parametrize("N,W,H,deg,seed", [FEW[0], MANY[0]])
def test_depth_alone_and_alpha_alone(N, W, H, deg, seed, which):
    dev = _dev()
    s = _scene(N, W, H, deg, seed)
    o, oa = _oracle_scene(s)
    _check_grads(s, dev, o, oa, o["margin"] >= BORDER, which, seed + 200)


@pytest.mark.parametrize("opacity_scale", [0.25, 1.0])
def test_segmented_lists_with_early_termination(opacity_scale):
    """Few-tile lists of several 256-entry depth segments whose pixels saturate inside the list: D checkpoints seed the
    backward of the segments in front."""
    dev = _dev()
    s = _scene(24000, 96, 80, 2, 43, opacity_scale)
    o, oa = _oracle_scene(s)
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert tl.max() > 3 * 256 and o["n_contrib"].max() < tl.max()
    _, (color, radii, depth, alpha) = _run_aux(s, dev)
    strict = _check_maps(o, oa, depth, alpha)
    _check_grads(s, dev, o, oa, strict, "cda", 7)


def test_full_size_cfg3_view():
    dev = _dev()
    s = _scene(200000, 1920, 1080, 3, 3)
    o, oa = _oracle_scene(s)
    _, (color, radii, depth, alpha) = _run_aux(s, dev)
    strict = _check_maps(o, oa, depth, alpha)
    _check_grads(s, dev, o, oa, strict, "cda", 9)


@pytest.mark.parametrize("N,W,H,deg,seed", [FEW[0], MANY[0]])
def test_colour_radii_and_colour_gradients_unchanged(N, W, H, deg, seed):
    """The aux op's colour and radii are the plain op's bits; a colour-only loss gives the plain op's gradients bit for bit."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = _dev()
    s = _scene(N, W, H, deg, seed)
    dL = torch.from_numpy(s["dL_dimage"]).to(dev)
    xp = _inputs(s, dev)
    cp, rp = GaussianRasterizer(_settings(s, dev))(**xp)
    (cp * dL).sum().backward()
    xa, (ca, ra, depth, alpha) = _run_aux(s, dev)
    (ca * dL).sum().backward()
    assert torch.equal(ca.detach(), cp.detach()) and torch.equal(ra, rp)
    for name in xp:
        assert torch.equal(xa[name].grad, xp[name].grad), name


@pytest.mark.parametrize("N,W,H,deg,seed", [FEW[1], MANY[0]])
def test_deterministic_and_hinted_call(N, W, H, deg, seed):
    """Two backward runs give identical bits; the next call of the same scene runs with the learned short-list / long-rows
    hints and gives the same maps."""
    dev = _dev()
    s = _scene(N, W, H, deg, seed)
    rng = np.random.RandomState(3)
    t = lambda a: torch.from_numpy(a).to(dev)
    gD, gA = t(rng.normal(0, 1, (H, W)).astype(np.float32)), t(rng.normal(0, 1, (H, W)).astype(np.float32))
    dL = t(s["dL_dimage"])
    runs = []
    for _ in range(2):
        x, (color, radii, depth, alpha) = _run_aux(s, dev)
        ((color * dL).sum() + (depth[0] * gD).sum() + (alpha[0] * gA).sum()).backward()
        runs.append((depth.detach().clone(), alpha.detach().clone(), {k: v.grad.clone() for k, v in x.items()}))
    (d0, a0, g0), (d1, a1, g1) = runs
    assert torch.equal(d0, d1) and torch.equal(a0, a1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ---- the skinned op ------------------------------------------------------------------------------------------------------------
def _skin_scene(N, J, seed, Wd=256, Hd=224, f=1500.0):
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
    Rc = lo.rotation_6d_to_matrix(torch.from_numpy(rs.normal(size=(N, 6)).astype(np.float32))).numpy()
    scales = np.exp(rs.normal(-4.6, 0.4, (N, 3))).astype(np.float32)
    opac = rs.uniform(0.05, 0.95, (N, 1)).astype(np.float32)
    shs = np.concatenate([rs.normal(0, 1, (N, 1, 3)), rs.normal(0, 0.15, (N, 15, 3))], 1).astype(np.float32)
    cam = make_camera(np.eye(4, dtype=np.float32), f, f, Wd / 2, Hd / 2, Wd, Hd)
    return dict(N=N, J=J, xyz=xyz, A=A, w=w.astype(np.float32), Rc=Rc, scales=scales, opac=opac, shs=shs, cam=cam, W=Wd, H=Hd,
                smpl_scale=np.array([1.07], np.float32), transl=np.array([-0.04, 0.09, 4.0], np.float32),
                bg=np.array([1, 1, 1], np.float32), dL=rs.normal(0, 1, (3, Hd, Wd)).astype(np.float32))


def _avatar_shaped(N=30000, J=52, Wd=96, Hd=128, seed=41):
    """One narrow body far from a long-focal-length camera: a handful of tiles with lists of several thousand entries."""
    s = _skin_scene(N, J, seed, Wd, Hd, 937.5)
    rs_ = np.random.RandomState(seed)
    s["xyz"] = (rs_.normal(0, 1, (N, 3)) * np.array([0.05, 0.13, 0.04])).astype(np.float32)
    s["scales"] = np.exp(rs_.normal(-5.3, 0.3, (N, 3))).astype(np.float32)
    s["opac"] = rs_.uniform(0.3, 0.95, (N, 1)).astype(np.float32)
    s["A"][:, :3, 3] *= 0.2
    s["transl"] = np.array([-0.01, 0.02, 10.0], np.float32)
    return s


def _skin_settings(s, dev):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    c = s["cam"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return GaussianRasterizationSettings(
        image_height=c["image_height"], image_width=c["image_width"], tanfovx=math.tan(c["fovx"] * 0.5),
        tanfovy=math.tan(c["fovy"] * 0.5), bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(c["world_view_transform"]),
        projmatrix=t(c["full_proj_transform"]), sh_degree=3, campos=t(c["camera_center"]), prefiltered=False, debug=False)


@pytest.mark.parametrize("which", ["small", "long_lists"])
def test_skinned_maps_and_gradients_against_the_oracle(which):
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = _dev()
    s = _skin_scene(5000, 24, 12) if which == "small" else _avatar_shaped()
    N, Wd, Hd, cam = s["N"], s["W"], s["H"], s["cam"]
    req = lambda a: torch.from_numpy(a).to(dev).requires_grad_(True)
    t = lambda a: torch.from_numpy(a).to(dev)
    xyz, Rc, sc, op, sh, A, tr = req(s["xyz"]), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"]), req(s["A"]), req(s["transl"])
    m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
    color, radii, pxyz, pq, psc, depth, alpha = rasterize_skinned_gaussians(
        xyz, Rc, sc, op, sh, t(s["w"]), A, _skin_settings(s, dev), smpl_scale=t(s["smpl_scale"]), transl=tr, return_posed=True,
        means2D=m2d, return_aux=True)
    o, oa = _oracle_pair(pxyz.detach().cpu().numpy(), s["opac"], cam["world_view_transform"], cam["full_proj_transform"],
                         cam["camera_center"], Wd, Hd, math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"],
                         psc.cpu().numpy(), pq.detach().cpu().numpy(), s["shs"], 3)
    if which == "long_lists":
        tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
        assert tl.max() > 8192, tl.max()                       # long rows, sparse backward over many depth segments
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    strict = _check_maps(o, oa, depth, alpha)
    rng = np.random.RandomState(17)
    dLc = s["dL"].copy(); dLc[:, ~strict] = 0
    gD = rng.normal(0, 1, (Hd, Wd)).astype(np.float32); gD[~strict] = 0
    gA = rng.normal(0, 1, (Hd, Wd)).astype(np.float32); gA[~strict] = 0
    ((color * t(dLc)).sum() + (depth[0] * t(gD)).sum() + (alpha[0] * t(gA)).sum()).backward()
    ref = _reference_grads(o, oa, dLc, gD, gA, cam["world_view_transform"])
    # LBS^T reference: torch autograd through the restatement, seeded with the posed-space gradients
    T = lambda a: torch.from_numpy(a).clone().requires_grad_(True)
    oxyz, oRc, osc, oA, otr = T(s["xyz"]), T(s["Rc"]), T(s["scales"]), T(s["A"]), T(s["transl"])
    pxyz_o, pq_o, psc_o, _ = lo.deform_gaussians(oxyz, oRc, osc, torch.from_numpy(s["w"]), oA,
                                                 smpl_scale=torch.from_numpy(s["smpl_scale"]), transl=otr)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    ((pxyz_o * f(ref["means3D"])).sum() + (pq_o * f(ref["rotations"])).sum() + (psc_o * f(ref["scales"])).sum()).backward()
    _grad_close("xyz_canon", xyz.grad.cpu().numpy(), oxyz.grad.numpy(), atol=1e-5)
    _grad_close("rotmat_canon", Rc.grad.cpu().numpy(), oRc.grad.numpy(), atol=1e-5)
    _grad_close("scales", sc.grad.cpu().numpy(), osc.grad.numpy(), atol=1e-5)
    _grad_close("opacity", op.grad.cpu().numpy(), ref["opacities"])
    _grad_close("sh", sh.grad.cpu().numpy(), ref["shs"])
    _grad_close("viewspace", m2d.grad.cpu().numpy(), ref["means2D"])
    _grad_close("A", A.grad.cpu().numpy()[:, :3, :], oA.grad.numpy()[:, :3, :], rtol=2e-3, atol=2e-4)
    _grad_close("transl", tr.grad.cpu().numpy(), otr.grad.numpy(), rtol=2e-3, atol=2e-4)


def test_get_render_pkg_fused_carries_the_maps():
    from sings_amd.renderer import get_render_pkg_fused
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = _dev()
    s = _skin_scene(5000, 24, 21)
    t = lambda a: torch.from_numpy(a).to(dev)
    canon = dict(xyz_canon=t(s["xyz"]), rotmat_canon=t(s["Rc"]), scales=t(s["scales"]), opacity=t(s["opac"]), shs=t(s["shs"]),
                 lbs_weights=t(s["w"]), active_sh_degree=3)
    data = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in s["cam"].items()}
    with torch.no_grad():
        pkg = get_render_pkg_fused(data, canon, t(s["A"]), t(s["bg"]), smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]),
                                   return_aux=True)
        out = rasterize_skinned_gaussians(canon["xyz_canon"], canon["rotmat_canon"], canon["scales"], canon["opacity"], canon["shs"],
                                          canon["lbs_weights"], t(s["A"]), _skin_settings(s, dev), smpl_scale=t(s["smpl_scale"]),
                                          transl=t(s["transl"]), return_aux=True)
    assert torch.equal(pkg["render_raw"], out[0]) and torch.equal(pkg["depth"], out[2]) and torch.equal(pkg["alpha"], out[3])
    assert tuple(pkg["alpha"].shape) == (1, s["H"], s["W"]) and float(pkg["alpha"].max()) > 0.5
