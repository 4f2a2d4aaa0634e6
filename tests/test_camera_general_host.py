"""CPU anchors of the general-camera tests (tests/camera_case.py): the references the GPU file compares with are themselves only
ever held against each other on identity-view scenes, so under rotated / off-origin / fx != fy / off-centre cameras they are
anchored here first, from the fp64 C oracle alone:

 * equivariance -- the world-space scene through extrinsic E == the E-moved scene through the identity camera (fp64 round-off);
 * the C restatement against its autograd twin, per camera;
 * finite differences of the explicit backward (and, for fov-clamped splats, proof that the frozen coordinate is NOT the
   derivative: a kernel that differentiated through the clamp would be caught);
 * the SH direction with campos != 0 against the reference-generated golden G9;
 * mutated cameras (view rotation transposed, tanfovx / tanfovy exchanged, campos zeroed, principal point centred) move the result
   by >= 100 x the GPU tolerances: the inputs discriminate the mistakes they are meant to catch;
 * the conditions every GPU scene relies on (borderline share, visible share, populated clamp groups).
"""
import numpy as np
import pytest
import torch

import camera_case as cc
import sh_case
from oracle import raster_oracle as ro
from oracle import raster_torch as rt

# the GPU tolerances the power checks are scaled by: tests/test_gpu_raster.py RGB_TOL and _grad_close(rtol, atol)
RGB_TOL, G_RTOL, G_ATOL = 1e-5, 2e-4, 2e-6
BORDER = 2e-5


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _run64(s, view, proj, campos, means=None, rots=None, deg=None, tanfov=None, want_margin=True, scale_modifier=1.0):
    f = lambda a: np.asarray(a, np.float64)
    tx, ty = tanfov or (s["tanfovx"], s["tanfovy"])
    return ro.forward(f(s["means3D"]) if means is None else means, f(s["opacities"]), view, proj, campos, s["W"], s["H"], tx, ty,
                      f(s["bg"]), scales=f(s["scales"]), rotations=f(s["rotations"]) if rots is None else rots, shs=f(s["shs"]),
                      sh_degree=s["sh_degree"] if deg is None else deg, dtype=np.float64, want_margin=want_margin,
                      scale_modifier=scale_modifier)


def test_camera_family_is_what_it_says():
    cams = cc.cameras(128, 96)
    assert tuple(cams) == cc.NAMES
    for name, c in cams.items():
        R = c["extrinsic"][:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6, name      # (orbit: fp32 rotations)
        assert np.array_equal(c["world_view_transform"], c["extrinsic"].T.astype(np.float32))
        assert np.array_equal(c["full_proj_transform"], (c["world_view_transform"] @ c["P"].T.astype(np.float32)).astype(np.float32))
        assert np.abs(c["camera_center"] + R.T @ c["extrinsic"][:3, 3]).max() < 1e-5
        if name != "identity":
            assert np.abs(R - np.eye(3)).max() > 0.3 and np.abs(c["camera_center"]).max() > 0.3, name
    g, o = cams["generic"], cams["offcentre"]
    assert abs(g["fy"] / g["fx"] - 1.2) < 1e-12 and abs(g["tanfovx"] * 96 / (g["tanfovy"] * 128) - 1.2) < 1e-9
    assert (o["cx"], o["cy"]) == (64 + 7.5, 48 - 4.25) and np.array_equal(o["world_view_transform"], g["world_view_transform"])
    assert abs(o["P"][0, 2] - 2 * 7.5 / 128) < 1e-6 and abs(o["P"][1, 2] + 2 * 4.25 / 96) < 1e-6 and g["P"][0, 2] == 0 == g["P"][1, 2]
    # roll exchanges the roles of x and y: each view axis lies (mostly) along the other world axis
    Rr = cams["roll"]["extrinsic"][:3, :3]
    assert abs(Rr[0, 1]) > 0.98 and abs(Rr[1, 0]) > 0.98
    # the orbit cameras are the production ones
    from sings_amd.camera import get_rotating_camera
    orbit = get_rotating_camera(img_size=(96, 128), device="cpu", nframes=5)
    for i in (1, 3):
        c = cams[f"orbit{i}"]
        # (the producer's matrix inverse leaves 1e-16 in the last column; the extrinsic here has exact zeros there)
        assert np.abs(c["world_view_transform"] - orbit[i]["world_view_transform"].numpy()).max() < 1e-12
        assert np.abs(c["full_proj_transform"] - orbit[i]["full_proj_transform"].numpy()).max() < 1e-5
        assert abs(c["tanfovx"] - np.tan(0.2)) < 1e-12 and abs(c["tanfovy"] - np.tan(0.2)) < 1e-12


@pytest.mark.parametrize("name", cc.GENERAL)
def test_oracle_is_equivariant_under_the_extrinsic(name):
    """fp64: rendering the world-space scene through E equals rendering the E-moved scene (p' = R p + t, q' = q_E (x) q) through
    the identity camera with the same intrinsics.  Degree 0 (SH coefficients do not rotate with the scene) and unit quaternions
    (the un-normalised quaternion-to-matrix map is not equivariant off the unit sphere).  Bounds: fp64 round-off with margin --
    measured 6e-15 (image) to 7e-14 (gradients) on these cases."""
    W, H = 96, 64
    cam = cc.cameras(W, H)[name]
    s = cc.scene(cam, 500, 0, 41, unit_quats=True)
    view, proj, campos = cc.matrices64(cam)
    E = cam["extrinsic"]; R, t = E[:3, :3], E[:3, 3]
    means = s["means3D"].astype(np.float64)
    q = s["rotations"].astype(np.float64); q /= np.linalg.norm(q, axis=1, keepdims=True)
    L = cc.quat_left(cc.rotmat_to_quat(R))
    dL = s["dL_dimage"].astype(np.float64)
    a = _run64(s, view, proj, campos, means=means, rots=q)
    ga = ro.backward(a, dL)
    b = _run64(s, np.eye(4), cam["P"].T.copy(), np.zeros(3), means=means @ R.T + t, rots=q @ L.T)
    gb = ro.backward(b, dL)
    assert (a["radii"] > 0).mean() > 0.5
    for k in ("radii", "rect", "tiles_touched", "keys", "point_list", "ranges", "n_contrib"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["R"] == b["R"]
    assert np.abs(a["color"] - b["color"]).max() <= 1e-12
    assert _rel(ga["dL_dmeans3D"], gb["dL_dmeans3D"] @ R) <= 1e-11           # dL/dp = R^T dL/dp'
    assert _rel(ga["dL_dscales"], gb["dL_dscales"]) <= 1e-11
    assert _rel(ga["dL_dopacity"], gb["dL_dopacity"]) <= 1e-11
    # dL/dq = L(q_E)^T dL/dq' -- for the component TANGENT to the unit sphere.  The oracle differentiates the un-normalised
    # quaternion-to-matrix map R(q) = (1 - |q|^2) I + |q|^2 R(q / |q|), whose radial derivative 2 (R - I) does not commute with
    # the extrinsic (2 (R_E R - I) != R_E 2 (R - I)): the radial component is not equivariant and is left to the twin and the
    # finite differences below.  L is orthogonal, so tangent maps to tangent.
    tang = lambda g_, q_: g_ - (g_ * q_).sum(1, keepdims=True) * q_
    ta, tb = tang(ga["dL_drots"], q), tang(gb["dL_drots"], q @ L.T) @ L
    assert _rel(ta, tb) <= 1e-11 and np.abs(ta).max() > 0.1 * np.abs(ga["dL_drots"]).max()
    assert np.abs(ga["dL_drots"]).max() > 0 and np.abs(ga["dL_dmeans3D"]).max() > 0
    # the clamp groups take part, and keep their flags under the motion
    xo, yo = cc.clamp_flags(cam, s["means3D"])
    assert ((a["radii"] > 0) & xo).sum() >= 32 and ((a["radii"] > 0) & yo).sum() >= 32


@pytest.mark.parametrize("name", cc.NAMES)
def test_c_restatement_and_autograd_twin_agree_per_camera(name):
    """tests/test_oracle_raster_twin.py's comparison (its thresholds: integers equal, images 1e-12, gradients 2e-9) at degree 3 in
    fp64 under every camera, fov-clamped splats and non-unit quaternions included."""
    W, H = 96, 64
    s = cc.scene(cc.cameras(W, H)[name], 500, 3, 42)
    dL = s["dL_dimage"].astype(np.float64)
    o = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"], s["tanfovy"],
                   s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=3, dtype=np.float64)
    g = ro.backward(o, dL)
    t, tg = rt.forward_backward(s, dL, torch.float64)
    vis = o["radii"] > 0
    np.testing.assert_array_equal(t["radii"], o["radii"])
    np.testing.assert_array_equal(t["rect"][vis], o["rect"][vis])
    np.testing.assert_array_equal(t["tiles_touched"], o["tiles_touched"])
    assert t["R"] == o["R"]
    for k in ("keys", "point_list", "ranges", "n_contrib"):
        np.testing.assert_array_equal(t[k], o[k], err_msg=k)
    assert _rel(t["color"], o["color"]) < 1e-12
    assert _rel(t["final_T"].numpy(), o["final_T"]) < 1e-12
    assert _rel(t["xy"].numpy()[vis], o["xy"][vis]) < 1e-13 and _rel(t["rgb"].numpy()[vis], o["rgb"][vis]) < 1e-13
    assert _rel(t["conic"].numpy()[vis], o["conic_opacity"][vis, :3]) < 1e-12
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drots", "dL_dsh"):
        assert _rel(tg[k], g[k].reshape(tg[k].shape)) < 2e-9, (k, _rel(tg[k], g[k].reshape(tg[k].shape)))
    assert _rel(tg["dL_dmean2D"], g["dL_dmean2D"][:, :2]) < 2e-9
    clamped = s["clamp_kind"] >= 0
    assert np.abs(g["dL_dmeans3D"][clamped]).max() > 0


@pytest.mark.parametrize("name", ["generic", "offcentre"])
def test_explicit_backward_matches_fp64_finite_differences_under_a_general_camera(name, monkeypatch):
    """Method and bounds of test_oracle_raster.py::test_explicit_backward_matches_fp64_finite_differences (central differences,
    eps 1e-6, 12 random entries per input, median < 1e-6, worst < 1e-3, scale_modifier 1.3) over the Gaussians the fov clamp leaves
    alone.

    The clamped ones: once t.x / t.z is beyond the limit the forward uses lim * t.z and no longer reads t.x, so in the FROZEN
    coordinate the true derivative of the Jacobian path is zero -- which is what the freeze (x_grad_mul = 0) returns: there the
    explicit backward must AGREE with the finite difference (same bound as above).  What the freeze guards against is the
    un-gated chain-rule term -fx / t.z^2 dL/dJ02: the autograd twin with a straight-through clamp (forward clamped, backward
    as if t.x had been used) carries exactly that term, and must leave the oracle, in the frozen view-space coordinate and
    nowhere else, by more than 100 x the GPU gradient tolerance (2e-4 |g| + 2e-6 max|g|): a kernel without the freeze, or one that
    gates x with the y flag, fails the GPU comparison."""
    W, H = 48, 32
    cam = cc.cameras(W, H)[name]
    s = cc.scene(cam, 60, 3, 7, clamp=(4, 4, 2))
    s["opacities"] = np.minimum(s["opacities"], 0.95)          # the 0.99 alpha clamp is gradient-transparent by design
    names = ["means3D", "opacities", "scales", "rotations", "shs"]
    p = {k: s[k].astype(np.float64) for k in names}
    f = lambda a: np.asarray(a, np.float64)

    def fwd():
        return ro.forward(p["means3D"], p["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"],
                          s["tanfovy"], s["bg"], scales=p["scales"], rotations=p["rotations"], shs=p["shs"], sh_degree=3,
                          dtype=np.float64, scale_modifier=1.3, want_margin=False)
    dL = np.random.RandomState(0).normal(size=(3, H, W))
    o = fwd(); g = ro.backward(o, dL)
    gm = dict(means3D=g["dL_dmeans3D"], opacities=g["dL_dopacity"], scales=g["dL_dscales"], rotations=g["dL_drots"],
              shs=g["dL_dsh"])

    def fd_of(k, i, j, eps=1e-6):
        flat = p[k].reshape(len(p[k]), -1)
        old = flat[i, j]
        flat[i, j] = old + eps; lp = (fwd()["color"] * dL).sum()
        flat[i, j] = old - eps; lm = (fwd()["color"] * dL).sum()
        flat[i, j] = old
        return (lp - lm) / (2 * eps)
    rs = np.random.RandomState(1)
    plain = np.nonzero((o["radii"] > 0) & (s["clamp_kind"] < 0))[0]
    xo, yo = cc.clamp_flags(cam, s["means3D"])
    assert not (xo | yo)[plain].any() and len(plain) > 30
    for k in names:
        errs = []
        for _ in range(12):
            i = rs.choice(plain); j = rs.randint(p[k].reshape(len(p[k]), -1).shape[1])
            fd = fd_of(k, i, j); an = gm[k].reshape(len(p[k]), -1)[i, j]
            if k == "scales":
                an = 1.3 * an      # upstream reports dL/d(scale_modifier * scale) as dL/dscale (no factor: raster_core.inc.c)
            errs.append(abs(fd - an) / (abs(fd) + abs(an) + 1e-7))
        assert np.median(errs) < 1e-6 and max(errs) < 1e-3, (k, errs)
    # the clamped population, in view space (dL/dp_view = R dL/dp_world); frozen coordinate 0 (x) / 1 (y)
    R = cam["extrinsic"][:3, :3]
    scale = np.abs(g["dL_dmeans3D"]).max()
    monkeypatch.setattr(rt, "_clamp_frozen", lambda coord, tz, lim: coord + (torch.clamp(coord / tz, -lim, lim) * tz - coord).detach())
    s64 = dict(s, **{k: p[k] for k in names})
    _, thaw = rt.forward_backward(s64, dL, torch.float64, scale_modifier=1.3)
    monkeypatch.undo()
    an_v = g["dL_dmeans3D"] @ R.T; thaw_v = thaw["dL_dmeans3D"] @ R.T
    ratio = np.abs(thaw_v - an_v) / (G_RTOL * np.abs(an_v) + G_ATOL * scale)
    assert ratio[s["clamp_kind"] < 0].max() < 1e-3                   # the thawed twin is the oracle wherever nothing is clamped
    for kind, coords in ((0, (0,)), (1, (1,)), (2, (0, 1))):
        idx = np.nonzero((s["clamp_kind"] == kind) & (o["radii"] > 0) & (np.abs(g["dL_dmeans3D"]).sum(1) > 0))[0]
        assert len(idx) >= 2, (kind, len(idx))
        for c in coords:
            assert ratio[idx, c].max() > 100, (kind, c, ratio[idx, c])
            for i in idx:
                fd_c = R[c] @ np.array([fd_of("means3D", i, j) for j in range(3)])
                assert abs(fd_c - an_v[i, c]) / (abs(fd_c) + abs(an_v[i, c]) + 1e-7) < 1e-3, (kind, i, c, fd_c, an_v[i, c])
        other = [c for c in range(3) if c not in coords]
        assert ratio[idx][:, other].max() < 1e-3


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_direction_is_mean_minus_campos(deg):
    """The six sh_case groups with Gaussians and camera centre moved by (0.7, -1.1, 0.4): colours and clamp flags of golden G9
    under the criterion of test_oracle_raster.py::test_sh_colour_against_the_reference_spherical_harmonics.  (The shifted fp32
    means round: the direction moves by ~1e-7, inside the 2e-6 of that criterion.)"""
    seen = 0
    for g in cc.shifted_sh_groups():
        assert np.abs(g["campos"]).min() > 0.3 and np.abs(g["viewmatrix"][3, :3]).max() > 0.3
        o = ro.forward(g["means3D"], g["opacities"], g["viewmatrix"], g["projmatrix"], g["campos"], sh_case.W, sh_case.H,
                       sh_case.TANFOV, sh_case.TANFOV, np.zeros(3, np.float32), scales=g["scales"], rotations=g["rotations"],
                       shs=g["shs"], sh_degree=deg)
        assert (o["radii"] > 0).all()
        rgb, clamped = sh_case.expected_rgb(deg, g["idx"])
        assert np.abs(o["rgb"] - rgb).max() <= 2e-6, np.abs(o["rgb"] - rgb).max()
        sure = np.abs(sh_case.G9[f"eval_deg{deg}"][g["idx"]] + 0.5) > 1e-5
        assert np.array_equal(o["clamped"].astype(bool)[sure], clamped[sure])
        seen += g["idx"].size
        if deg == 3:
            # a direction from the mean alone (campos dropped) is told apart by far more than the criterion
            z = ro.forward(g["means3D"], g["opacities"], g["viewmatrix"], g["projmatrix"], np.zeros(3, np.float32), sh_case.W,
                           sh_case.H, sh_case.TANFOV, sh_case.TANFOV, np.zeros(3, np.float32), scales=g["scales"],
                           rotations=g["rotations"], shs=g["shs"], sh_degree=deg)
            assert np.abs(z["rgb"] - rgb).max() > 100 * 2e-6
    assert seen == 512


def _mutants(s, cams):
    view = s["viewmatrix"].copy(); view[:3, :3] = view[:3, :3].T.copy()
    yield "view rotation transposed", dict(viewmatrix=view)
    yield "tanfovx / tanfovy exchanged", dict(tanfovx=s["tanfovy"], tanfovy=s["tanfovx"])
    yield "campos zeroed", dict(campos=np.zeros(3, np.float32))
    if s["cam"]["name"] == "offcentre":
        yield "principal point centred", dict(projmatrix=cams["generic"]["full_proj_transform"])


@pytest.mark.parametrize("name", ["generic", "offcentre"])
def test_mutated_cameras_are_told_apart(name):
    """Each mistake the general cameras are there to catch, made on purpose in the oracle's INPUTS (the view rotation read
    transposed, fx and fy exchanged, the SH direction without the camera centre, and -- under `offcentre` -- a centred principal
    point), moves the fp32 oracle's image and dL/dmeans3D by at least 100 x the tolerances the GPU tests compare them with."""
    case = next(c for c in cc.BACKWARD if c[0] == name)
    _, N, W, H, deg, seed = case
    cams = cc.cameras(W, H)
    s = cc.scene(cams[name], N, deg, seed)

    def run(**kw):
        a = dict(s, **kw)
        o = ro.forward(a["means3D"], a["opacities"], a["viewmatrix"], a["projmatrix"], a["campos"], W, H, a["tanfovx"], a["tanfovy"],
                       a["bg"], scales=a["scales"], rotations=a["rotations"], shs=a["shs"], sh_degree=deg)
        return o, ro.backward(o, s["dL_dimage"])
    o, g = run()
    ref = g["dL_dmeans3D"].astype(np.float64)
    bound = G_RTOL * np.abs(ref) + G_ATOL * np.abs(ref).max()
    seen = 0
    for what, kw in _mutants(s, cams):
        om, gm = run(**kw)
        d_img = np.abs(om["color"] - o["color"]).max()
        d_grad = (np.abs(gm["dL_dmeans3D"] - ref) / bound).max()
        assert d_img >= 100 * RGB_TOL, (what, d_img)
        assert d_grad >= 100, (what, d_grad)
        seen += 1
    assert seen == (4 if name == "offcentre" else 3)


@pytest.mark.parametrize("case", cc.GPU_SCENES, ids=lambda c: "-".join(str(v) for v in c))
def test_conditions_the_gpu_scenes_rely_on(case):
    """From oracle runs alone: few enough borderline pixels for _check_image's cap, more than half of the Gaussians visible, and
    each fov-clamp group populated with splats that are rendered AND carry a gradient (so the GPU comparison of those rows is not
    a comparison of zeros)."""
    name, N, W, H, deg, seed = case
    s = cc.gpu_scene(*case)
    o = ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], W, H, s["tanfovx"], s["tanfovy"],
                   s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=deg)
    border = o["margin"] < BORDER
    assert border.sum() <= 8 + 6e-4 * border.size, (border.sum(), border.size)
    vis = o["radii"] > 0
    assert vis.mean() > 0.5
    dL = s["dL_dimage"].copy(); dL[:, border] = 0
    g = ro.backward(o, dL)
    live = vis & (np.abs(g["dL_dmeans3D"]).sum(1) > 0)
    xo, yo = cc.clamp_flags(s["cam"], s["means3D"])
    kind = s["clamp_kind"]
    assert np.array_equal(kind == 0, xo & ~yo) and np.array_equal(kind == 1, yo & ~xo) and np.array_equal(kind == 2, xo & yo)
    for k, key in ((0, "x"), (1, "y"), (2, "xy")):
        assert (live & (kind == k)).sum() >= cc.CLAMP_MIN[key], (key, (live & (kind == k)).sum())


@pytest.mark.parametrize("name,seed", [("generic", 51), ("roll", 51), ("offcentre", 51), ("generic", 52)])
def test_conditions_the_skinned_gpu_scenes_rely_on(name, seed):
    """The skinned scenes of tests/test_gpu_camera_general.py, posed by the LBS oracle (the GPU tests feed the raster oracle the
    kernel's own posed values, a few ulps away): the body moved to world space by the inverse extrinsic lands in view -- more than
    half of the Gaussians visible -- and more than 99 % of the pixels are clear of the hard thresholds."""
    import test_gpu_camera_general as G
    import test_gpu_skinned as TS
    s = G._skinned_scene(name, seed=seed)
    _, (x, q, sc, _) = TS._oracle_deform(s)
    o = G._skinned_oracle(s, x.numpy(), q.numpy(), sc.numpy())
    assert (o["radii"] > 0).mean() > 0.5 and (o["margin"] >= BORDER).mean() > 0.99
    # and in view space the body sits where the identity-camera scene puts it: 2 m in front of the camera
    tv = cc.to_view(s["cam"], x.numpy())
    assert abs(np.median(tv[:, 2]) - 2.0) < 0.2 and np.abs(np.median(tv[:, :2], 0)).max() < 0.2
