"""Several avatars in one frame through the fused K-frame forward (include/sings_scene.h: ``SceneFramesEngine``, ``SceneAnimator``).

The bar, bit for bit: a scene of ONE avatar is ``SkinnedFramesEngine``'s forward; in a scene of several, segment s of the posed
outputs and of the radii is avatar s's own ``SkinnedFramesEngine`` forward, and the image, the radii, the pair counts and the maps
are the plain rasterizer's for the concatenated posed sets -- what the reference's gs_renderer_multiple.py computes.  That the fused
preprocess equals the plain raster of its own posed output was confirmed on the MI355X for all three rotation formats (isotropic,
6-D, 3x3 matrices) with per-frame ext_tfs before these tests were written (``test_get_render_pkg_fused_matches_unfused`` covers
the isotropic case), so every format is held to equality here, none to a measured difference.

The avatars stand where ``scene.avatar_scene`` puts them (10 m in front of an identity camera) and are seen through a 600-pixel
focal length -- the whole body in a 160 x 288 image -- with scales enlarged so that a few hundred Gaussians cover the body."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 16


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _cameras(W, H, K, focal=600.0, per_frame=True):
    """K camera dicts (``render``'s keys): one shared dict K times, or K cameras shifted along x."""
    from sings_amd.camera import make_camera
    cam = make_camera(np.eye(4, dtype=np.float32), focal, focal, W / 2, H / 2, W, H)
    P_T = np.linalg.inv(cam["world_view_transform"]) @ cam["full_proj_transform"]
    out = []
    for f in range(K if per_frame else 1):
        view = cam["world_view_transform"].copy()
        view[3, 0] += 0.02 * f
        out.append(dict(fovx=cam["fovx"], fovy=cam["fovy"], image_height=H, image_width=W, world_view_transform=_t(view),
                        full_proj_transform=_t((view @ P_T).astype(np.float32)),
                        camera_center=_t(np.linalg.inv(view)[3, :3].astype(np.float32))))
    return out if per_frame else out * K


def _settings(cams, bg):
    """(one settings per frame, the K-frame settings) of K camera dicts."""
    from sings_amd.posed import _stack_cameras
    from sings_amd.renderer import _settings as one
    return [one(c, bg, 1.0, 0) for c in cams], _stack_cameras(list(cams), len(cams), bg, 1.0, 0)


def _placements(K, center, seed, scale=1.0, spread=0.05):
    """K placements (trans [K,3], rotmat [K,3,3], scale [K,1]) that turn and scale an avatar about ``center``."""
    from sings_amd.body import rodrigues
    rs = np.random.RandomState(seed)
    R = rodrigues(torch.from_numpy(rs.normal(0, 0.15, (K, 3)).astype(np.float32))).to(_dev()).contiguous()
    e = _t((scale * (1.0 + spread * rs.uniform(-1, 1, (K, 1)))).astype(np.float32))
    c = torch.as_tensor(center, dtype=torch.float32, device=_dev())
    return (c[None] - e * (R @ c[None, :, None])[..., 0]).contiguous(), R, e


def _avatar(P, J, rot, seed, K, smpl_scale="frames", ext="frames", scale_mul=8.0, offset=(0.0, 0.0, 0.0)):
    """An avatar of P Gaussians and J joints (23: the 24-joint body with its last joint folded into the one before) ->
    dict(canon=, A [K,J,16], transl [K,3], smpl_scale, ext_tfs, J, rw).  ``rot``: None (isotropic), 6 or 9; ``smpl_scale`` / ``ext``:
    None, "shared" or "frames"."""
    from sings_amd.body import joint_transforms, rodrigues
    from sings_amd.scene import avatar_scene
    Jb = 24 if J == 23 else J
    s = avatar_scene(N=P, J=Jb, W=160, H=288, seed=seed, isotropic=rot is None)
    rs = np.random.RandomState(seed + 1000)
    w = s["lbs_weights"]
    if J == 23:
        w = w[:, :23].copy()
        w[:, 22] += s["lbs_weights"][:, 23]
    jr = _t(s["joints_rest"])
    A = torch.stack([joint_transforms(_t(rs.normal(0, 0.2, Jb * 3).astype(np.float32)), jr, tuple(s["parents"])).reshape(Jb, 16)[:J]
                     for _ in range(K)]).contiguous()
    transl = _t((s["transl"][None] + np.asarray(offset)[None] + rs.normal(0, 0.03, (K, 3))).astype(np.float32))
    rotmat = None
    if rot == 6:
        rotmat = _t(rs.normal(size=(P, 6)).astype(np.float32))
    elif rot == 9:
        rotmat = rodrigues(torch.from_numpy(rs.normal(0, 1.0, (P, 3)).astype(np.float32))).to(_dev()).contiguous()
    canon = dict(xyz_canon=_t(s["xyz_canon"]), rotmat_canon=rotmat, scales=_t(s["scales"] * np.float32(scale_mul)),
                 opacity=_t(s["opacities"]), shs=_t(s["shs"]), lbs_weights=_t(w), active_sh_degree=0)
    sc = {None: None, "shared": _t(np.array([1.04], np.float32)),
          "frames": _t(np.linspace(0.93, 1.07, K, dtype=np.float32)[:, None])}[smpl_scale]
    center = [0.0, 0.0, float(s["transl"][2] + s["xyz_canon"][:, 2].mean())]
    e = None
    if ext == "frames":
        e = _placements(K, center, seed)
    elif ext == "shared":
        e = tuple(x[0] for x in _placements(1, center, seed))
    return dict(canon=canon, A=A, transl=transl, smpl_scale=sc, ext_tfs=e, J=J, rw=rot, P=P)


def _frames(avatars):
    return [dict(canon=a["canon"], A=a["A"], transl=a["transl"], smpl_scale=a["smpl_scale"], ext_tfs=a["ext_tfs"]) for a in avatars]


def _alone(a, W, H, K, stacked, cap, aux=False):
    """Avatar ``a`` through its own SkinnedFramesEngine -> (color, radii, (xyz, q, scales) [K,P,...], counts, alpha | None)."""
    from sings_amd.engine import SkinnedFramesEngine
    c = a["canon"]
    eng = SkinnedFramesEngine(a["P"], a["J"], W, H, M, K, _dev(), cap, with_rot=a["rw"] is not None, rot_width=a["rw"] or 9, aux=aux)
    eng.set_camera(stacked)
    eng.set_frames(c["xyz_canon"], c["rotmat_canon"], c["lbs_weights"], a["A"], a["smpl_scale"], a["transl"], a["ext_tfs"])
    posed = tuple(torch.empty(K, a["P"], w, device=_dev()) for w in (3, 4, 3))
    Rs = eng.forward(c["shs"], c["opacity"], c["scales"], sync_num_rendered=True, posed_out=posed)
    torch.cuda.synchronize()
    return eng.color.clone(), eng.radii.clone(), posed, Rs, eng.alpha.clone() if aux else None


def _plain(avatars, posed, one, W, H, cap, short_lists=False):
    """The reference's way, frame by frame: the posed sets concatenated (SH block included) and rasterized once ->
    [(color, radii, R)]."""
    from sings_amd.engine import RasterEngine
    Ptot = sum(a["P"] for a in avatars)
    eng = RasterEngine(Ptot, W, H, M, _dev(), cap)
    shs = torch.cat([a["canon"]["shs"] for a in avatars]).contiguous()
    op = torch.cat([a["canon"]["opacity"] for a in avatars]).contiguous()
    out = []
    for f, rs in enumerate(one):
        xyz, q, sc = (torch.cat([p[n][f] for p in posed]).contiguous() for n in range(3))
        eng.set_camera(rs, short_lists=short_lists)
        R = eng.forward(xyz, shs, op, sc, q, sync_num_rendered=True)
        torch.cuda.synchronize()
        out.append((eng.color.clone(), eng.radii.clone(), R))
    return out


def _scene(avatars, W, H, K, stacked, cap, aux=False, **hints):
    from sings_amd.scene_anim import SceneFramesEngine
    eng = SceneFramesEngine([(a["P"], a["J"], a["rw"]) for a in avatars], W, H, M, K, _dev(), cap, aux=aux)
    eng.set_camera(stacked, **hints)
    eng.set_frames(_frames(avatars))
    posed = tuple(torch.empty(K, eng.P, w, device=_dev()) for w in (3, 4, 3))
    Rs = eng.forward(sync_num_rendered=True, posed_out=posed)
    torch.cuda.synchronize()
    return eng, posed, Rs


def _check_against_the_parts(avatars, W, H, K, cams, cap, **hints):
    """The equalities of a scene: posed segments and radii = every avatar's own forward, image / radii / counts = the plain raster
    of the concatenated posed sets.  -> (engine, the avatars' own results)."""
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    one, stacked = _settings(cams, bg)
    eng, posed, Rs = _scene(avatars, W, H, K, stacked, cap, **hints)
    own = [_alone(a, W, H, K, stacked, cap, aux=True) for a in avatars]
    assert eng.starts == [sum(a["P"] for a in avatars[:s]) for s in range(len(avatars))]
    for s, (a, o) in enumerate(zip(avatars, own)):
        lo, hi = eng.starts[s], eng.starts[s] + a["P"]
        for n in range(3):
            assert torch.equal(posed[n][:, lo:hi], o[2][n]), (s, n)
        assert torch.equal(eng.radii_of(s), eng.radii[:, lo:hi]) and eng.radii_of(s).shape == (K, a["P"])
        assert torch.equal(eng.radii_of(s), o[1]), s
        assert int((o[1] > 0).sum()) > 0, s                                      # (every avatar is in view)
    ref = _plain(avatars, [o[2] for o in own], one, W, H, cap, short_lists=bool(hints.get("short_lists")))
    for f, (color, radii, R) in enumerate(ref):
        assert 0 < R <= cap and Rs[f] == R, (f, Rs[f], R)
        assert torch.equal(eng.radii[f], radii), f
        assert torch.equal(eng.color[f], color), f
    assert not torch.equal(eng.color[0], eng.color[K - 1])
    return eng, own


# ---- 1. a scene of one avatar is the existing path --------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
def test_a_scene_of_one_avatar_is_the_skinned_k_frame_forward_bit_for_bit(K):
    P, J, W, H, cap = 5037, 52, 160, 288, 1 << 18
    a = _avatar(P, J, 6, 11 + K, K)
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    one, stacked = _settings(_cameras(W, H, K), bg)
    color, radii, posed, Rs, _ = _alone(a, W, H, K, stacked, cap)
    eng, got, got_Rs = _scene([a], W, H, K, stacked, cap)
    assert all(0 < r <= cap for r in Rs) and got_Rs == Rs
    assert float((color < 0.99).float().mean()) > 0.01                           # the avatar is in view
    assert torch.equal(eng.color, color) and torch.equal(eng.radii, radii)
    for n in range(3):
        assert torch.equal(got[n], posed[n]), n
    assert eng.starts == [0] and torch.equal(eng.radii_of(0), radii) and eng.num_rendered() == Rs
    for fn in (eng.backward, eng.backward_records, eng.backward_gaussians):
        with pytest.raises(RuntimeError, match="forward-only"):
            fn(None)


# ---- 2. a mixed scene -------------------------------------------------------------------------------------------------------------
def _mixed(K):
    return [_avatar(3001, 24, None, 3, K, smpl_scale=None, ext="frames"),
            _avatar(257, 52, 6, 4, K, smpl_scale="frames", ext="frames", offset=(0.05, 0.0, 0.1)),
            _avatar(40, 23, 9, 5, K, smpl_scale="shared", ext=None, offset=(-0.05, 0.1, -0.1))]


def test_a_mixed_scene_is_its_avatars_posed_alone_and_rasterized_together():
    """Blocks: 12 + 2 + 1; the last block of avatar 0 holds 185 Gaussians (three live waves, one of them partly), avatar 1's second
    block ONE Gaussian (three wholly dead waves), avatar 2's only block 40."""
    W, H, K = 160, 288, 3
    avatars = _mixed(K)
    eng, own = _check_against_the_parts(avatars, W, H, K, _cameras(W, H, K), 1 << 18)
    solid = torch.stack([o[4] > 0.5 for o in own]).sum(0)                         # [K,1,H,W]: avatars that are solid there on their own
    assert int((solid >= 2).sum()) > 0, "the avatars do not overlap on screen"


# ---- 3. many tiles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short_lists", [False, True])
def test_a_scene_on_a_frame_of_many_tiles(short_lists):
    """1056 x 1056: 66 x 66 = 4356 tiles, 68 x 68 counter words > SG_HIST_TILES_MAX: no whole-image histogram, and with the
    short-lists hint direct binning."""
    from sings_amd import _lib
    W = H = 1056
    assert ((W + 15) // 16) ** 2 == 4356 and (((W + 15) // 16 + 3) // 4 * 4) ** 2 > _lib.HIST_TILES_MAX
    K = 2
    avatars = [_avatar(3000, 52, 6, 7, K, scale_mul=3.0),
               _avatar(777, 24, None, 8, K, smpl_scale=None, ext="shared", scale_mul=3.0, offset=(0.1, 0.0, 0.0))]
    eng, _ = _check_against_the_parts(avatars, W, H, K, _cameras(W, H, K, focal=2000.0), 1 << 19, short_lists=short_lists)
    assert eng._rows == (_lib.FLAG_SHORT_LISTS if short_lists else 0)


# ---- 4. the maps ------------------------------------------------------------------------------------------------------------------
def test_depth_and_alpha_of_a_scene():
    from sings_amd.rasterizer import GaussianRasterizer
    W, H, K, cap = 160, 288, 2, 1 << 18
    avatars = [_avatar(2000, 52, 6, 21, K), _avatar(300, 24, None, 22, K, smpl_scale=None, ext=None, offset=(0.05, 0.0, 0.1))]
    cams = _cameras(W, H, K)
    bg = _t(np.array([0.2, 0.9, 0.5], np.float32))
    one, stacked = _settings(cams, bg)
    eng, posed, Rs = _scene(avatars, W, H, K, stacked, cap, aux=True)
    plain, _, _ = _scene(avatars, W, H, K, stacked, cap)
    assert torch.equal(eng.color, plain.color) and torch.equal(eng.radii, plain.radii)
    shs = torch.cat([a["canon"]["shs"] for a in avatars]).contiguous()
    op = torch.cat([a["canon"]["opacity"] for a in avatars]).contiguous()
    with torch.no_grad():
        for f in range(K):
            color, radii, depth, alpha = GaussianRasterizer(one[f]).forward_aux(
                means3D=posed[0][f], means2D=torch.zeros_like(posed[0][f]), opacities=op, shs=shs, scales=posed[2][f], rotations=posed[1][f])
            assert torch.equal(eng.color[f], color) and torch.equal(eng.radii[f], radii), f
            assert torch.equal(eng.depth[f], depth) and torch.equal(eng.alpha[f], alpha), f
    assert float(eng.alpha.max()) > 0.5 and float(eng.depth.max()) > 5.0
    # colour = sum_i c_i alpha_i T_i + (1 - alpha) bg: the sum is the image over a black background.  In fp32 the kernel adds T bg
    # and stores alpha = 1 - T, so (1 - alpha) is T to 2^-24 (two roundings of values <= 1), bg <= 1, and the product, the sum and
    # the kernel's own sum round once each at the image's magnitude v: half an ulp, <= 2^-24 v, each.
    _, black = _settings(cams, torch.zeros(3, device=_dev()))
    base, _, _ = _scene(avatars, W, H, K, black, cap)
    want = base.color + (1.0 - eng.alpha) * bg[None, :, None, None]
    tol = 2.0 ** -24 * (1.0 + 3.0 * max(1.0, float(eng.color.abs().max())))
    err = float((eng.color - want).abs().max())
    print("colour = sum + (1 - alpha) bg: max error", err, "bound", tol)
    assert err <= tol, (err, tol)


# ---- 5. a degenerate avatar -------------------------------------------------------------------------------------------------------
def test_an_avatar_whose_joints_are_nan_in_one_frame_is_absent_from_that_frame_only():
    W, H, K, cap = 160, 288, 3, 1 << 18
    avatars = _mixed(K)
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    _, stacked = _settings(_cameras(W, H, K), bg)
    good, _, good_Rs = _scene(avatars, W, H, K, stacked, cap)
    without, _, without_Rs = _scene([avatars[0], avatars[2]], W, H, K, stacked, cap)
    bad_A = avatars[1]["A"].clone()
    bad_A[1] = float("nan")
    bad, _, bad_Rs = _scene([avatars[0], dict(avatars[1], A=bad_A), avatars[2]], W, H, K, stacked, cap)
    assert int((good.radii_of(1)[1] > 0).sum()) > 0 and not torch.equal(good.color[1], without.color[1])
    assert int((bad.radii_of(1)[1] != 0).sum()) == 0
    assert torch.equal(bad.color[1], without.color[1]) and bad_Rs[1] == without_Rs[1]
    assert torch.equal(bad.radii_of(0)[1], without.radii_of(0)[1]) and torch.equal(bad.radii_of(2)[1], without.radii_of(1)[1])
    for f in (0, 2):
        assert torch.equal(bad.color[f], good.color[f]) and torch.equal(bad.radii[f], good.radii[f]) and bad_Rs[f] == good_Rs[f], f


# ---- 6. the animator --------------------------------------------------------------------------------------------------------------
def _per_frame_plain(avatars, cams, bg, F, W, H, cap):
    """The per-frame plain path: every avatar posed on its own, one frame per launch, the posed sets concatenated and rasterized
    -> F clamped images."""
    from sings_amd.engine import RasterEngine, SkinnedEngine
    from sings_amd.renderer import _settings as one
    posers = [SkinnedEngine(a["P"], a["J"], W, H, M, _dev(), cap, with_rot=a["rw"] is not None, rot_width=a["rw"] or 9) for a in avatars]
    raster = RasterEngine(sum(a["P"] for a in avatars), W, H, M, _dev(), cap)
    shs = torch.cat([a["canon"]["shs"] for a in avatars]).contiguous()
    op = torch.cat([a["canon"]["opacity"] for a in avatars]).contiguous()
    out = []
    for f in range(F):
        rs = one(cams[f], bg, 1.0, 0)
        posed = []
        for a, e in zip(avatars, posers):
            c = a["canon"]
            p = tuple(torch.empty(a["P"], w, device=_dev()) for w in (3, 4, 3))
            e.set_camera(rs)
            e.set_frame(c["xyz_canon"], c["rotmat_canon"], c["lbs_weights"], a["A"][f], None if a["smpl_scale"] is None else a["smpl_scale"][f],
                        a["transl"][f], None if a["ext_tfs"] is None else tuple(x[f] for x in a["ext_tfs"]))
            e.forward(c["shs"], c["opacity"], c["scales"], posed_out=p)
            posed.append(p)
        raster.set_camera(rs)
        xyz, q, sc = (torch.cat([p[n] for p in posed]).contiguous() for n in range(3))
        R = raster.forward(xyz, shs, op, sc, q, sync_num_rendered=True)
        assert 0 < R <= cap, (f, R)
        out.append(torch.clamp(raster.color, 0.0, 1.0))
    return out


def _jobs(avatars, cams, F):
    return [(cams[f], [(a["A"][f].reshape(a["J"], 4, 4), a["transl"][f], None if a["smpl_scale"] is None else a["smpl_scale"][f],
                        None if a["ext_tfs"] is None else tuple(x[f] for x in a["ext_tfs"])) for a in avatars]) for f in range(F)]


def _expanded(a, F):
    """``a`` with ONE placement handed over as the reference's ``.expand`` views [F,...] (AnimDataset_opt.get_chunk)."""
    ext = tuple(x[:1].expand(F, *x.shape[1:]) for x in a["ext_tfs"])
    assert all(x.stride(0) == 0 for x in ext)
    return dict(a, ext_tfs=ext)


@pytest.mark.parametrize("per_frame_cameras", [False, True])
def test_the_animator_renders_the_per_frame_plain_paths_images_in_order(per_frame_cameras):
    from sings_amd.posed import frames_to_u8
    from sings_amd.scene_anim import SceneAnimator
    W, H, F, K = 160, 288, 11, 4
    avatars = [_expanded(_avatar(1500, 52, 6, 31, F), F), _avatar(400, 24, None, 32, F, smpl_scale=None, ext=None, offset=(0.05, 0.0, 0.1))]
    cams = _cameras(W, H, F, per_frame=per_frame_cameras)
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    want = _per_frame_plain(avatars, cams, bg, F, W, H, 1 << 18)
    assert not torch.equal(want[0], want[F - 1]) and float((want[0] < 0.99).float().mean()) > 0.01
    fa = SceneAnimator([a["canon"] for a in avatars], streams=2)
    got = list(fa.render_frames_batched(iter(_jobs(avatars, cams, F)), bg, frames_per_launch=K))
    torch.cuda.synchronize()
    assert [i for i, _ in got] == list(range(F))                                  # three launches of 4, 4 and 3 (padded) frames, in order
    assert fa.key[4] == K and len(fa.engs) == 2 and fa.engs[0]._cam_stride == int(per_frame_cameras)
    for f, img in got:
        assert torch.equal(img, want[f]), f
    got8 = dict(fa.render_frames_batched(iter(_jobs(avatars, cams, F)), bg, frames_per_launch=K, out="bgr8"))
    torch.cuda.synchronize()
    for f in range(F):
        assert got8[f].dtype == torch.uint8 and tuple(got8[f].shape) == (H, W, 3)
        assert torch.equal(got8[f], frames_to_u8(want[f], bgr=True)), f


def test_animate_scene_takes_per_avatar_lists():
    from sings_amd.body import joint_transforms
    from sings_amd.scene import avatar_scene
    from sings_amd.scene_anim import animate_scene
    W, H, F = 160, 288, 5
    avatars = [_avatar(600, 52, 6, 41, F, ext=None), _avatar(200, 24, None, 42, F, smpl_scale=None, ext="frames", offset=(0.05, 0.0, 0.1))]
    cams = _cameras(W, H, F)
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    from sings_amd.posed import joint_transforms_batch
    rs = np.random.RandomState(9)
    poses, rest, cano, parents = [], [], [], []
    for a, seed in zip(avatars, (41, 42)):
        s = avatar_scene(N=8, J=a["J"], W=W, H=H, seed=seed)
        jr = _t(s["joints_rest"])
        poses.append(_t(rs.normal(0, 0.2, (F, a["J"] * 3)).astype(np.float32)))
        rest.append(jr); parents.append(tuple(s["parents"]))
        cano.append(joint_transforms(_t(rs.normal(0, 0.05, a["J"] * 3).astype(np.float32)), jr, parents[-1]))
        # (the joint transforms as animate_scene derives them from the poses: the per-frame plain path below is given the same)
        a["A"] = (joint_transforms_batch(poses[-1], jr, parents[-1]) @ torch.inverse(cano[-1])[None]).reshape(F, a["J"], 16).contiguous()
    want = _per_frame_plain(avatars, cams, bg, F, W, H, 1 << 18)
    got = dict(animate_scene([a["canon"] for a in avatars], poses, rest, cano, cams, bg, transl=[a["transl"] for a in avatars],
                             smpl_scale=[a["smpl_scale"] for a in avatars], ext_tfs=[a["ext_tfs"] for a in avatars], parents=parents,
                             frames_per_launch=2))
    torch.cuda.synchronize()
    assert sorted(got) == list(range(F))
    for f in range(F):
        assert torch.equal(got[f], want[f]), f


def test_a_refused_long_rows_hint_is_dropped_and_the_batch_rendered_again():
    """A placement scale of ~0.01 puts each avatar's 10 000 Gaussians on the four tiles around the image centre: lists of 20 000
    entries, beyond the 16 384 of SG_FLAG_LONG_ROWS.  The optimistic batch is refused on the device and rendered again."""
    from sings_amd.scene_anim import SceneAnimator
    W, H, F, K = 160, 288, 3, 4
    avatars = [_avatar(10000, 52, None, 51, F, scale_mul=1.0), _avatar(10000, 24, None, 52, F, smpl_scale=None, scale_mul=1.0)]
    for a, seed in zip(avatars, (51, 52)):
        a["ext_tfs"] = _placements(F, [0.0, 0.0, 10.0], seed, scale=0.01, spread=0.2)
    cams = _cameras(W, H, F, per_frame=False)
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    want = _per_frame_plain(avatars, cams, bg, F, W, H, 1 << 19)
    assert not any(torch.equal(w, torch.ones_like(w)) for w in want)
    fa = SceneAnimator([a["canon"] for a in avatars], streams=2)
    assert fa.long_rows is True
    got = dict(fa.render_frames_batched(iter(_jobs(avatars, cams, F)), bg, frames_per_launch=K))
    torch.cuda.synchronize()
    assert fa.long_rows is False and sorted(got) == list(range(F))
    for f in range(F):
        assert torch.equal(got[f], want[f]), f


def test_an_overflowing_batch_is_rendered_again_on_grown_engines_and_one_that_still_overflows_raises(monkeypatch):
    """Gaussians of ~10 pixels sigma (scales x 28): ~20 tiles each, beyond the animator's first capacity of 8 pairs per Gaussian."""
    from sings_amd.overflow import EngineCapacity
    from sings_amd.scene_anim import SceneAnimator
    W, H, F, K = 160, 288, 5, 4
    avatars = [_avatar(4000, 52, 6, 61, F, scale_mul=28.0), _avatar(4000, 24, None, 62, F, smpl_scale=None, ext=None, scale_mul=28.0)]
    cams = _cameras(W, H, F)
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    floor = EngineCapacity.floor(0, 8000, W, H)
    want = _per_frame_plain(avatars, cams, bg, F, W, H, 1 << 21)
    fa = SceneAnimator([a["canon"] for a in avatars], streams=2)
    got = dict(fa.render_frames_batched(iter(_jobs(avatars, cams, F)), bg, frames_per_launch=K))
    torch.cuda.synchronize()
    assert fa.cap > floor, (fa.cap, floor)                                       # (the overflow re-render ran)
    assert sorted(got) == list(range(F))
    for f in range(F):
        assert torch.equal(got[f], want[f]), f
    # a capacity rule that never grows enough: hint kept or dropped, the batch overflows twice more and the animator gives up
    monkeypatch.setattr(EngineCapacity, "grown", staticmethod(lambda need: floor + 1024))
    fb = SceneAnimator([a["canon"] for a in avatars], streams=2)
    with pytest.raises(RuntimeError, match="after two re-renders"):
        list(fb.render_frames_batched(iter(_jobs(avatars, cams, F)), bg, frames_per_launch=K))
    torch.cuda.synchronize()
