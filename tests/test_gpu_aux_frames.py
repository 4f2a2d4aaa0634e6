"""Depth and alpha maps of K frames per call (``rasterize_skinned_frames(return_aux=True)``, ``get_render_pkgs_fused``,
``SkinnedFramesEngine(aux=True)``, ``FrameAnimator.render_frames_batched``; the ``*_frames_aux`` entry points of include/sings_hip.h).

The bar is the K-frame contract of tests/test_gpu_frames.py extended to the maps: colour, radii, depth and alpha of every frame, and
its dL/dA, dL/dtransl and screen-space gradient, are BIT-IDENTICAL to a single-frame ``rasterize_skinned_gaussians(return_aux=True)``
call; the canonical gradients equal the single-frame gradients summed in frame order.  One case is also held against the raster
oracle's two-pass composition + the LBS oracle, as tests/test_gpu_aux_maps.py holds the single-frame op.
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_aux_maps import _check_maps, _grad_close, _oracle_pair, _reference_grads, _skin_scene
from test_gpu_frames import _avatar

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _leaves(ins, with_rot):
    c = lambda x: x.detach().clone().requires_grad_(True)
    return dict(xyz=c(ins["xyz"]), rot=c(ins["rot"]) if with_rot else None, sc=c(ins["sc"]), op=c(ins["op"]), sh=c(ins["sh"]))


def _map_losses(K, H, W, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    gD = torch.randn(K, 1, H, W, generator=g).to(dev)
    gA = torch.randn(K, 1, H, W, generator=g).to(dev)
    return gD, gA


def _frames_call(ins, A, transl, rs, with_rot, dL, gD, gA, return_aux=True):
    from sings_amd.skinned import rasterize_skinned_frames
    K, N = A.shape[0], ins["xyz"].shape[0]
    lv = _leaves(ins, with_rot)
    Ak, trk = A.clone().requires_grad_(True), transl.clone().requires_grad_(True)
    m2d = torch.zeros(K, N, 3, device=A.device, requires_grad=True)
    out = rasterize_skinned_frames(lv["xyz"], lv["rot"], lv["sc"], lv["op"], lv["sh"], ins["w"], Ak, rs, smpl_scale=ins["smpl_scale"],
                                   transl=trk, means2D=m2d, return_aux=return_aux)
    loss = (out[0] * dL).sum()
    if gD is not None:
        loss = loss + (out[2] * gD).sum()
    if gA is not None:
        loss = loss + (out[3] * gA).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in lv.items() if v is not None}
    return [o.detach() for o in out], grads, Ak.grad, trk.grad, m2d.grad


@pytest.mark.parametrize("K,per_frame_camera,with_rot,N,W,H", [
    (1, False, False, 20000, 160, 288), (3, False, False, 20000, 160, 288), (3, True, True, 20000, 160, 288),
    (8, False, True, 20000, 160, 288), (8, True, False, 20000, 160, 288),
    (3, True, False, 20000, 1280, 1056),                               # many tiles: the dense backward, the plain frames forward
    (8, False, False, 150000, 512, 896)])                              # the cfg4 avatar size, J = 52
def test_frames_maps_and_gradients_equal_single_frame_calls_bit_for_bit(K, per_frame_camera, with_rot, N, W, H):
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = _dev()
    J = 52
    s, ins, A, transl, one, stacked, dL = _avatar(N, J, W, H, 7, K, per_frame_camera, with_rot)
    gD, gA = _map_losses(K, H, W, 5, dev)
    (color, radii, depth, alpha), g, dA, dtr, dm2 = _frames_call(ins, A, transl, stacked, with_rot, dL, gD, gA)
    assert float(alpha.max()) > 0.5 and float(depth.abs().max()) > 0.0
    acc = {}
    for f in range(K):
        lv = _leaves(ins, with_rot)
        A1, tr1 = A[f].clone().requires_grad_(True), transl[f].clone().requires_grad_(True)
        m1 = torch.zeros(N, 3, device=dev, requires_grad=True)
        c1, r1, d1, a1 = rasterize_skinned_gaussians(lv["xyz"], lv["rot"], lv["sc"], lv["op"], lv["sh"], ins["w"], A1, one[f],
                                                     smpl_scale=ins["smpl_scale"], transl=tr1, means2D=m1, return_aux=True)
        ((c1 * dL[f]).sum() + (d1 * gD[f]).sum() + (a1 * gA[f]).sum()).backward()
        torch.cuda.synchronize()
        assert torch.equal(color[f], c1.detach()), f
        assert torch.equal(radii[f], r1), f
        assert torch.equal(depth[f], d1.detach()), f
        assert torch.equal(alpha[f], a1.detach()), f
        assert torch.equal(dA[f], A1.grad), f
        assert torch.equal(dtr[f], tr1.grad), f
        assert torch.equal(dm2[f], m1.grad), f
        for k, v in lv.items():
            if v is not None:
                acc[k] = v.grad.clone() if f == 0 else acc[k] + v.grad    # the single-frame gradients summed in frame order
    for k in acc:
        assert torch.equal(g[k], acc[k]), k


def test_colour_radii_and_colour_gradients_unchanged_by_return_aux():
    dev = _dev()
    N, J, W, H, K = 20000, 52, 160, 288, 8
    s, ins, A, transl, one, stacked, dL = _avatar(N, J, W, H, 11, K, True, True)
    plain, gp, dAp, dtrp, dm2p = _frames_call(ins, A, transl, stacked, True, dL, None, None, return_aux=False)
    aux, ga, dAa, dtra, dm2a = _frames_call(ins, A, transl, stacked, True, dL, None, None, return_aux=True)
    assert torch.equal(plain[0], aux[0]) and torch.equal(plain[1], aux[1])
    for k in gp:
        assert torch.equal(gp[k], ga[k]), k
    assert torch.equal(dAp, dAa) and torch.equal(dtrp, dtra) and torch.equal(dm2p, dm2a)


def test_two_runs_are_bitwise_equal():
    dev = _dev()
    N, J, W, H, K = 20000, 52, 160, 288, 6
    s, ins, A, transl, one, stacked, dL = _avatar(N, J, W, H, 13, K, True, False)
    gD, gA = _map_losses(K, H, W, 9, dev)
    r1 = _frames_call(ins, A, transl, stacked, False, dL, gD, gA)
    r2 = _frames_call(ins, A, transl, stacked, False, dL, gD, gA)
    for a, b in zip(r1[0], r2[0]):
        assert torch.equal(a, b)
    for k in r1[1]:
        assert torch.equal(r1[1][k], r2[1][k]), k
    for a, b in zip(r1[2:], r2[2:]):
        assert torch.equal(a, b)


def test_frames_maps_and_gradients_against_the_oracle():
    """K = 3 few-tile frames, a camera per frame: maps against the raster oracle's two-pass composition, gradients through the
    posed-space reference and the LBS oracle, summed over the frames (the single-frame test's borderline-pixel rule)."""
    from oracle import lbs_oracle as lo
    from sings_amd.camera import make_camera
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.skinned import rasterize_skinned_frames, rasterize_skinned_gaussians
    dev = _dev()
    K = 3
    s = _skin_scene(5000, 24, 31)
    N, Wd, Hd = s["N"], s["W"], s["H"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cams = []
    for f in range(K):
        ext = np.eye(4, dtype=np.float32); ext[0, 3] = 0.015 * f; ext[1, 3] = -0.01 * f
        cams.append(make_camera(ext, 1500.0, 1500.0, Wd / 2, Hd / 2, Wd, Hd))
    rng = np.random.RandomState(3)
    As = np.stack([s["A"] for _ in range(K)]).copy()
    for f in range(1, K):
        As[f, :, :3, 3] += rng.normal(0, 0.01, (s["J"], 3)).astype(np.float32)
    trs = np.stack([s["transl"] + np.array([0.01 * f, -0.005 * f, 0.05 * f], np.float32) for f in range(K)]).astype(np.float32)

    def settings(c):
        return GaussianRasterizationSettings(
            image_height=Hd, image_width=Wd, tanfovx=math.tan(c["fovx"] * 0.5), tanfovy=math.tan(c["fovy"] * 0.5), bg=t(s["bg"]),
            scale_modifier=1.0, viewmatrix=t(c["world_view_transform"]), projmatrix=t(c["full_proj_transform"]), sh_degree=3,
            campos=t(c["camera_center"]), prefiltered=False, debug=False)
    stacked = settings(cams[0])._replace(viewmatrix=t(np.stack([c["world_view_transform"] for c in cams])),
                                         projmatrix=t(np.stack([c["full_proj_transform"] for c in cams])),
                                         campos=t(np.stack([c["camera_center"] for c in cams])))
    req = lambda a: t(a).requires_grad_(True)
    xyz, Rc, sc, op, sh, A, tr = req(s["xyz"]), req(s["Rc"]), req(s["scales"]), req(s["opac"]), req(s["shs"]), req(As), req(trs)
    m2d = torch.zeros(K, N, 3, device=dev, requires_grad=True)
    color, radii, depth, alpha = rasterize_skinned_frames(xyz, Rc, sc, op, sh, t(s["w"]), A, stacked, smpl_scale=t(s["smpl_scale"]),
                                                          transl=tr, means2D=m2d, return_aux=True)
    seeds, refs = [], []
    for f in range(K):
        with torch.no_grad():
            _, _, pxyz, pq, psc = rasterize_skinned_gaussians(t(s["xyz"]), t(s["Rc"]), t(s["scales"]), t(s["opac"]), t(s["shs"]),
                                                              t(s["w"]), t(As[f]), settings(cams[f]), smpl_scale=t(s["smpl_scale"]),
                                                              transl=t(trs[f]), return_posed=True)
        c = cams[f]
        o, oa = _oracle_pair(pxyz.cpu().numpy(), s["opac"], c["world_view_transform"], c["full_proj_transform"], c["camera_center"],
                             Wd, Hd, math.tan(c["fovx"] * 0.5), math.tan(c["fovy"] * 0.5), s["bg"], psc.cpu().numpy(),
                             pq.cpu().numpy(), s["shs"], 3)
        np.testing.assert_array_equal(radii[f].cpu().numpy(), o["radii"])
        strict = _check_maps(o, oa, depth[f], alpha[f])
        dLc = rng.normal(0, 1, (3, Hd, Wd)).astype(np.float32); dLc[:, ~strict] = 0
        gD = rng.normal(0, 1, (Hd, Wd)).astype(np.float32); gD[~strict] = 0
        gA = rng.normal(0, 1, (Hd, Wd)).astype(np.float32); gA[~strict] = 0
        seeds.append((dLc, gD, gA))
        refs.append(_reference_grads(o, oa, dLc, gD, gA, c["world_view_transform"]))
    loss = sum((color[f] * t(dLc)).sum() + (depth[f, 0] * t(gD)).sum() + (alpha[f, 0] * t(gA)).sum()
               for f, (dLc, gD, gA) in enumerate(seeds))
    loss.backward()
    # LBS^T reference: torch autograd through the LBS oracle per frame, seeded with that frame's posed-space gradients
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone().requires_grad_(True)
    oxyz, oRc, osc, oA, otr = T(s["xyz"]), T(s["Rc"]), T(s["scales"]), T(As), T(trs)
    F32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    for f in range(K):
        pxyz_o, pq_o, psc_o, _ = lo.deform_gaussians(oxyz, oRc, osc, torch.from_numpy(s["w"]), oA[f],
                                                     smpl_scale=torch.from_numpy(s["smpl_scale"]), transl=otr[f])
        ((pxyz_o * F32(refs[f]["means3D"])).sum() + (pq_o * F32(refs[f]["rotations"])).sum() +
         (psc_o * F32(refs[f]["scales"])).sum()).backward()
    _grad_close("xyz_canon", xyz.grad.cpu().numpy(), oxyz.grad.numpy(), atol=1e-5)
    _grad_close("rotmat_canon", Rc.grad.cpu().numpy(), oRc.grad.numpy(), atol=1e-5)
    _grad_close("scales", sc.grad.cpu().numpy(), osc.grad.numpy(), atol=1e-5)
    _grad_close("opacity", op.grad.cpu().numpy(), sum(r["opacities"] for r in refs))
    _grad_close("sh", sh.grad.cpu().numpy(), sum(r["shs"] for r in refs))
    for f in range(K):
        _grad_close(f"viewspace[{f}]", m2d.grad[f].cpu().numpy(), refs[f]["means2D"])
        _grad_close(f"A[{f}]", A.grad[f].cpu().numpy()[:, :3, :], oA.grad[f].numpy()[:, :3, :], rtol=2e-3, atol=2e-4)
        _grad_close(f"transl[{f}]", tr.grad[f].cpu().numpy(), otr.grad[f].numpy(), rtol=2e-3, atol=2e-4)


def test_a_frame_that_overflows_has_background_zero_maps_and_zero_gradient():
    """One aux engine call whose capacity lies between the frames' pair counts: frames that fit equal single-frame aux calls (K = 1
    engines, gradients summed in frame order), frames that do not render the background with depth = alpha = 0 and contribute
    nothing -- poisoned workspaces (the aux workspace included) prove that nothing stale is followed."""
    from sings_amd.engine import SkinnedFramesEngine
    dev = _dev()
    N, J, W, H, K = 20000, 52, 160, 288, 6
    s, ins, A, transl, one, stacked, dL = _avatar(N, J, W, H, 9, K, False, False)
    transl = transl.clone(); transl[:, 2] -= torch.linspace(0.0, 0.6 * float(transl[0, 2].abs()), K, device=dev) * torch.sign(transl[:, 2])
    gD, gA = _map_losses(K, H, W, 21, dev)
    big = SkinnedFramesEngine(N, J, W, H, 16, K, dev, 64 * N)
    big.set_camera(one[0]); big.set_frames(ins["xyz"], None, ins["w"], A, ins["smpl_scale"], transl)
    R = big.forward(ins["sh"], ins["op"], ins["sc"], sync_num_rendered=True)
    assert min(R) * 1.05 < max(R), R
    cap = (sorted(R)[K // 2 - 1] + sorted(R)[K // 2]) // 2
    fits = [r <= cap for r in R]
    assert any(fits) and not all(fits)
    flat_ref, ref = None, {}
    for f in range(K):
        if not fits[f]:
            continue
        e1 = SkinnedFramesEngine(N, J, W, H, 16, 1, dev, cap, aux=True)
        e1.set_camera(one[0]); e1.set_frames(ins["xyz"], None, ins["w"], A[f:f + 1].contiguous(), ins["smpl_scale"], transl[f:f + 1].contiguous())
        assert e1.forward(ins["sh"], ins["op"], ins["sc"], sync_num_rendered=True) == [R[f]]
        e1.backward(ins["sh"], ins["op"], ins["sc"], dL[f:f + 1].contiguous(), dL_ddepth=gD[f:f + 1].contiguous(),
                    dL_dalpha=gA[f:f + 1].contiguous())
        torch.cuda.synchronize()
        flat_ref = e1.grad_flat.clone() if flat_ref is None else flat_ref + e1.grad_flat
        ref[f] = [x[0].clone() for x in (e1.color, e1.depth, e1.alpha, e1.d_means2D, e1.d_A, e1.d_transl)]
    eng = SkinnedFramesEngine(N, J, W, H, 16, K, dev, cap, aux=True)
    for buf in (eng.geom, eng.img, eng.bwd_ws, eng.aux_ws):
        buf.fill_(0xA5)
    eng.binning.view(K, -1)[:, eng.L.bin_ranges:].fill_(0xA5)
    eng.depth.fill_(7.0); eng.alpha.fill_(7.0)
    eng.set_camera(one[0]); eng.set_frames(ins["xyz"], None, ins["w"], A, ins["smpl_scale"], transl)
    assert eng.forward(ins["sh"], ins["op"], ins["sc"], sync_num_rendered=True) == R
    eng.backward(ins["sh"], ins["op"], ins["sc"], dL, dL_ddepth=gD, dL_dalpha=gA)
    torch.cuda.synchronize()
    bg = torch.from_numpy(np.ascontiguousarray(s["bg"])).to(dev)
    for f in range(K):
        got = [eng.color[f], eng.depth[f], eng.alpha[f], eng.d_means2D[f], eng.d_A[f], eng.d_transl[f]]
        if fits[f]:
            for name, a, b in zip(("color", "depth", "alpha", "means2D", "A", "transl"), got, ref[f]):
                assert torch.equal(a, b), (f, name)
        else:
            assert torch.equal(eng.color[f], bg[:, None, None].expand(3, H, W)), f
            assert float(eng.depth[f].abs().max()) == 0.0 and float(eng.alpha[f].abs().max()) == 0.0, f
            for x in got[3:]:
                assert float(x.abs().max()) == 0.0, f
    assert torch.isfinite(eng.grad_flat).all()
    assert torch.equal(eng.grad_flat, flat_ref)


@pytest.mark.parametrize("long_list", [False, True])
def test_render_frames_batched_maps_equal_get_render_pkgs_fused(long_list):
    """``render_frames_batched(return_aux=True)`` hands out the maps ``get_render_pkgs_fused(return_aux=True)`` renders for the same
    frames -- also when the long-rows hint fails and the batch is rendered again (the scene of test_gpu_frames.py's fallback test)."""
    from sings_amd.posed import FrameAnimator
    from sings_amd.renderer import get_render_pkgs_fused
    dev = _dev()
    N, J, W, H, F = (100000, 52, 160, 288, 4) if long_list else (20000, 52, 160, 288, 6)
    s, ins, A, transl, one, stacked, dL = _avatar(N, J, W, H, 5, F, False, True)
    canon = dict(xyz_canon=ins["xyz"] * (0.02 if long_list else 1.0), rotmat_canon=None, scales=ins["sc"], opacity=ins["op"],
                 shs=ins["sh"], lbs_weights=ins["w"], active_sh_degree=0)
    camd = {k_: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k_, v in s["cam"].items()}
    bg = torch.from_numpy(s["bg"]).to(dev)
    with torch.no_grad():
        pkg = get_render_pkgs_fused(camd, canon, A.reshape(F, J, 4, 4), bg, smpl_scale=ins["smpl_scale"], transl=transl,
                                    return_aux=True)
    assert tuple(pkg["depth"].shape) == (F, 1, H, W) and tuple(pkg["alpha"].shape) == (F, 1, H, W)
    assert float(pkg["alpha"].max()) > 0.5
    jobs = [(camd, A[f].reshape(J, 4, 4), transl[f], ins["smpl_scale"], None) for f in range(F)]
    fa = FrameAnimator(canon, streams=2)
    got = {i: (img, d, a) for i, img, d, a in fa.render_frames_batched(iter(jobs), bg, frames_per_launch=4, return_aux=True)}
    torch.cuda.synchronize()
    assert sorted(got) == list(range(F))
    if long_list:
        assert fa.long_rows is False                                 # the hint failed and the batch was rendered again
    for f in range(F):
        img, d, a = got[f]
        assert torch.equal(img, pkg["render"][f]), f
        assert torch.equal(d, pkg["depth"][f]) and torch.equal(a, pkg["alpha"][f]), f


# ---- frames in different regimes ---------------------------------------------------------------------------------------------
# transl z factors of the avatar (W 160 x H 288, N 20 000): 0.5 -> the body fills the frame, lists <= ~140 entries and thousands of
# pixels saturate (over-saturated); 1.0 -> short lists (< 256); 2.0 -> ~600; 4.0 -> lists past 1024 (several depth segments with
# D checkpoints, the bucket sort).  Frame 0 is not the longest, so a frame-0 base for the checkpoints, the z values or the dL/dz
# plane of a later frame reads another frame's data.
REGIMES = {4: [1.0, 4.0, 0.5, 2.0], 16: [0.5, 2.0, 1.0, 4.0, 4.0, 1.0, 0.5, 2.0, 1.0, 0.5, 4.0, 2.0, 0.5, 4.0, 1.0, 2.0]}


@pytest.mark.parametrize("K,with_rot", [(4, True), (16, False)])
def test_frames_in_different_regimes_equal_single_frame_calls_and_the_oracle(K, with_rot):
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = _dev()
    N, J, W, H = 20000, 52, 160, 288
    s, ins, A, transl, one, stacked, dL = _avatar(N, J, W, H, 7, K, True, with_rot)
    zf = torch.tensor(REGIMES[K], device=dev)
    transl = transl.clone()
    transl[:, 2] = transl[:, 2] * zf
    gD, gA = _map_losses(K, H, W, 23, dev)
    # the oracle's view of every frame (posed by the single-frame op): the regimes hold, and one long-list frame's seeds avoid its
    # borderline pixels so that it can be held against the oracle below
    posed, lists = [], []
    for f in range(K):
        with torch.no_grad():
            out = rasterize_skinned_gaussians(ins["xyz"], ins["rot"], ins["sc"], ins["op"], ins["sh"], ins["w"], A[f], one[f],
                                              smpl_scale=ins["smpl_scale"], transl=transl[f], return_posed=True)
        c = s["cam"]
        vm, pm, cp = (one[f].viewmatrix.cpu().numpy(), one[f].projmatrix.cpu().numpy(), one[f].campos.cpu().numpy())
        o, oa = _oracle_pair(out[2].cpu().numpy(), s["opacities"], vm, pm, cp, W, H, math.tan(c["fovx"] * 0.5),
                             math.tan(c["fovy"] * 0.5), s["bg"], out[4].cpu().numpy(), out[3].cpu().numpy(), s["shs"], 0)
        posed.append((o, oa, vm))
        lists.append(int((o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]).max()))
    saturated = [int((p[0]["final_T"] < 1.5e-4).sum()) for p in posed]
    assert min(lists) < 256 and max(lists) > 1024 and lists[0] < max(lists), lists
    assert max(saturated) > 1000, saturated
    fl = int(np.argmax(lists))
    o, oa, vm = posed[fl]
    strict = torch.from_numpy(o["margin"] >= 2e-5).to(dev)
    dL = dL.clone(); dL[fl][:, ~strict] = 0
    gD[fl, 0][~strict] = 0; gA[fl, 0][~strict] = 0

    (color, radii, depth, alpha), g, dA, dtr, dm2 = _frames_call(ins, A, transl, stacked, with_rot, dL, gD, gA)
    acc = {}
    for f in range(K):
        lv = _leaves(ins, with_rot)
        A1, tr1 = A[f].clone().requires_grad_(True), transl[f].clone().requires_grad_(True)
        m1 = torch.zeros(N, 3, device=dev, requires_grad=True)
        c1, r1, d1, a1 = rasterize_skinned_gaussians(lv["xyz"], lv["rot"], lv["sc"], lv["op"], lv["sh"], ins["w"], A1, one[f],
                                                     smpl_scale=ins["smpl_scale"], transl=tr1, means2D=m1, return_aux=True)
        ((c1 * dL[f]).sum() + (d1 * gD[f]).sum() + (a1 * gA[f]).sum()).backward()
        torch.cuda.synchronize()
        for name, a, b in (("color", color[f], c1.detach()), ("radii", radii[f], r1), ("depth", depth[f], d1.detach()),
                           ("alpha", alpha[f], a1.detach()), ("dA", dA[f], A1.grad), ("dtransl", dtr[f], tr1.grad),
                           ("means2D", dm2[f], m1.grad)):
            assert torch.equal(a, b), (f, REGIMES[K][f], name)
        for k, v in lv.items():
            if v is not None:
                acc[k] = v.grad.clone() if f == 0 else acc[k] + v.grad
    for k in acc:
        assert torch.equal(g[k], acc[k]), k
    # the long-list frame against the oracle: maps, its screen-space gradient and dL/dtransl (= the sum of the posed-mean
    # gradients, the dz x view-row term included)
    np.testing.assert_array_equal(radii[fl].cpu().numpy(), o["radii"])
    _check_maps(o, oa, depth[fl], alpha[fl])
    ref = _reference_grads(o, oa, dL[fl].cpu().numpy(), gD[fl, 0].cpu().numpy(), gA[fl, 0].cpu().numpy(), vm)
    _grad_close("viewspace", dm2[fl].cpu().numpy(), ref["means2D"])
    _grad_close("transl", dtr[fl].cpu().numpy(), ref["means3D"].sum(0), rtol=2e-3, atol=2e-4)
