"""Per-frame placement (ext_tfs) and smpl_scale in the skinned K-frame forward, and 8-bit HWC frames out
(SgFrameBatch.placement / SG_PLACEMENT_*, sg_frames_to_u8; ``SkinnedFramesEngine.set_frames(ext_tfs=...)``,
``FrameAnimator.render_frames_batched``, ``animate_chunk(frames_per_launch=K, out=...)``, ``posed.frames_to_u8``).

The bar: a K-frame forward whose frames carry their own placement and scale gives, frame by frame, the posed Gaussians of the
reference's ``forward_chunk`` pieces (golden G8) and bit for bit the images, radii, posed outputs and maps of K single-frame
forwards with that frame's ext_tfs; the animation driver takes the reference's chunk inputs (``.expand`` views of one AMASS
placement, ``smpl_scale`` ones [F,1]) through the K-frame path with the per-frame loop's images, fallbacks included; and the 8-bit
frames are numpy's ``(clip(x, 0, 1) * float32(255)).astype(uint8)`` to the bit.
"""
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_frames import _avatar

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "motion_golden.npz"))


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _placements(K, center, seed, scale=1.0, spread=0.05):
    """K distinct placements (trans [K,3], rotmat [K,3,3], scale [K,1]) that turn the avatar about ``center`` (a world point in
    view) and scale it about it: p' = center + e R (p - center)."""
    from sings_amd.body import rodrigues
    dev = _dev()
    rs = np.random.RandomState(seed)
    aa = torch.from_numpy(rs.normal(0, 0.15, (K, 3)).astype(np.float32))
    R = rodrigues(aa).to(dev).contiguous()
    e = torch.from_numpy((scale * (1.0 + spread * rs.uniform(-1, 1, (K, 1)))).astype(np.float32)).to(dev)
    c = torch.as_tensor(center, dtype=torch.float32, device=dev)
    trans = (c[None] - e * (R @ c[None, :, None])[..., 0]).contiguous()
    return trans, R, e


def _center(s):
    """The point on the camera's axis (identity extrinsic) at the avatar's depth."""
    return [0.0, 0.0, float(s["transl"][2] + s["xyz_canon"][:, 2].mean())]


# ---- 1. reference pin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iso", [False, True])
def test_k_frame_forward_with_per_frame_placement_against_the_reference_pieces(iso):
    """ONE K = 3 sg_skinned_forward_frames call, bits 0 and 1 set, on G8's inputs: its posed outputs are the reference's
    forward_chunk with three distinct ext_tfs and smpl_scale 1.07 / 0.93 / 1.0 (tolerances of test_motion.py's G8 test)."""
    from sings_amd import _lib
    from sings_amd.camera import make_camera
    from sings_amd.engine import SkinnedFramesEngine
    from sings_amd.rasterizer import GaussianRasterizationSettings
    dev = _dev()
    T = lambda k: torch.from_numpy(np.ascontiguousarray(G["g8_" + k])).to(dev)
    N, J, K, W, H = 500, 24, 3, 64, 64
    cam = make_camera(np.eye(4, dtype=np.float32), 60.0, 60.0, W / 2, H / 2, W, H)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), torch.ones(3, device=dev), 1.0,
                                       t(cam["world_view_transform"]), t(cam["full_proj_transform"]), 0, t(cam["camera_center"]),
                                       False, False)
    eng = SkinnedFramesEngine(N, J, W, H, 16, K, dev, 1 << 18, with_rot=not iso, rot_width=6)
    eng.set_camera(rs)
    eng.set_frames(T("xyz_canon"), None if iso else T("rot6d"), T("w"), T("A"), T("smpl_scale"), T("transl"),
                   (T("ext_trans"), T("ext_rot"), T("ext_scale")))
    assert eng._fb.placement == _lib.PLACEMENT_EXT_TFS | _lib.PLACEMENT_SMPL_SCALE
    posed = tuple(torch.empty(K, N, w, device=dev) for w in (3, 4, 3))
    g = torch.Generator(device="cpu").manual_seed(3)
    Rs = eng.forward(torch.rand(N, 16, 3, generator=g).to(dev), torch.rand(N, 1, generator=g).to(dev), T("scales"),
                     sync_num_rendered=True, posed_out=posed)
    assert all(0 <= r <= eng.cap for r in Rs)
    tag = f"g8_{'iso' if iso else 'aniso'}_ext"
    xyz, q, sc = (x.cpu().numpy() for x in posed)
    np.testing.assert_allclose(xyz, G[tag + "_xyz"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(sc, G[tag + "_scales"], rtol=1e-6, atol=1e-9)
    same = np.abs(q - G[tag + "_rotq"]).max(-1) < 2e-5       # (a different matrix_to_quaternion pick is the same rotation)
    assert same.mean() > 0.995, same.mean()
    # the three frames really differ in placement and scale
    assert not np.allclose(sc[0], sc[1]) and not np.allclose(xyz[0], xyz[2])


# ---- 2. bit identity with single-frame forwards ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,per_frame_camera,with_rot", [(2, False, False), (5, True, True), (8, False, True), (16, True, False)])
def test_per_frame_placement_equals_single_frame_forwards_bit_for_bit(K, per_frame_camera, with_rot):
    from sings_amd import _lib
    from sings_amd.engine import SkinnedEngine, SkinnedFramesEngine
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = _dev()
    N, J, W, H = 20000, 52, 160, 288
    s, ins, A, transl, one, stacked, _ = _avatar(N, J, W, H, 21 + K, K, per_frame_camera, with_rot)
    ext = _placements(K, _center(s), K)
    sc = torch.from_numpy(np.linspace(0.93, 1.07, K, dtype=np.float32)[:, None]).to(dev)        # smpl_scale [K,1]
    cap = 24 * N
    pw = (3, 4, 3)
    ref = SkinnedEngine(N, J, W, H, 16, dev, cap, with_rot=with_rot, rot_width=6)
    ref.throughput = True
    want = []
    for f in range(K):
        ext_f = tuple(x[f] for x in ext)
        posed = tuple(torch.empty(N, w, device=dev) for w in pw)
        ref.set_camera(one[f])
        ref.set_frame(ins["xyz"], ins["rot"], ins["w"], A[f], sc[f], transl[f], ext_f)
        R = ref.forward(ins["sh"], ins["op"], ins["sc"], sync_num_rendered=True, posed_out=posed)
        assert 0 < R <= cap
        with torch.no_grad():
            _, _, depth, alpha = rasterize_skinned_gaussians(ins["xyz"], ins["rot"], ins["sc"], ins["op"], ins["sh"], ins["w"], A[f],
                                                             one[f], smpl_scale=sc[f], transl=transl[f], ext_tfs=ext_f,
                                                             return_aux=True)
        torch.cuda.synchronize()
        want.append([ref.color.clone(), ref.radii.clone()] + list(posed) + [depth, alpha])
    assert float((want[0][0] < 0.99).float().mean()) > 0.01                 # the avatar is in view
    assert not torch.equal(want[0][2], want[-1][2])
    for aux in (False, True):
        eng = SkinnedFramesEngine(N, J, W, H, 16, K, dev, cap, with_rot=with_rot, rot_width=6, aux=aux)
        eng.set_camera(stacked)
        eng.set_frames(ins["xyz"], ins["rot"], ins["w"], A, sc, transl, ext)
        assert eng._fb.placement == _lib.PLACEMENT_EXT_TFS | _lib.PLACEMENT_SMPL_SCALE
        posed = tuple(torch.empty(K, N, w, device=dev) for w in pw)
        Rs = eng.forward(ins["sh"], ins["op"], ins["sc"], sync_num_rendered=True, posed_out=posed)
        torch.cuda.synchronize()
        assert all(0 < r <= cap for r in Rs)
        for f in range(K):
            got = [eng.color[f], eng.radii[f]] + [p[f] for p in posed]
            for n, (a, b) in enumerate(zip(got, want[f][:5])):
                assert torch.equal(a, b), (aux, f, n)
            if aux:
                assert torch.equal(eng.depth[f], want[f][5]) and torch.equal(eng.alpha[f], want[f][6]), f


def test_flag_zero_with_one_placement_equals_the_placement_repeated():
    """One shared set (flag 0), the same set repeated per frame (bits 0 and 1) and an ``.expand`` view: the same bits."""
    from sings_amd import _lib
    from sings_amd.engine import SkinnedFramesEngine
    dev = _dev()
    N, J, W, H, K = 20000, 52, 160, 288, 8
    s, ins, A, transl, one, stacked, _ = _avatar(N, J, W, H, 31, K, True, True)
    tr, R, e = (x[:1] for x in _placements(1, _center(s), 4))
    sc1 = torch.tensor([1.05], device=dev)
    eng = SkinnedFramesEngine(N, J, W, H, 16, K, dev, 24 * N, with_rot=True, rot_width=6)
    eng.set_camera(stacked)
    outs = []
    for ext, sc, bits in (((tr[0], R[0], e[0]), sc1, 0),
                          ((tr.repeat(K, 1), R.repeat(K, 1, 1), e.repeat(K, 1)), sc1.repeat(K), 3),
                          ((tr[0].expand(K, 3), R[0].expand(K, 3, 3), e[0].expand(K, 1)), sc1.expand(K, 1), 0)):
        eng.set_frames(ins["xyz"], ins["rot"], ins["w"], A, sc, transl, ext)
        assert eng._fb.placement == bits
        posed = tuple(torch.empty(K, N, w, device=dev) for w in (3, 4, 3))
        eng.forward(ins["sh"], ins["op"], ins["sc"], posed_out=posed)
        torch.cuda.synchronize()
        outs.append([eng.color.clone(), eng.radii.clone()] + list(posed))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    assert _lib.PLACEMENT_EXT_TFS | _lib.PLACEMENT_SMPL_SCALE == 3


# ---- 3. the reference's chunk inputs through animate_chunk ----------------------------------------------------------------------
def _amass_chunk(F):
    from sings_amd.body import joint_transforms, rodrigues
    from sings_amd.camera import make_camera
    from sings_amd.motion import manual_alignment
    from sings_amd.scene import avatar_scene
    dev = _dev()
    s = avatar_scene(N=8000, J=24, W=128, H=224, seed=7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = make_camera(np.eye(4, dtype=np.float32), 400.0, 400.0, 64, 112, 128, 224)
    data = dict(fovx=cam["fovx"], fovy=cam["fovy"], image_height=224, image_width=128,
                world_view_transform=t(cam["world_view_transform"]), full_proj_transform=t(cam["full_proj_transform"]),
                camera_center=t(cam["camera_center"]))
    rs = np.random.RandomState(3)
    poses = t(rs.normal(0, 0.2, (F, 72)).astype(np.float32))
    transl = t(rs.normal(0, 0.02, (F, 3)).astype(np.float32))
    jr = t(s["joints_rest"])
    canon = dict(xyz_canon=t(s["xyz_canon"]), rotmat_canon=None, scales=t(s["scales"]), opacity=t(s["opacities"]),
                 shs=t(s["shs"]), lbs_weights=t(s["lbs_weights"]), active_sh_degree=0)
    A_cano = joint_transforms(torch.zeros(72, device=dev), jr, tuple(s["parents"]))
    # AnimDataset_opt.get_chunk: ONE manual_alignment placement as .expand views, smpl_scale ones [F,1]
    tr, aa, scale = manual_alignment("AMASS")
    manual_trans = torch.tensor(tr, dtype=torch.float32)[None].to(dev)
    manual_rotmat = rodrigues(torch.tensor(aa, dtype=torch.float32)[None]).to(dev)
    manual_scale = torch.tensor([[scale]], dtype=torch.float32).to(dev)
    ext_tfs = (manual_trans.expand(F, -1), manual_rotmat.expand(F, -1, -1), manual_scale.expand(F, -1))
    assert ext_tfs[0].stride(0) == 0 and ext_tfs[1].stride(0) == 0
    smpl_scale = torch.ones(F, 1, device=dev)
    return s, canon, poses, jr, A_cano, data, transl, smpl_scale, ext_tfs


def test_animate_chunk_takes_the_reference_chunk_inputs_through_the_k_frame_path(monkeypatch):
    from sings_amd import _lib
    from sings_amd.engine import SkinnedFramesEngine
    from sings_amd.posed import animate_chunk
    F = 37                                                            # 4 batches of 8 + a short tail of 5
    s, canon, poses, jr, A_cano, data, transl, smpl_scale, ext_tfs = _amass_chunk(F)
    bg = torch.ones(3, device=_dev())
    kw = dict(transl=transl, smpl_scale=smpl_scale, ext_tfs=ext_tfs, parents=tuple(s["parents"]), chunk_size=16)
    ref = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, **kw))
    assert sorted(ref) == list(range(F))
    assert float((ref[0] < 0.99).float().mean()) > 0.01               # the placed avatar is in view
    assert not torch.equal(ref[0], ref[F - 1])
    seen = []
    fwd = SkinnedFramesEngine.forward

    def spy(self, *a, **k):
        seen.append((self.K, int(self._fb.placement)))
        return fwd(self, *a, **k)
    monkeypatch.setattr(SkinnedFramesEngine, "forward", spy)
    got = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, streams=2, frames_per_launch=8, **kw))
    torch.cuda.synchronize()
    # five K-frame launches (the expand views are one shared placement: flag 0; the ones [F,1] one scale per frame)
    assert seen == [(8, _lib.PLACEMENT_SMPL_SCALE)] * 5, seen
    assert sorted(got) == list(range(F))
    for f in range(F):
        assert torch.equal(got[f], ref[f]), f
    # the same placement as [F,...] rows of their own (what `.expand(...).to(device)` of a host tensor hands over): one per frame
    seen.clear()
    kw_rows = dict(kw, ext_tfs=tuple(x.contiguous() for x in ext_tfs))
    got = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, streams=2, frames_per_launch=8, **kw_rows))
    torch.cuda.synchronize()
    assert seen == [(8, _lib.PLACEMENT_EXT_TFS | _lib.PLACEMENT_SMPL_SCALE)] * 5, seen
    for f in range(F):
        assert torch.equal(got[f], ref[f]), f
    # 8-bit BGR frames out of the same path: the float frames converted the reference's way
    seen.clear()
    got8 = dict(animate_chunk(canon, poses, jr, A_cano, data, bg, streams=2, frames_per_launch=8, out="bgr8", **kw))
    torch.cuda.synchronize()
    assert len(seen) == 5
    for f in range(F):
        assert got8[f].dtype == torch.uint8 and got8[f].shape == (224, 128, 3)
        assert np.array_equal(got8[f].cpu().numpy(), _np_u8(ref[f].cpu().numpy(), True)), f
    # ... and out of the per-frame loop
    got_rgb = dict(animate_chunk(canon, poses[:3], jr, A_cano, data, bg, out="rgb8", **kw))
    for f in range(3):
        assert np.array_equal(got_rgb[f].cpu().numpy(), _np_u8(ref[f].cpu().numpy(), False)), f


# ---- 4. the fallbacks keep the placement ----------------------------------------------------------------------------------------
def _single_frame_refs(canon, camd, A, bg, sc, transl, ext):
    from sings_amd.renderer import get_render_pkg_fused
    with torch.no_grad():
        return [get_render_pkg_fused(camd, canon, A[f], bg, smpl_scale=sc[f], transl=transl[f],
                                     ext_tfs=tuple(x[f] for x in ext))["render"].clone() for f in range(A.shape[0])]


def test_long_rows_fallback_keeps_the_placement():
    """An ext_scale of ~0.01 crowds the 100k-Gaussian avatar into a few tiles (lists beyond 16384 entries): the optimistic
    SG_FLAG_LONG_ROWS batch is refused on the device and rendered again, with the same per-frame placements."""
    from sings_amd.posed import FrameAnimator
    dev = _dev()
    N, J, W, H, F = 100000, 52, 160, 288, 4
    s, ins, A, transl, one, stacked, _ = _avatar(N, J, W, H, 5, F, False, True)
    ext = _placements(F, _center(s), 8, scale=0.01, spread=0.2)
    sc = torch.from_numpy(np.linspace(0.95, 1.05, F, dtype=np.float32)[:, None]).to(dev)
    canon = dict(xyz_canon=ins["xyz"], rotmat_canon=None, scales=ins["sc"], opacity=ins["op"], shs=ins["sh"], lbs_weights=ins["w"],
                 active_sh_degree=0)
    camd = {k_: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k_, v in s["cam"].items()}
    bg = torch.from_numpy(s["bg"]).to(dev)
    want = _single_frame_refs(canon, camd, A.reshape(F, J, 4, 4), bg, sc, transl, ext)
    bgv = torch.clamp(bg, 0.0, 1.0)[:, None, None].expand(3, H, W)
    assert not any(torch.equal(w, bgv) for w in want)
    jobs = [(camd, A[f].reshape(J, 4, 4), transl[f], sc[f], tuple(x[f] for x in ext)) for f in range(F)]
    fa = FrameAnimator(canon, streams=2)
    assert fa.long_rows is True
    got = dict(fa.render_frames_batched(iter(jobs), bg, frames_per_launch=4))
    torch.cuda.synchronize()
    assert fa.long_rows is False and sorted(got) == list(range(F))         # (the hint was refused: the batch was rendered again)
    for f in range(F):
        assert torch.equal(got[f], want[f]), f


_overflow_scene_cache = []


def _overflow_scene():
    """The scene of the capacity-overflow test and its single-frame references, rendered once for the three paths."""
    if not _overflow_scene_cache:
        dev = _dev()
        N, J, W, H, F = 20000, 52, 160, 288, 5
        s, ins, A, transl, one, stacked, _ = _avatar(N, J, W, H, 6, F, False, True)
        ext = _placements(F, _center(s), 9)
        sc = torch.from_numpy(np.linspace(0.95, 1.05, F, dtype=np.float32)[:, None]).to(dev)
        canon = dict(xyz_canon=ins["xyz"], rotmat_canon=None, scales=ins["sc"] * 15.0, opacity=ins["op"], shs=ins["sh"],
                     lbs_weights=ins["w"], active_sh_degree=0)
        camd = {k_: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v)
                for k_, v in s["cam"].items()}
        bg = torch.from_numpy(s["bg"]).to(dev)
        want = _single_frame_refs(canon, camd, A.reshape(F, J, 4, 4), bg, sc, transl, ext)
        jobs = [(camd, A[f].reshape(J, 4, 4), transl[f], sc[f], tuple(x[f] for x in ext)) for f in range(F)]
        _overflow_scene_cache.append((canon, bg, jobs, want, (N, W, H)))
    return _overflow_scene_cache[0]


@pytest.mark.parametrize("path", ["render_round", "render_frames", "render_frames_batched"])
def test_capacity_overflow_fallback_keeps_the_placement(path):
    """Gaussians large enough that a frame's pairs exceed the animator's first capacity (8 per Gaussian): the frame (or the batch) is
    rendered again on grown workspaces, with the same per-frame placements and scales, on each of the three paths -- rounds of 2, 2
    and 1 jobs, the pipelined per-frame path, and K = 4 frames per launch, whose short tail batch (5 = 4 + 1) is padded with its
    last frame's placement.  Scales x 15: the largest frame produces R = 1 167 541 pairs against a floor of 160 180, so a single
    frame overflows as the batch does and each path ends with the capacity 1 460 450 (measured on the MI355X)."""
    from sings_amd.overflow import EngineCapacity
    from sings_amd.posed import FrameAnimator
    canon, bg, jobs, want, (N, W, H) = _overflow_scene()
    F = len(jobs)
    fa = FrameAnimator(canon, streams=2)
    floor = EngineCapacity.floor(0, N, W, H)
    if path == "render_round":
        got = {f0 + k: img for f0 in range(0, F, 2) for k, img in enumerate(fa.render_round(jobs[f0:f0 + 2], bg))}
    elif path == "render_frames":
        got = dict(fa.render_frames(iter(jobs), bg))
    else:
        got = dict(fa.render_frames_batched(iter(jobs), bg, frames_per_launch=4))
    torch.cuda.synchronize()
    assert fa.cap > floor, (fa.cap, floor)                                # (the overflow re-render ran)
    assert sorted(got) == list(range(F))
    for f in range(F):
        assert torch.equal(got[f], want[f]), f


# ---- 5. backward refused --------------------------------------------------------------------------------------------------------
def test_backward_refuses_placement_and_per_frame_scale():
    import ctypes as C
    from sings_amd import _lib
    from sings_amd.engine import SkinnedFramesEngine
    from sings_amd._marshal import _frame_batch, _ptr
    dev = _dev()
    N, J, W, H, K = 2000, 52, 160, 288, 3
    s, ins, A, transl, one, stacked, dL = _avatar(N, J, W, H, 2, K, False, False)
    eng = SkinnedFramesEngine(N, J, W, H, 16, K, dev, 24 * N)
    eng.set_camera(stacked)
    ext = _placements(K, _center(s), 1)
    for sc, e in ((ins["smpl_scale"].repeat(K), None), (ins["smpl_scale"], ext), (ins["smpl_scale"], tuple(x[0] for x in ext))):
        eng.set_frames(ins["xyz"], None, ins["w"], A, sc, transl, e)
        eng.forward(ins["sh"], ins["op"], ins["sc"])
        for call in (lambda: eng.backward(ins["sh"], ins["op"], ins["sc"], dL), lambda: eng.backward_records(dL),
                     lambda: eng.backward_gaussians(ins["sh"], ins["op"], ins["sc"])):
            with pytest.raises(RuntimeError, match="forward-only"):
                call()
    eng.set_frames(ins["xyz"], None, ins["w"], A, ins["smpl_scale"], transl)     # shared scale, no placement: differentiable
    eng.forward(ins["sh"], ins["op"], ins["sc"])
    eng.backward(ins["sh"], ins["op"], ins["sc"], dL)
    torch.cuda.synchronize()
    # the C entry points refuse the bits themselves (before anything is launched)
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for bit in (_lib.PLACEMENT_EXT_TFS, _lib.PLACEMENT_SMPL_SCALE):
        fb = _frame_batch(K, 0, 3, bit)
        rc = lib.sg_rasterize_backward_records_frames(C.byref(eng._s), C.byref(fb), N, _ptr(eng.geom), _ptr(eng.binning), eng.cap,
                                                      _ptr(eng.img), _ptr(eng.bwd_ws), _ptr(dL), st)
        assert rc != 0 and "forward-only" in lib.sg_last_error().decode()
        rc = lib.sg_skinned_backward_gaussians_frames(
            C.byref(eng._s), C.byref(fb), N, C.byref(eng._k), _ptr(ins["sh"]), _ptr(ins["op"]), _ptr(ins["sc"]), _ptr(eng.radii),
            _ptr(eng.geom), _ptr(eng.binning), eng.cap, _ptr(eng.bwd_ws), _ptr(eng.skin_ws), 0, None, None, _ptr(eng.d_xyz), None,
            _ptr(eng.d_scales), _ptr(eng.d_opacity), _ptr(eng.d_sh), _ptr(eng.d_means2D), _ptr(eng.d_A), _ptr(eng.d_transl), st)
        assert rc != 0 and "forward-only" in lib.sg_last_error().decode()
    torch.cuda.synchronize()


# ---- 6. 8-bit frames ------------------------------------------------------------------------------------------------------------
def _np_u8(x, bgr):
    """The reference's conversion in numpy: (clip(x, 0, 1) * float32(255)).astype(uint8), HWC (NaN, undefined in numpy's cast,
    is 0 here), channels reversed for BGR."""
    x = np.where(np.isnan(x), np.float32(0), x).astype(np.float32)
    y = (np.clip(x, 0, 1) * np.float32(255)).astype(np.uint8)
    y = np.moveaxis(y, -3, -1)
    return np.ascontiguousarray(y[..., ::-1] if bgr else y)


def _crafted():
    """k/255 and its neighbours one ulp either side for every k, 0, 1, negatives, values above 1, +-inf and NaN."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    vals = [k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
            np.array([0.0, -0.0, 1.0, -1e-30, -0.5, -3.0, 1.0000001, 1.5, 7e30, np.inf, -np.inf, np.nan, 0.5, 0.999999,
                      np.float32(1) / np.float32(255) * np.float32(0.5)], np.float32)]
    return np.concatenate(vals).astype(np.float32)


@pytest.mark.parametrize("K,H,W", [(1, 37, 53), (16, 37, 53), (1, 32, 48), (16, 24, 40)])
@pytest.mark.parametrize("bgr", [False, True])
def test_frames_to_u8_equals_numpy(K, H, W, bgr):
    from sings_amd.posed import frames_to_u8
    dev = _dev()
    rs = np.random.RandomState(K * 1000 + H)
    x = rs.uniform(-0.2, 1.2, (K, 3, H, W)).astype(np.float32)
    c = _crafted()
    flat = x.reshape(-1)
    for off in (0, flat.size // 2, flat.size - c.size):                   # crafted values in every channel, first and last pixels
        flat[off:off + c.size] = c
    got = frames_to_u8(torch.from_numpy(x).to(dev), bgr=bgr)
    assert got.dtype == torch.uint8 and got.shape == (K, H, W, 3) and got.is_cuda
    want = _np_u8(x, bgr)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (got.cpu().numpy().reshape(-1) == 0).any() and (got.cpu().numpy() == 255).any()
    one = frames_to_u8(torch.from_numpy(x[0]).to(dev), bgr=bgr)                   # [3,H,W] -> [H,W,3]
    assert one.shape == (H, W, 3) and np.array_equal(one.cpu().numpy(), want[0])
    nan_at = np.isnan(x)
    assert nan_at.any() and (np.moveaxis(got.cpu().numpy(), -1, -3)[:, ::-1 if bgr else 1][nan_at] == 0).all()


def test_frames_to_u8_of_rendered_frames():
    """Rendered K-frame images (the raw, unclamped colour: values beyond [0, 1] included) through both channel orders."""
    from sings_amd.engine import SkinnedFramesEngine
    from sings_amd.posed import frames_to_u8
    dev = _dev()
    N, J, W, H, K = 20000, 52, 160, 288, 16
    s, ins, A, transl, one, stacked, _ = _avatar(N, J, W, H, 17, K, True, False)
    eng = SkinnedFramesEngine(N, J, W, H, 16, K, dev, 24 * N)
    eng.set_camera(stacked)
    eng.set_frames(ins["xyz"], None, ins["w"], A, ins["smpl_scale"], transl, _placements(K, _center(s), 2))
    eng.forward(ins["sh"], ins["op"], ins["sc"])
    torch.cuda.synchronize()
    x = eng.color.cpu().numpy()
    assert (x < 0.99).mean() > 0.01
    for bgr in (False, True):
        assert np.array_equal(frames_to_u8(eng.color, bgr=bgr).cpu().numpy(), _np_u8(x, bgr))
        assert np.array_equal(frames_to_u8(torch.clamp(eng.color, 0.0, 1.0), bgr=bgr).cpu().numpy(), _np_u8(x, bgr))
