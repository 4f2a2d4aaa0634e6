"""The fused skinning kernels (sg_skin.hip, sg_skin.h, sg_skin_bwd.inc, sg_skin_bwd_frames.inc) at every joint-count and tile edge: the
cases of tests/skin_edge_case.py (J from 1 to 64 across the chunk, k-step, float4 / scalar staging and 64 KiB LDS boundaries; P
from 1 across the wave and workgroup boundaries), proved to test what they claim by tests/test_skin_edge_cases_host.py.

 a. single frame against the oracles: the checks of test_gpu_skinned.test_fused_forward / test_fused_backward, unchanged;
 b. pure LBS^T at a bar the raster noise does not set: only upstream gradients on the posed means and quaternions drive the
    backward (posed_scales is not differentiable in the operator, so dL/dscales must come back exactly zero); against fp64 autograd
    of the restatement at test_gpu_skinned._close's pairs x 0.1 -- 4.4 x the fp32 restatement's own error on 6-D rotations, 9 x or
    more on every other array (measured by the host file; skin_edge_case's docstring), the margin covering the device's
    ascending-joint W.A sums and its slab / two-stage dA sums against BLAS order.  Measured on the MI355X, worst ratio to the bar:
    xyz_canon 0.114, canonical rotation 0.535 (6-D, P = 1; 0.063 with 3 x 3 matrices), A 0.006, transl 0.002;
 c. one-hot weight rows: T = A[j] exactly, unused joints' dL/dA exactly zero, sum_j dL/dA[j] = sum_i dT_i;
 d. K frames equal K single-frame calls bit for bit (the protocol of test_gpu_frames) -- with (a) this chains the K-frame kernels
    to the fp64 reference;
 e. inputs inside a NaN-filled buffer: any read beyond P J or J 16 floats, even one multiplied by a zero weight, turns an output
    into NaN (every access stays inside the one allocation);
 f. the scene forward with per-avatar J and block offsets.
"""
import math

import numpy as np
import pytest
import torch

import skin_edge_case as sec
import test_gpu_skinned as TS
from oracle import raster_oracle as ro

pytestmark = pytest.mark.gpu
BORDER = 2e-5
CAP = 1 << 14                    # pairs: P <= 300 Gaussians on the 4 x 3 tiles of a 64 x 48 image


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _req(a):
    return None if a is None else _t(a).requires_grad_(True)


def _run_single(s, deg, image_loss):
    """rasterize_skinned_gaussians(return_posed=True, means2D=...) on a single-frame scene + backward of <posed means, wx> +
    <posed quaternions, wq> (+ <image, dL> off the oracle's borderline pixels) -> dict of outputs, leaves and the oracle's results."""
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = _dev()
    P = s["P"]
    rs = TS._settings(s, dev, deg)
    lv = dict(xyz=_req(s["xyz"]), rot=_req(s["rot_in"]), sc=_req(s["scales"]), op=_req(s["opac"]), sh=_req(s["shs"]), A=_req(s["A"]),
              tr=_req(s["transl"]))
    m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
    color, radii, pxyz, pq, psc = rasterize_skinned_gaussians(lv["xyz"], lv["rot"], lv["sc"], lv["op"], lv["sh"], _t(s["w"]), lv["A"], rs,
                                                              smpl_scale=_t(s["smpl_scale"]), transl=lv["tr"], return_posed=True,
                                                              means2D=m2d)
    wx, wq, _ = sec.upstream(s)
    loss = (pxyz * _t(wx)).sum() + (pq * _t(wq)).sum()
    out = dict(rs=rs, lv=lv, m2d=m2d, color=color, radii=radii, pxyz=pxyz, pq=pq, psc=psc, wx=wx, wq=wq)
    if image_loss:
        cam = s["cam"]
        o = ro.forward(pxyz.detach().cpu().numpy(), s["opac"], cam["world_view_transform"], cam["full_proj_transform"],
                       cam["camera_center"], s["W"], s["H"], math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"],
                       scales=psc.cpu().numpy(), rotations=pq.detach().cpu().numpy(), shs=s["shs"], sh_degree=deg)
        dL = s["dL"].copy(); dL[:, o["margin"] < BORDER] = 0
        loss = loss + (color * _t(dL)).sum()
        out.update(o=o, dL=dL)
    loss.backward()
    torch.cuda.synchronize()
    return out


# ---- a. single frame against the oracles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sec.SINGLE, ids=sec.case_id)
def test_single_frame_against_the_oracles(case):
    from diff_gaussian_rasterization import GaussianRasterizer
    P, J, seed, rot, deg = case
    s = sec.scene(P, J, seed, rot)
    r = _run_single(s, deg, image_loss=True)
    c = lambda x: x.detach().cpu().numpy()
    lv, m2d, color, radii, pxyz, pq, psc, o = (r[k] for k in ("lv", "m2d", "color", "radii", "pxyz", "pq", "psc", "o"))
    # -- test_fused_forward's checks
    _, (oxyz, oq, osc, _) = sec.deform(s)
    assert np.abs(c(pxyz) - oxyz.numpy()).max() < 2e-5
    assert np.abs(c(psc) - osc.numpy()).max() < 1e-8
    assert np.abs(c(pq) - oq.numpy()).max() < 2e-5
    assert int((radii > 0).sum()) > 0.5 * P
    with torch.no_grad():
        c2, r2 = GaussianRasterizer(r["rs"])(means3D=pxyz.detach(), means2D=torch.zeros_like(pxyz), opacities=_t(s["opac"]),
                                             shs=_t(s["shs"]), scales=psc, rotations=pq.detach())
    assert torch.equal(radii, r2) and torch.equal(color.detach(), c2)
    assert np.array_equal(o["radii"], c(radii))
    strict = o["margin"] >= BORDER
    assert np.abs(c(color) - o["color"]).max(0)[strict].max() <= 1e-5
    # -- test_fused_backward's checks: torch autograd through the restatement, seeded with the oracle's posed-space gradients
    g = ro.backward(o, r["dL"])
    olv, (pxyz_o, pq_o, psc_o, _) = sec.deform(s, grad=True)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    ((pxyz_o * (f32(g["dL_dmeans3D"]) + f32(r["wx"]))).sum() + (pq_o * (f32(g["dL_drots"]) + f32(r["wq"]))).sum()
     + (psc_o * f32(g["dL_dscales"])).sum()).backward()
    TS._close("xyz_canon", c(lv["xyz"].grad), olv["xyz"].grad.numpy())
    TS._close("scales", c(lv["sc"].grad), olv["scales"].grad.numpy())
    if rot != "iso":
        TS._close("rot_canon", c(lv["rot"].grad), olv["rot"].grad.numpy())
    TS._close("A", c(lv["A"].grad)[:, :3, :], olv["A"].grad.numpy()[:, :3, :], rtol=2e-3, atol_scale=2e-4)
    assert np.abs(c(lv["A"].grad)[:, 3, :]).max() == 0
    TS._close("transl", c(lv["tr"].grad), olv["transl"].grad.numpy(), rtol=2e-3, atol_scale=2e-4)
    TS._close("opacity", c(lv["op"].grad), g["dL_dopacity"], rtol=2e-4, atol_scale=2e-6)
    TS._close("sh", c(lv["sh"].grad), g["dL_dsh"], rtol=2e-4, atol_scale=2e-6)
    TS._close("viewspace", c(m2d.grad), g["dL_dmean2D"], rtol=2e-4, atol_scale=2e-6)


# ---- b. pure LBS^T ----------------------------------------------------------------------------------------------------------------
def _lbs_t_against_fp64(label, s, r):
    """The device gradients of a run driven by the upstream gradients alone against fp64 autograd of the restatement at the bar
    of (b); prints every array's ratio to the bar before asserting."""
    c = lambda x: x.detach().cpu().numpy()
    lv = r["lv"]
    ref = sec.lbs_gradients(s, r["wx"], r["wq"], None)
    got = dict(xyz_canon=c(lv["xyz"].grad), rot_canon=None if lv["rot"] is None else c(lv["rot"].grad), scales=c(lv["sc"].grad),
               A=c(lv["A"].grad), transl=c(lv["tr"].grad))
    ratios = {n: sec.bar_ratio(n, got[n], ref[n]) for n in sec.BAR if got[n] is not None}
    print(f"LBS^T ratio to the bar of (b) [{label}]: " + ", ".join(f"{n} {v:.3f}" for n, v in ratios.items()))
    assert not np.any(got["scales"]) and not np.any(ref["scales"])      # no loss reaches the posed scales: exactly zero
    assert np.abs(got["A"].reshape(-1, 4, 4)[:, 3, :]).max() == 0
    for n in ratios:
        a, b = got[n], ref[n]
        if n == "A":
            a, b = a.reshape(-1, 4, 4)[:, :3, :], b.reshape(-1, 4, 4)[:, :3, :]
        TS._close(n, a, b, rtol=sec.BAR[n][0], atol_scale=sec.BAR[n][1])
    return got, ref


@pytest.mark.parametrize("case", sec.SINGLE, ids=sec.case_id)
def test_lbs_transpose_against_fp64_autograd(case):
    """Measured on the MI355X over SINGLE (worst ratio to this bar per array): see LAB.md, "fused skinning kernels at the edges"."""
    P, J, seed, rot, deg = case
    s = sec.scene(P, J, seed, rot)
    r = _run_single(s, deg, image_loss=False)
    _lbs_t_against_fp64(sec.case_id(case), s, r)
    assert float(r["m2d"].grad.abs().max()) == 0.0                       # (no image loss: no screen-space gradient)


# ---- c. one-hot weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sec.ONE_HOT, ids=sec.case_id)
def test_one_hot_weights(case):
    P, J, seed = case
    s = sec.one_hot(P, J, seed)
    r = _run_single(s, 0, image_loss=False)
    c = lambda x: x.detach().cpu().numpy()
    _, (oxyz, oq, osc, T) = sec.deform(s)
    joint = s["w"].argmax(1)
    assert np.array_equal(T.numpy(), s["A"][joint])                      # the restatement with T = A[j], exactly
    oxyz = oxyz.numpy()
    ulp = np.spacing(np.abs(oxyz).max(1, keepdims=True).astype(np.float32))
    assert (np.abs(c(r["pxyz"]).astype(np.float64) - oxyz) / ulp).max() <= 2.0
    got, ref = _lbs_t_against_fp64("one-hot " + sec.case_id(case), s, r)
    unused = [j for j in range(J) if j not in s["used"]]
    assert J < 3 or unused
    assert not np.any(got["A"].reshape(J, 16)[unused]), "dL/dA of a joint no Gaussian uses"
    # sum_j w_ij = 1: the joints' dL/dA rows sum to the Gaussians' dT
    TS._close("sum_j dA", got["A"].reshape(J, 4, 4)[:, :3, :].astype(np.float64).sum(0), ref["A"].reshape(J, 4, 4)[:, :3, :].sum(0),
              rtol=sec.BAR["A"][0], atol_scale=sec.BAR["A"][1])


# ---- d. K frames equal K single-frame calls ---------------------------------------------------------------------------------------
def _rot_args(s):
    """(rotation tensor for the engines, with_rot, rot_width)"""
    if s["rot"] == "iso":
        return None, False, 9
    return (_t(s["rot_in"]), True, 6) if s["rot"] == "6d" else (_t(s["rot_in"].reshape(-1, 9)), True, 9)


def _frames_inputs(s):
    rot, with_rot, rw = _rot_args(s)
    K, J = s["K"], s["J"]
    return dict(xyz=_t(s["xyz"]), rot=rot, with_rot=with_rot, rw=rw, w=_t(s["w"]), sc=_t(s["scales"]), op=_t(s["opac"]), sh=_t(s["shs"]),
                A=_t(s["A"].reshape(K, J, 16)), transl=_t(s["transl"]), smpl_scale=_t(s["smpl_scale"]), dL=_t(s["dL"]))


def _frames_equal_single_calls(s, accumulate_first=False):
    """test_gpu_frames.test_skinned_frames_equal_single_frame_calls_bit_for_bit's protocol on scene ``s``."""
    from sings_amd.engine import SkinnedEngine, SkinnedFramesEngine
    dev = _dev()
    K, P, J, W, H = s["K"], s["P"], s["J"], s["W"], s["H"]
    i = _frames_inputs(s)
    rs = TS._settings(s, dev, 0)
    ref = SkinnedEngine(P, J, W, H, sec.M, dev, CAP, with_rot=i["with_rot"], rot_width=i["rw"])
    ref.throughput = True
    start = torch.from_numpy(np.random.RandomState(3).normal(size=ref.grad_flat.numel()).astype(np.float32)).to(dev)
    ref.grad_flat.copy_(start)
    per_frame = []
    for f in range(K):
        ref.set_camera(rs)
        ref.set_frame(i["xyz"], i["rot"], i["w"], i["A"][f], i["smpl_scale"], i["transl"][f])
        R = ref.forward(i["sh"], i["op"], i["sc"], sync_num_rendered=True)
        assert 0 < R <= CAP
        ref.backward(i["sh"], i["op"], i["sc"], i["dL"][f], accumulate=accumulate_first or f > 0)
        torch.cuda.synchronize()
        per_frame.append([x.clone() for x in (ref.color, ref.radii, ref.d_means2D, ref.d_A, ref.d_transl)] + [R])
    ref_grad = ref.grad_flat.clone()
    eng = SkinnedFramesEngine(P, J, W, H, sec.M, K, dev, CAP, with_rot=i["with_rot"], rot_width=i["rw"])
    eng.set_camera(rs)
    eng.set_frames(i["xyz"], i["rot"], i["w"], i["A"], i["smpl_scale"], i["transl"])
    for rep in range(2):                                            # twice: the workspaces are reused (SG_FLAG_WS_CLEAN)
        eng.grad_flat.copy_(start)
        Rs = eng.forward(i["sh"], i["op"], i["sc"], sync_num_rendered=True)
        eng.backward(i["sh"], i["op"], i["sc"], i["dL"], accumulate=accumulate_first)
        torch.cuda.synchronize()
        assert Rs == [p[5] for p in per_frame] and eng.num_rendered() == Rs
        for f in range(K):
            c, r, m2, dA, dt, _ = per_frame[f]
            assert torch.equal(eng.color[f], c), f"image of frame {f}"
            assert torch.equal(eng.radii[f], r) and torch.equal(eng.d_means2D[f], m2), f"radii / means2D of frame {f}"
            assert torch.equal(eng.d_A[f], dA), f"dL/dA of frame {f}"
            assert torch.equal(eng.d_transl[f], dt), f"dL/dtransl of frame {f}"
        assert torch.equal(eng.grad_flat, ref_grad), "summed canonical-Gaussian gradient"
    assert torch.isfinite(ref_grad).all() and not torch.equal(ref_grad, start)
    assert float(torch.stack([p[3] for p in per_frame]).abs().max()) > 0
    assert float((per_frame[0][0] - per_frame[-1][0]).abs().max()) > 1e-3      # (the frames really differ)


@pytest.mark.parametrize("case", sec.FRAMES, ids=sec.case_id)
def test_frames_equal_single_frame_calls_bit_for_bit(case):
    K, P, J, seed, rot = case
    _frames_equal_single_calls(sec.scene(P, J, seed, rot, K=K))


def test_frames_accumulating_from_the_first_call():
    """``accumulate=True`` on the engine's call (the ACC variant of the K-frame kernel: the sums start from what the buffer holds)
    against a chain of single-frame calls whose first one accumulates too; J = 63 (scalar staging, a padded last k-step)."""
    K, P, J, seed, rot = next(c for c in sec.FRAMES if (c[0], c[1], c[2]) == (3, 257, 63))
    _frames_equal_single_calls(sec.scene(P, J, seed, rot, K=K), accumulate_first=True)


def _per_frame_cameras(s, rs):
    """(one settings per frame, the stacked settings): camera f shifted along x by 0.02 f, as tests/test_gpu_frames._avatar."""
    cam, K = s["cam"], s["K"]
    view = np.repeat(cam["world_view_transform"][None], K, 0).copy()
    view[:, 3, 0] += 0.02 * np.arange(K)
    P_T = np.linalg.inv(cam["world_view_transform"]) @ cam["full_proj_transform"]
    proj = np.stack([(v @ P_T).astype(np.float32) for v in view])
    campos = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in view])
    one = [rs._replace(viewmatrix=_t(view[f]), projmatrix=_t(proj[f]), campos=_t(campos[f])) for f in range(K)]
    return one, rs._replace(viewmatrix=_t(view), projmatrix=_t(proj), campos=_t(campos))


def _case_17_65_2():
    K, P, J, seed, rot = next(c for c in sec.FRAMES if (c[0], c[1], c[2]) == (2, 65, 17))
    return sec.scene(P, J, seed, rot, K=K)


def test_frames_autograd_with_a_camera_per_frame_and_a_shared_translation():
    from sings_amd.skinned import rasterize_skinned_frames, rasterize_skinned_gaussians
    dev = _dev()
    s = _case_17_65_2()
    K, P = s["K"], s["P"]
    i = _frames_inputs(s)
    one, stacked = _per_frame_cameras(s, TS._settings(s, dev, 0))
    shared = i["transl"][0].clone()

    def leaves():
        lv = {k: i[k].clone().requires_grad_(True) for k in ("xyz", "sc", "op", "sh")}
        lv["rot"] = None if i["rot"] is None else i["rot"].clone().requires_grad_(True)
        return lv
    lv = leaves()
    A, tr = i["A"].clone().requires_grad_(True), shared.clone().requires_grad_(True)
    m2d = torch.zeros(K, P, 3, device=dev, requires_grad=True)
    color, radii = rasterize_skinned_frames(lv["xyz"], lv["rot"], lv["sc"], lv["op"], lv["sh"], i["w"], A, stacked,
                                            smpl_scale=i["smpl_scale"], transl=tr, means2D=m2d)
    (color * i["dL"]).sum().backward()
    torch.cuda.synchronize()
    acc, tr_sum = {}, None
    for f in range(K):
        l1 = leaves()
        A1, tr1 = i["A"][f].clone().requires_grad_(True), shared.clone().requires_grad_(True)
        m1 = torch.zeros(P, 3, device=dev, requires_grad=True)
        c1, r1 = rasterize_skinned_gaussians(l1["xyz"], l1["rot"], l1["sc"], l1["op"], l1["sh"], i["w"], A1, one[f],
                                             smpl_scale=i["smpl_scale"], transl=tr1, means2D=m1)
        (c1 * i["dL"][f]).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(color[f], c1.detach()) and torch.equal(radii[f], r1), f
        assert torch.equal(A.grad[f], A1.grad) and torch.equal(m2d.grad[f], m1.grad), f
        tr_sum = tr1.grad.clone() if f == 0 else tr_sum + tr1.grad
        for k, v in l1.items():
            if v is not None:
                acc[k] = v.grad.clone() if f == 0 else acc[k] + v.grad
    assert not torch.equal(color[0], color[1]) and int((radii > 0).sum()) > 0
    assert tuple(tr.grad.shape) == (3,) and torch.equal(tr.grad, tr_sum)
    for k in acc:
        assert torch.equal(lv[k].grad, acc[k]) and float(acc[k].abs().max()) > 0, k


def test_frames_with_depth_and_alpha_maps():
    """``SkinnedFramesEngine(aux=True)`` with dL_ddepth and dL_dalpha against two single-frame ``return_aux`` calls, as
    tests/test_gpu_aux_frames.py holds the K-frame maps."""
    from sings_amd.engine import SkinnedFramesEngine
    from sings_amd.skinned import rasterize_skinned_gaussians
    dev = _dev()
    s = _case_17_65_2()
    K, P, J, W, H = s["K"], s["P"], s["J"], s["W"], s["H"]
    i = _frames_inputs(s)
    rs = TS._settings(s, dev, 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    gD, gA = torch.randn(K, 1, H, W, generator=g).to(dev), torch.randn(K, 1, H, W, generator=g).to(dev)
    eng = SkinnedFramesEngine(P, J, W, H, sec.M, K, dev, CAP, with_rot=i["with_rot"], rot_width=i["rw"], aux=True)
    eng.set_camera(rs)
    eng.set_frames(i["xyz"], i["rot"], i["w"], i["A"], i["smpl_scale"], i["transl"])
    eng.forward(i["sh"], i["op"], i["sc"])
    eng.backward(i["sh"], i["op"], i["sc"], i["dL"], dL_ddepth=gD, dL_dalpha=gA)
    torch.cuda.synchronize()
    assert float(eng.alpha.max()) > 0.5 and float(eng.depth.abs().max()) > 0.0
    acc = {}
    for f in range(K):
        lv = dict(d_xyz=i["xyz"].clone().requires_grad_(True), d_scales=i["sc"].clone().requires_grad_(True),
                  d_opacity=i["op"].clone().requires_grad_(True), d_sh=i["sh"].clone().requires_grad_(True),
                  d_rot=None if i["rot"] is None else i["rot"].clone().requires_grad_(True))
        A1, tr1 = i["A"][f].clone().requires_grad_(True), i["transl"][f].clone().requires_grad_(True)
        m1 = torch.zeros(P, 3, device=dev, requires_grad=True)
        c1, r1, d1, a1 = rasterize_skinned_gaussians(lv["d_xyz"], lv["d_rot"], lv["d_scales"], lv["d_opacity"], lv["d_sh"], i["w"], A1, rs,
                                                     smpl_scale=i["smpl_scale"], transl=tr1, means2D=m1, return_aux=True)
        ((c1 * i["dL"][f]).sum() + (d1 * gD[f]).sum() + (a1 * gA[f]).sum()).backward()
        torch.cuda.synchronize()
        for name, a, b in (("color", eng.color[f], c1.detach()), ("radii", eng.radii[f], r1), ("depth", eng.depth[f], d1.detach()),
                           ("alpha", eng.alpha[f], a1.detach()), ("dA", eng.d_A[f], A1.grad), ("dtransl", eng.d_transl[f], tr1.grad),
                           ("means2D", eng.d_means2D[f], m1.grad)):
            assert torch.equal(a, b), (f, name)
        for k, v in lv.items():
            if v is not None:
                acc[k] = v.grad.clone() if f == 0 else acc[k] + v.grad    # the single-frame gradients summed in frame order
    for k, v in acc.items():
        assert torch.equal(getattr(eng, k), v.view_as(getattr(eng, k))) and float(v.abs().max()) > 0, k


# ---- e. inputs inside a NaN-filled buffer -----------------------------------------------------------------------------------------
GAP = 65536


def _inside_nan(tensors):
    """The tensors as contiguous views of ONE flat NaN-filled fp32 buffer: >= GAP NaN floats before, between and after them, every
    view at a multiple of 4 floats (16 bytes: the float4 paths still apply)."""
    up4 = lambda n: (n + 3) // 4 * 4
    total = GAP + sum(up4(t.numel()) + GAP for t in tensors if t is not None)
    buf = torch.full((total,), float("nan"), dtype=torch.float32, device=_dev())
    out, o = [], GAP
    for t in tensors:
        if t is None:
            out.append(None)
            continue
        assert o % 4 == 0
        v = buf[o:o + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + 4 * o and v.data_ptr() % 16 == 0
        out.append(v)
        o += up4(t.numel()) + GAP
    assert o == total and int(torch.isnan(buf).sum()) >= GAP * (len(out) + 1)
    return buf, out


@pytest.mark.parametrize("K,P,J,rot", [(1, 65, 17, "6d"), (3, 65, 17, "mat"), (1, 63, 64, "mat"), (3, 63, 64, "6d")],
                         ids=lambda v: str(v))
def test_inputs_inside_a_nan_filled_buffer(K, P, J, rot):
    from sings_amd.engine import SkinnedEngine, SkinnedFramesEngine
    dev = _dev()
    s = sec.scene(P, J, 500 + J + K, rot, K=None if K == 1 else K)
    rs = TS._settings(s, dev, 0)
    W, H = s["W"], s["H"]
    rotten, with_rot, rw = _rot_args(s)
    plain = [_t(s["w"]), _t(s["A"].reshape(-1, J, 16) if K > 1 else s["A"].reshape(J, 16)), _t(s["xyz"]), rotten, _t(s["scales"])]
    others = dict(op=_t(s["opac"]), sh=_t(s["shs"]), smpl_scale=_t(s["smpl_scale"]), transl=_t(s["transl"]), dL=_t(s["dL"]))

    def run(w, A, xyz, rot_c, sc):
        if K == 1:
            e = SkinnedEngine(P, J, W, H, sec.M, dev, CAP, with_rot=with_rot, rot_width=rw)
            e.set_camera(rs)
            e.set_frame(xyz, rot_c, w, A, others["smpl_scale"], others["transl"])
            posed = tuple(torch.empty(P, n, device=dev) for n in (3, 4, 3))
        else:
            e = SkinnedFramesEngine(P, J, W, H, sec.M, K, dev, CAP, with_rot=with_rot, rot_width=rw)
            e.set_camera(rs)
            e.set_frames(xyz, rot_c, w, A, others["smpl_scale"], others["transl"])
            posed = tuple(torch.empty(K, P, n, device=dev) for n in (3, 4, 3))
        R = e.forward(others["sh"], others["op"], sc, sync_num_rendered=True, posed_out=posed)
        e.backward(others["sh"], others["op"], sc, others["dL"])
        torch.cuda.synchronize()
        return [R, e.color.clone(), e.radii.clone(), *posed, e.d_means2D.clone(), e.d_A.clone(), e.d_transl.clone(), e.grad_flat.clone()]
    want = run(*plain)
    buf, views = _inside_nan(plain)
    got = run(*views)
    names = ("R", "color", "radii", "posed xyz", "posed q", "posed scales", "d_means2D", "d_A", "d_transl", "grad_flat")
    assert got[0] == want[0] and np.all(np.asarray(got[0]) > 0)
    for n, a, b in zip(names[1:], got[1:], want[1:]):
        assert a.dtype == torch.int32 or bool(torch.isfinite(a).all()), n
        assert torch.equal(a, b), n
    assert float(want[7].abs().max()) > 0 and float(want[9].abs().max()) > 0
    for v, t in zip(views, plain):                                    # (the kernels wrote nothing into their inputs)
        assert t is None or torch.equal(v, t)


# ---- f. the scene forward ---------------------------------------------------------------------------------------------------------
def test_scene_forward_with_three_joint_counts():
    """Avatars of (P, J) = (1, 1), (65, 17) and (257, 64) in one K = 2 launch: blocks 1 + 1 + 2, every segment with its own J and
    first block.  Each avatar's posed values equal its own K-frame forward's; the image equals the plain rasterizer's for the
    concatenated posed sets (tests/test_gpu_scene.py's bar, frame by frame)."""
    import test_gpu_scene as SC
    K, W, H = sec.SCENE_K, 64, 48
    avatars = []
    for P, J, seed, rot in sec.SCENE_AVATARS:
        s = sec.scene(P, J, seed, rot, K=K)
        rot_t, _, rw = _rot_args(s)
        canon = dict(xyz_canon=_t(s["xyz"]), rotmat_canon=rot_t, scales=_t(s["scales"]), opacity=_t(s["opac"]), shs=_t(s["shs"]),
                     lbs_weights=_t(s["w"]), active_sh_degree=0)
        avatars.append(dict(canon=canon, A=_t(s["A"].reshape(K, J, 16)), transl=_t(s["transl"]), smpl_scale=_t(s["smpl_scale"]),
                            ext_tfs=None, J=J, rw=None if rot == "iso" else rw, P=P))
    bg = _t(np.array([1.0, 1.0, 1.0], np.float32))
    one, stacked = SC._settings(SC._cameras(W, H, K, focal=375.0), bg)
    eng, posed, Rs = SC._scene(avatars, W, H, K, stacked, CAP)
    assert eng.starts == [0, 1, 66] and eng.P == 323
    own = [SC._alone(a, W, H, K, stacked, CAP) for a in avatars]
    for n_, (a, o) in enumerate(zip(avatars, own)):
        lo_, hi = eng.starts[n_], eng.starts[n_] + a["P"]
        for n in range(3):
            assert torch.isfinite(o[2][n]).all() and torch.equal(posed[n][:, lo_:hi], o[2][n]), (n_, n)
        assert torch.equal(eng.radii_of(n_), o[1]) and int((o[1] > 0).sum()) > 0, n_
    ref = SC._plain(avatars, [o[2] for o in own], one, W, H, CAP)
    for f, (color, radii, R) in enumerate(ref):
        assert 0 < R <= CAP and Rs[f] == R, (f, Rs[f], R)
        assert torch.equal(eng.radii[f], radii) and torch.equal(eng.color[f], color), f
    assert not torch.equal(eng.color[0], eng.color[K - 1])
    # ... and the K-camera rasterizer's (one camera per call: the frames' posed sets differ)
    from sings_amd.engine import RasterFramesEngine
    shs = torch.cat([a["canon"]["shs"] for a in avatars]).contiguous()
    op = torch.cat([a["canon"]["opacity"] for a in avatars]).contiguous()
    plain = RasterFramesEngine(eng.P, W, H, sec.M, 1, _dev(), CAP)
    for f in range(K):
        xyz, q, sc = (torch.cat([o[2][n][f] for o in own]).contiguous() for n in range(3))
        plain.set_camera(one[f])
        assert plain.forward(xyz, shs, op, sc, q, sync_num_rendered=True) == [Rs[f]]
        torch.cuda.synchronize()
        assert torch.equal(eng.color[f], plain.color[0]) and torch.equal(eng.radii[f], plain.radii[0]), f
