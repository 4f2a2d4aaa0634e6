"""``AvatarTrainer.densify_and_subdivide`` (the reference's ``hybrid`` densification, sings_hybrid.py:1022-1150) on the small avatar of
tests/test_gpu_train_loop.py with a ``bumpy_sphere`` mesh as anchors: a few steps, the subdivision with thresholds picked from the
run's own statistics, a few more steps -- eager and graph-replayed, with the torch and the fused optimiser -- and the state after a
call driven with the recorded decision of the reference composite (tests/golden/topology_golden.npz, ``comp`` / ``comp_cap``)."""
import math
import os

import numpy as np
import pytest
import torch

from mesh_case import bumpy_sphere
from test_gpu_train_loop import H, LRS, W, _modules, _scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ULP = 2.0 ** -23                                  # relative spacing of fp32 (unit round-off u = ULP / 2)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topology_golden.npz"))


def _mesh_scene(golden):
    """The scene of test_gpu_train_loop with the 86 vertices of bumpy_sphere(12, 8) as anchors (the mesh, labels and skinning weights of
    the golden composite)."""
    sc = _scene()
    v, f, lab = bumpy_sphere(12, 8)
    assert np.array_equal(f, golden["comp_faces"]) and np.array_equal(lab, golden["comp_vertex_label"])
    sc["xyz"] = (v * np.array([0.2, 0.42, 0.15])).astype(np.float32)
    sc["w"] = golden["comp_lbs_weights"]
    sc["faces"], sc["labels"] = f, lab
    return sc


def _trainer(sc, optimizer, use_graph):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.topology import MeshState
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tri, geo, app = _modules(DEV)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-4.95)                           # softplus: about 0.0071, around the 0.008 clip of the interpolation
    mod = AvatarStep(t(sc["xyz"]), t(sc["w"]), tri, geo, app).to(DEV)
    cam = sc["cam"]
    consts = dict(bg=t(sc["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    mesh = MeshState.from_faces(t(sc["faces"]), t(sc["labels"]))
    return AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(sc["smpl_scale"]), transl=t(sc["transl"]), use_graph=use_graph,
                         sh_degree=0, max_sh_degree=1, optimizer=optimizer, mesh=mesh)


def _moments(tr):
    if tr.fused:
        st = tr.opt.state_dict()["state"][0]
    else:
        st = tr.opt.state[tr.m.xyz]
    return st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def _decode(tr):
    from sings_amd import decode
    m = tr.m
    with torch.no_grad():
        return decode.decode_attributes(m.xyz, m.triplane, m.geometry_dec, m.appearance_dec, m.thickness_factor, m.scaling_multiplier)


def _edges_by_torch(faces):
    f = faces.cpu().long()
    e = torch.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    return torch.unique(e, dim=0)


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _check_call(tr, before, result, stale):
    """What must hold after ANY densify_and_subdivide: ``before`` = the state in front of the call."""
    m, mesh = tr.m, tr.mesh
    selected, faces_idx, n_old, n_new = result
    sel_edges = _edges_by_torch(before["faces"][faces_idx.cpu()]).to(DEV)
    E = int(sel_edges.shape[0])
    # N grows by exactly the number of unique edges of the selected faces
    assert n_old == before["xyz"].shape[0] and n_new == n_old + E == int(m.xyz.shape[0]) and E > 0
    assert m.lbs_weights.shape[0] == mesh.vertex_label.shape[0] == mesh.level_id.shape[0] == n_new and mesh.gs_level_mark == [0, n_new]
    assert m.denom.shape[0] == n_new and float(m.denom.abs().max()) == 0.0
    # old anchors and their Adam moments untouched, new moments zero
    assert _bits_equal(m.xyz.detach()[:n_old], before["xyz"])
    for new, old in zip(_moments(tr), before["moments"]):
        assert float(old.abs().max()) > 0 and _bits_equal(new[:n_old], old) and float(new[n_old:].abs().max()) == 0.0
    assert tr.opt.param_groups[0]["params"][0] is m.xyz
    # the new anchors: midpoints of xyz_canon (anchor + offset) of the edges, in the edges' lexicographic order
    a, b = sel_edges[:, 0], sel_edges[:, 1]
    xc = before["attrs"]["xyz_canon"]
    assert _bits_equal(m.xyz.detach()[n_old:], (xc[a] + xc[b]) * 0.5)
    # skinning weights: the endpoints' mean; rows still sum to 1.  In exact arithmetic the mean of two rows that sum to s_a, s_b sums
    # to (s_a + s_b) / 2; each of its J entries is rounded once (<= u relative, u = 2^-24), so the fp64 sum of the stored row is within
    # u = ulp / 2 of that; the input rows (w / w.sum() in fp32) are within 1.5 ulp of 1 themselves (checked): 2 ulp in all.
    w = m.lbs_weights.double()
    assert float((before["w"].double().sum(1) - 1).abs().max()) <= 1.5 * ULP
    assert _bits_equal(m.lbs_weights[:n_old], before["w"]) and _bits_equal(m.lbs_weights[n_old:], (before["w"][a] + before["w"][b]) * 0.5)
    assert float((w.sum(1) - 1).abs().max()) <= 2 * ULP
    # labels of the new vertices: the smaller endpoint's
    assert mesh.vertex_label.dtype == torch.int32
    assert torch.equal(mesh.vertex_label[:n_old], before["labels"]) and torch.equal(mesh.vertex_label[n_old:], before["labels"][a])
    # the faces: F + 3 Fs of them, and `edges` = the unique sorted rows of ALL new faces
    Fs = int(torch.unique(faces_idx).shape[0])
    assert mesh.faces.shape[0] == before["faces"].shape[0] + 3 * Fs and int(mesh.faces.max()) == n_new - 1
    assert torch.equal(mesh.edges.cpu().long(), _edges_by_torch(mesh.faces))
    # scaling_multiplier: per-Gaussian [N,1]; a selected old row times mean_scale / scale, an unselected one kept.  fp32 mean over n
    # values: <= n u relative; the division and the product one rounding each
    sm = m.scaling_multiplier
    assert tuple(sm.shape) == (n_new, 1)
    sc = (before["attrs"]["scales"] * tr.smpl_scale.reshape(1, -1))[:, :1].double()
    want = torch.where(selected.to(DEV).reshape(-1, 1), sc.mean() / sc, torch.ones_like(sc))
    assert float(((sm[:n_old].double() - want) / want).abs().max()) <= (n_old + 4) * ULP / 2
    # the decoded mean scale of every new Gaussian equals the clipped interpolated scale.  new multiplier r = fl(t / mean3(s)) with
    # t the interpolated scale and s the decoded scale at multiplier 1; decoded again: mean3(fl(s r)).  mean3 of three equal values is
    # a sum with one rounding (2x is exact) and a division (or a product with a rounded 1/3: <= 1.5 u): <= 2.5 u each, twice; the
    # division and the product u each: 7 u < 4 ulp relative.
    after = _decode(tr)
    interp = tr.last_subdivision["interpolated_scales"]
    src = (before["attrs"]["scales"] * tr.smpl_scale.reshape(1, -1))[:, :1].mean(-1).clamp(max=0.008)
    assert _bits_equal(interp, (src[a] + src[b]) * 0.5)
    rel = ((after["scales"][n_old:].mean(-1) - interp) / interp).abs().max()
    print(f"new rows: decoded mean scale vs interpolated, max rel {float(rel) / ULP:.2f} ulp; clipped sources "
          f"{float((src == 0.008).float().mean()):.2f}")
    assert float(rel) <= 4 * ULP
    # opacity reset on the new set: no opacity below 0.5
    off = m.appearance_dec.opacity_offset
    assert torch.is_tensor(off) and off.shape[0] == n_new and float(after["opacity"].min()) >= 0.5 - 1e-6
    # the stale graph refuses; the trainer dropped it
    assert tr.captured is None
    if stale is not None:
        with pytest.raises(RuntimeError, match="capture the step again"):
            stale.replay()


def _state(tr):
    m = tr.m
    return dict(xyz=m.xyz.detach().clone(), w=m.lbs_weights.clone(), labels=tr.mesh.vertex_label.clone(), faces=tr.mesh.faces.cpu().long(),
                moments=_moments(tr), attrs=_decode(tr))


@pytest.mark.parametrize("optimizer,use_graph", [("torch", False), ("torch", True), ("fused", False), ("fused", True)])
def test_steps_subdivision_steps(golden, optimizer, use_graph):
    from sings_amd import decode, rasterizer as rz
    from sings_amd.train_loop import CapturedStep
    sc = _mesh_scene(golden)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    A = [t(a) for a in sc["frames"]]; gts = [t(g) for g in sc["gts"]]; mask = t(sc["mask"])
    try:
        tr = _trainer(sc, optimizer, use_graph)
        assert tr.mesh.edges.shape[0] == 3 * len(sc["faces"]) // 2
        losses = [float(tr.step(A[i], gts[i], mask)["loss"]) for i in range(4)]
        stale = tr.captured
        assert (stale is not None) == use_graph and (stale is None or isinstance(stale, CapturedStep))
        # thresholds from the run's own statistics: the upper 40 % by gradient among the upper 70 % by scale
        before = _state(tr)
        g = (tr.m.xyz_gradient_accum / tr.m.denom.clamp_min(1)).reshape(-1)
        assert float(tr.m.denom.max()) == 4.0
        s = (before["attrs"]["scales"] * tr.smpl_scale.reshape(1, -1))[:, 0]
        gthr, sthr = float(torch.quantile(g, 0.605)), float(torch.quantile(s, 0.3))
        result = tr.densify_and_subdivide(gthr, sthr, max_n_gs=10 ** 6)
        selected = result[0]
        hands = torch.isin(before["labels"], torch.tensor([6, 7], dtype=torch.int32, device=DEV))
        assert 0 < int(selected.sum()) < 86 and not bool((selected & hands).any())
        assert torch.equal(selected, (g > gthr) & (s > sthr) & ~hands)
        _check_call(tr, before, result, stale)
        losses += [float(tr.step(A[i], gts[i], mask)["loss"]) for i in range(4, 7)]
        assert all(math.isfinite(x) for x in losses), losses
        assert int(tr.m.xyz.grad.shape[0]) == result[3]
        if use_graph:
            rz.check_deferred_overflow(DEV)
            assert tr.captured is not None and tr.captured.version == tr.m.topology_version
    finally:
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)


@pytest.mark.parametrize("name", ["comp", "comp_cap"])
def test_driven_with_the_reference_decision(golden, name):
    """``decision=``: the recorded masks and faces of the reference composite.  What the decision, the mesh, the labels and the weights
    determine -- faces, labels, weights, edges, N -- equals the composite's; what the network determines is held to ``_check_call``."""
    from sings_amd import decode, rasterizer as rz
    sc = _mesh_scene(golden)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    A = [t(a) for a in sc["frames"]]; gts = [t(g) for g in sc["gts"]]; mask = t(sc["mask"])
    try:
        tr = _trainer(sc, "fused" if name == "comp" else "torch", False)
        for i in range(2):
            tr.step(A[i], gts[i], mask)
        before = _state(tr)
        dec = (torch.from_numpy(golden[f"{name}_selected_pts_mask"].astype(bool)), torch.from_numpy(golden[f"{name}_selected_faces_idx"]).long())
        result = tr.densify_and_subdivide(0.0, 0.0, decision=dec)
        _check_call(tr, before, result, None)
        assert result[3] == len(golden[f"{name}_sub_vertices"])
        assert np.array_equal(tr.mesh.faces.cpu().numpy(), golden[f"{name}_sub_faces"])
        assert np.array_equal(tr.mesh.vertex_label.cpu().numpy(), golden[f"{name}_new_vertex_label"])
        assert np.array_equal(tr.m.lbs_weights.cpu().numpy().view(np.uint32), golden[f"{name}_new_lbs_weights"].view(np.uint32))
        assert np.array_equal(tr.mesh.edges.cpu().numpy(), golden[f"{name}_new_edges"])
        assert float(tr.mesh.level_id.abs().max()) == 0.0
        ld = tr.step(A[2], gts[2], mask)
        assert math.isfinite(float(ld["loss"]))
    finally:
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)


def test_needs_a_mesh(golden):
    from sings_amd import decode, rasterizer as rz
    sc = _mesh_scene(golden)
    try:
        tr = _trainer(sc, "torch", False)
        tr.mesh = None
        with pytest.raises(RuntimeError, match="mesh=MeshState"):
            tr.densify_and_subdivide(1.0, 1.0)
    finally:
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)
