"""The body model on the GPU (sings_amd/body_model.py, csrc/sg_body.hip) against the reference's own outputs (tests/golden/
gen_body_golden.py: G-a, its subdivision loop; G-b, its ``lbs``) and against the fp64 twins of tests/test_body_model_host.py.

Floats follow ``body_case.held``: at most twice as far from the fp64 twin as the reference's fp32 result, floor one ulp of the array's
scale.  ``verts``, ``T`` and ``A`` go through kernels that tests/test_gpu_lbs.py already holds: the same tolerances.  The filter is
held to its fp64 twin within four times the error of the twin's own fp32 evaluation (a different summation order, five compounding
iterations)."""
import math

import numpy as np
import pytest
import torch

import body_case as bc
from sings_amd import body_model as BM
from test_body_model_host import flat_two_sided

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_MODELS = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _model(J, B, level=0):
    """The model of (J, B) at a level of the REFERENCE's loop (``body_case.model_arrays``), built once per session."""
    if (J, B, level) not in _MODELS:
        _MODELS[J, B, level] = BM.BodyModel(device=DEV, **bc.model_arrays(J, B, level))
    return _MODELS[J, B, level]


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ---- subdivision ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,B", bc.COMBOS)
def test_subdivision_equals_the_reference(J, B):
    g, pre = bc.golden(), f"J{J}_B{B}_"
    m0 = _model(J, B)
    assert m0.parents[0] == -1 and m0.vertex_id.tolist() == list(range(6)) and m0.edges.shape == (12, 2)
    m1 = m0.subdivided(1, smooth=False)
    m2 = m0.subdivided(2, smooth=False)
    for m, V, level in ((m1, 18, 1), (m2, 66, 2)):
        assert m.num_verts == V and m.posedirs is None and m.num_joints == J and m.num_betas == B
        # integers: equal
        assert np.array_equal(_n(m.faces), g[pre + f"ga_faces_{level}"]) and m.faces.dtype == torch.int32
        assert np.array_equal(_n(m.vertex_id), g[pre + "ga_vertex_id"][:V]) and np.array_equal(_n(m.vertex_label), g[pre + "ga_vertex_label"][:V])
        e = g[pre + f"ga_faces_{level}"].astype(np.int64)
        assert np.array_equal(_n(m.edges), np.unique(np.sort(e[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0))
        # averaged attributes: a mean of two is rounded once -- equal as fp32 values
        assert np.array_equal(_n(m.v_template), g[pre + "ga_verts"][:V])
        assert np.array_equal(_n(m.lbs_weights), g[pre + "ga_lbs_weights"][:V])
        assert np.array_equal(_n(m.shapedirs), g[pre + "ga_shapedirs"][:V])
        rows = _n(m.J_regressor).astype(np.float64).sum(axis=1)
        assert np.abs(rows - 1).max() <= V * 2.0 ** -24                    # V roundings of values that sum to 1
    # the renormalised regressor, each level from the reference's own inputs: the averaged J^T of its previous level
    for level, parent in ((1, m0), (2, _model(J, B, 1))):
        child = parent.subdivided(1, smooth=False)
        ref = g[pre + f"ga_J_regressor_{level}"]
        _, _, at, _ = BM.subdivide_host(_n(parent.v_template), _n(parent.faces), {"Jt": np.ascontiguousarray(_n(parent.J_regressor).T)})
        bc.held(_n(child.J_regressor), ref, BM.renorm_host(at["Jt"]), f"J_regressor level {level} J={J} B={B}")
        again = parent.subdivided(1, smooth=False)
        assert _bits_equal(child.J_regressor, again.J_regressor)
    # smooth as a callable, and the filter by default
    moved = m0.subdivided(1, smooth=lambda v: v + 1.0)
    assert np.array_equal(_n(moved.v_template), g[pre + "ga_verts"][:18] + np.float32(1.0))
    smooth = m0.subdivided(1)
    want = BM.smooth_host(g[pre + "ga_verts"][:18], g[pre + "ga_faces_1"], _n(m1.edges))
    bound = 4 * np.abs(BM.smooth_host(g[pre + "ga_verts"][:18], g[pre + "ga_faces_1"], _n(m1.edges), dtype=np.float32) - want).max()
    assert np.abs(_n(smooth.v_template) - want).max() <= bound and not np.array_equal(_n(smooth.v_template), g[pre + "ga_verts"][:18])


def test_constructor_refuses_outside_the_envelope():
    a = bc.model_arrays(24, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BM.BodyModel(device="cpu", **a)
    cases = {"J > 64": dict(J_regressor=np.ones((65, 6), np.float32) / 6, lbs_weights=np.ones((6, 65), np.float32) / 65, parents=np.arange(-1, 64)),
             "B > 32": dict(shapedirs=np.zeros((6, 3, 33), np.float32)),
             "a face corner": dict(faces=np.array([[0, 1, 6]])),
             "labels": dict(vertex_label=np.zeros(5, np.int64)),
             "posedirs": dict(posedirs=np.zeros((207, 17), np.float32)),
             "weights": dict(lbs_weights=np.zeros((6, 23), np.float32)),
             "not finite": dict(v_template=np.full((6, 3), np.nan, np.float32)),
             "a cycle": dict(parents=np.array([-1, 2, 1] + list(range(2, 23)))),
             "pose_mean": dict(pose_mean=np.zeros(71, np.float32))}
    for what, change in cases.items():
        with pytest.raises(ValueError):
            BM.BodyModel(device=DEV, **dict(a, **change))
    m = BM.BodyModel(device=DEV, **dict(a, parents=np.array([5] + list(a["parents"][1:]))))          # parents[0] is forced to -1
    assert m.parents[0] == -1


# ---- shape, joints, canonical pose against G-b ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("J,B", bc.COMBOS)
def test_shape_and_joints_against_the_reference(J, B, level):
    g, pre, gb = bc.golden(), f"J{J}_B{B}_", bc.gb(J, B)
    a = bc.model_arrays(J, B, level)
    m = _model(J, B, level)
    betas, poses = g[pre + "betas"], g[pre + "poses"]
    J0, JS = m.joint_basis()
    assert m.joint_basis()[0] is J0 and J0.shape == (J, 3) and JS.shape == (J, 3, B)           # computed once, cached
    J0_64, JS_64 = BM.joint_basis_host(a["v_template"], a["shapedirs"], a["J_regressor"])
    for ib in range(2):
        key = f"gb_L{level}_b{ib}_"
        b = _t(betas[ib])
        # the rest joints: the reference's are the posed joints of its t-pose (rotations: the identity to 1e-8)
        bc.held(_n(m.joints_rest(b)), gb[key + "p0_J_transformed"], BM.joints_rest_host(J0_64, JS_64, betas[ib]), f"joints_rest b{ib}")
        for ip in range(3):
            kp = key + f"p{ip}_"
            s = m.shaped(b, _t(poses[ip]))
            tw = BM.shaped_host(a["v_template"], a["shapedirs"], betas[ib:ib + 1], a["posedirs"], poses[ip:ip + 1])
            for name, ref, t64 in (("v_shaped", gb[key + "v_shaped"], tw[0]), ("shape_offsets", gb[key + "shape_offsets"], tw[1]),
                                   ("pose_offsets", gb[kp + "pose_offsets_off0"], tw[2]), ("v_posed", gb[kp + "v_posed_off0"], tw[3])):
                assert s[name].shape == (1, a["v_template"].shape[0], 3)
                if float(np.abs(t64).max()) == 0.0:
                    assert float(s[name].abs().max()) == 0.0 and float(np.abs(ref).max()) == 0.0, name
                else:
                    bc.held(_n(s[name][0]), ref, t64[0], f"{name} L{level} b{ib} p{ip}")
        # without a pose: zero pose offsets (disable_posedirs=True)
        s = m.shaped(b)
        assert float(s["pose_offsets"].abs().max()) == 0.0 and _bits_equal(s["v_posed"], s["v_shaped"])
    # K = 1 and K = 3 rows; [B] and [1,B] agree
    b3 = _t(np.stack([betas[0], betas[1], betas[0]]))
    j3, j1 = m.joints_rest(b3), m.joints_rest(b3[:1])
    assert j3.shape == (3, J, 3) and j1.shape == (1, J, 3)
    want = BM.joints_rest_host(J0_64, JS_64, _n(b3))
    ulp = float(np.spacing(np.float32(np.abs(want).max())))
    assert np.abs(_n(j3) - want).max() <= (B + 2) * ulp and np.abs(_n(j1)[0] - want[0]).max() <= (B + 2) * ulp
    s3 = m.shaped(b3, _t(np.stack([poses[2], poses[1], poses[2]])))
    assert s3["v_posed"].shape == (3, a["v_template"].shape[0], 3) and _bits_equal(s3["v_posed"][0], s3["v_posed"][2])
    assert _bits_equal(s3["v_posed"][1], m.shaped(b3[1], _t(poses[1]))["v_posed"][0])
    # the gradient w.r.t. betas is the analytic basis
    bg = _t(betas[0]).requires_grad_(True)
    wgt = torch.linspace(-1, 1, J * 3, device=DEV).reshape(J, 3)
    (m.joints_rest(bg) * wgt).sum().backward()
    want_g = np.einsum("jcb,jc->b", _n(JS).astype(np.float64), _n(wgt).astype(np.float64))
    assert np.abs(_n(bg.grad) - want_g).max() <= 3 * J * 2.0 ** -23 * np.abs(_n(JS)).max()
    for bad in (b3.cpu(), b3.double(), torch.zeros(B + 1, device=DEV)):
        with pytest.raises((RuntimeError, ValueError)):
            m.joints_rest(bad)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("J,B", bc.COMBOS)
def test_canonical_against_the_reference(J, B, level):
    """``canonical`` is ``lbs`` at the da pose with ``disable_posedirs=False``: pose 1 of G-b."""
    g, pre, gb = bc.golden(), f"J{J}_B{B}_", bc.gb(J, B)
    m = _model(J, B, level)
    body = "smpl" if J == 24 else "smplh"
    assert np.array_equal(_n(m.canonical_pose("da_pose", body)), g[pre + "poses"][1])
    for ib in range(2):
        kp = f"gb_L{level}_b{ib}_p1_"
        c = m.canonical(_t(g[pre + "betas"][ib]), "da_pose", body)
        assert set(c) == {"verts", "A_t2cano", "inv_A_t2cano", "T_t2cano", "inv_T_t2cano", "canonical_offsets", "joints_rest"}
        # the tolerances tests/test_gpu_lbs.py holds the LBS kernel to against the reference's own output
        np.testing.assert_allclose(_n(c["verts"]), gb[kp + "verts_off0"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(_n(c["T_t2cano"]), gb[kp + "T"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(_n(c["A_t2cano"]), gb[kp + "A"], rtol=0, atol=3e-6)
        want = gb[f"gb_L{level}_b{ib}_shape_offsets"].astype(np.float64) + gb[kp + "pose_offsets_off0"]
        assert np.abs(_n(c["canonical_offsets"]) - want).max() <= 2 * float(np.spacing(np.float32(np.abs(want).max())))
        eye = torch.eye(4, device=DEV)
        assert float((c["A_t2cano"] @ c["inv_A_t2cano"] - eye).abs().max()) <= 1e-5
        assert float((c["T_t2cano"] @ c["inv_T_t2cano"] - eye).abs().max()) <= 1e-5
        assert _bits_equal(c["joints_rest"], m.joints_rest(_t(g[pre + "betas"][ib])))
    with pytest.raises(ValueError):
        m.canonical(_t(g[pre + "betas"][0]), "da_pose", "smplh" if J == 24 else "smpl")
    with pytest.raises(ValueError, match="Unknown pose type"):
        m.canonical(_t(g[pre + "betas"][0]), "x_pose", body)
    if J == 52 and level == 0:
        mean = np.linspace(-0.1, 0.1, 156).astype(np.float32)
        mm = BM.BodyModel(device=DEV, **dict(bc.model_arrays(J, B), pose_mean=mean))
        assert np.array_equal(_n(mm.canonical_pose("da_pose", "smplh")), g[pre + "poses"][1] + mean)


def test_level_4_crosses_a_workgroup():
    """1 026 vertices: more than one workgroup's span in the renormalisation, the joint basis and the blend shapes (the filter's
    level 4 is ``test_filter_against_its_twin``).  The reference's loop is recorded for two levels, so here its fp32 arithmetic is
    stood in for by the twins' own fp32 evaluation; the rule is the same."""
    J, B = 24, 10
    g, pre = bc.golden(), f"J{J}_B{B}_"
    m3 = _model(J, B, 2).subdivided(1, smooth=False)
    m4 = m3.subdivided(1, smooth=False)
    assert m3.num_verts == 258 and m4.num_verts == 1026 and int(m4.faces.shape[0]) == 2048
    _, _, at, _ = BM.subdivide_host(_n(m3.v_template), _n(m3.faces), {"Jt": np.ascontiguousarray(_n(m3.J_regressor).T)})
    bc.held(_n(m4.J_regressor), BM.renorm_host(at["Jt"], dtype=np.float32), BM.renorm_host(at["Jt"]), "J_regressor level 4")
    # a model of 1 026 vertices WITH pose correctives
    rs = np.random.RandomState(4)
    a = dict(v_template=_n(m4.v_template), shapedirs=_n(m4.shapedirs), J_regressor=_n(m4.J_regressor), lbs_weights=_n(m4.lbs_weights),
             parents=g[pre + "parents"], faces=_n(m4.faces), vertex_label=_n(m4.vertex_label),
             posedirs=rs.normal(0, 0.01, ((J - 1) * 9, 3 * 1026)).astype(np.float32))
    m = BM.BodyModel(device=DEV, **a)
    J0, JS = m.joint_basis()
    for got, t32, t64, what in zip((J0, JS), BM.joint_basis_host(a["v_template"], a["shapedirs"], a["J_regressor"], dtype=np.float32),
                                   BM.joint_basis_host(a["v_template"], a["shapedirs"], a["J_regressor"]), ("J0", "JS")):
        bc.held(_n(got), t32, t64, f"{what} at 1 026 vertices")
    betas = np.stack([g[pre + "betas"][0], g[pre + "betas"][1], g[pre + "betas"][0]])
    poses = g[pre + "poses"][[2, 1, 2]]
    s = m.shaped(_t(betas), _t(poses))
    t32 = BM.shaped_host(a["v_template"], a["shapedirs"], betas, a["posedirs"], poses, dtype=np.float32)
    t64 = BM.shaped_host(a["v_template"], a["shapedirs"], betas, a["posedirs"], poses)
    for i, name in enumerate(("v_shaped", "shape_offsets", "pose_offsets", "v_posed")):
        assert s[name].shape == (3, 1026, 3) and _bits_equal(s[name][0], s[name][2])
        bc.held(_n(s[name]), t32[i], t64[i], f"{name} at 1 026 vertices, K = 3")
    # the canonical pose against the fp64 chain, with the bound tests/test_gpu_lbs.py holds the LBS kernels to against fp64
    c = m.canonical(_t(betas[1]), "da_pose", "smpl")
    jr = BM.joints_rest_host(*BM.joint_basis_host(a["v_template"], a["shapedirs"], a["J_regressor"]), betas[1])
    A = BM.joint_transforms_host(g[pre + "poses"][1], jr, [int(p) for p in a["parents"]])
    one = BM.shaped_host(a["v_template"], a["shapedirs"], betas[1:2], a["posedirs"], g[pre + "poses"][1:2])
    verts, T = BM.skin_host(A, a["lbs_weights"], one[3][0])
    for got, want, what in ((c["verts"], verts, "verts"), (c["T_t2cano"], T, "T"), (c["A_t2cano"], A, "A")):
        err = np.abs(_n(got).astype(np.float64) - want)
        assert (err <= 2e-5 * np.abs(want) + 2e-6 * np.abs(want).max()).all(), (what, float(err.max()))


# ---- the filter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 4])
def test_filter_against_its_twin(level):
    v, f, e = bc.octa_level(level)
    x64 = BM.smooth_host(v, f, e)
    bound = 4 * float(np.abs(BM.smooth_host(v, f, e, dtype=np.float32) - x64).max())
    verts, faces, edges = _t(v), _t(f), _t(e.astype(np.int32))
    keep = verts.clone()
    out = BM.smooth_filter(verts, faces, edges)
    err = float(np.abs(_n(out).astype(np.float64) - x64).max())
    print(f"level {level} ({len(v)} vertices): device {err:.3e} from the fp64 twin, allowed {bound:.3e}")
    assert out.dtype == torch.float32 and out.shape == verts.shape and err <= bound
    assert _bits_equal(verts, keep)                                            # the input is not written
    assert _bits_equal(out, BM.smooth_filter(verts, faces, edges))             # two runs: the same bits
    assert _bits_equal(out, BM.smooth_filter(verts, faces))                    # the edges it builds itself are these edges
    assert _bits_equal(BM.smooth_filter(verts, faces, edges, iterations=0), verts)
    one = BM.smooth_filter(verts, faces, edges, lamb=0.25, iterations=1)
    assert np.abs(_n(one) - BM.smooth_host(v, f, e, lamb=0.25, iterations=1)).max() <= bound


def test_filter_refuses_and_writes_nothing():
    v, f, e = bc.octa_level(1)
    faces, edges = _t(f), _t(e.astype(np.int32))
    lonely = _t(np.concatenate([v, [[2, 2, 2]]]).astype(np.float32))
    nan = _t(v).clone(); nan[3, 1] = float("nan")
    fv, ff, fe = flat_two_sided()
    for verts, fa, ed, word in ((lonely, faces, edges, "no neighbour"), (nan, faces, edges, "not finite"),
                                (_t(fv), _t(ff), _t(fe.astype(np.int32)), "does not change")):
        keep = verts.clone()
        with pytest.raises(ValueError, match=word):
            BM.smooth_filter(verts, fa, ed)
        assert bool(torch.equal(verts.view(torch.int32), keep.view(torch.int32)))
    bad = faces.clone(); bad[2, 1] = 18
    with pytest.raises((ValueError, IndexError)):
        BM.smooth_filter(_t(v), bad, edges)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BM.smooth_filter(_t(v).cpu(), faces, edges)
    BM.smooth_filter(_t(v), faces, edges)                                      # and the untouched inputs still pass


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_body_to_trainer():
    """``from_body`` at level 2 -> ``fit_initial_attributes`` -> ``AvatarTrainer``; ``PoseTable`` from the canonical dict."""
    from sings_amd.avatar_init import fit_initial_attributes, from_body
    from sings_amd.body import joint_transforms_hip
    from sings_amd.pose import PoseTable
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.train_loop import AvatarTrainer
    from test_gpu_train_loop import H, LRS, W, _modules, _scene
    g, pre = bc.golden(), "J24_B10_"
    a = bc.model_arrays(24, 10)
    a["v_template"] = a["v_template"] * np.array([0.2, 0.42, 0.15], np.float32)                 # inside the tri-plane's box
    body = BM.BodyModel(device=DEV, **a).subdivided(2)
    betas = _t(g[pre + "betas"][0] * np.float32(0.1))
    tri, geo, app = _modules(DEV)
    module, mesh, targets, canon = from_body(body, betas, tri, geo, app, init_opacity=0.83)
    assert mesh.num_verts == body.num_verts == 66 == int(module.xyz.shape[0]) and canon["verts"].shape == (66, 3)
    assert _bits_equal(module.xyz.detach(), canon["verts"])
    first = fit_initial_attributes(module, targets, LRS, init_steps=5, patience=5)
    assert first["losses"].shape[0] == 5 and np.isfinite(first["losses"]).all()
    # the pose table of the kit's poses from what the body model made
    go, bp = _t(g["J24_B10_poses"][:, :3]), _t(g["J24_B10_poses"][:, 3:])
    table = PoseTable.from_axis_angle(go, bp, torch.zeros(3, 3, device=DEV), body.joints_rest(betas), canon["A_t2cano"]).to(DEV)
    by_hand = joint_transforms_hip(_t(g["J24_B10_poses"]), canon["joints_rest"], body.parents) @ canon["inv_A_t2cano"]
    frames = []
    for i in range(3):
        A, _ = table(i)
        assert float((A.detach() - by_hand[i]).abs().max()) <= 2e-5 * max(1.0, float(by_hand[i].abs().max()))
        frames.append(A.detach().contiguous())
    sc = _scene()
    cam = sc["cam"]
    consts = dict(bg=_t(sc["bg"]), view=_t(cam["world_view_transform"]), proj=_t(cam["full_proj_transform"]), campos=_t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    tr = AvatarTrainer(module, settings, consts["bg"], LRS, smpl_scale=_t(sc["smpl_scale"]), transl=_t(sc["transl"]), use_graph=False,
                       sh_degree=0, max_sh_degree=1, optimizer="fused", mesh=mesh)
    for i in range(3):
        ld = tr.step(frames[i], _t(sc["gts"][i]), _t(sc["mask"]))
        assert math.isfinite(float(ld["loss"]))


# ---- the loader -----------------------------------------------------------------------------------------------------------------------
def test_loader_round_trip(tmp_path):
    J, B = 52, 16
    a = bc.model_arrays(J, B)
    rs = np.random.RandomState(2)
    hl, hr = rs.normal(0, 0.1, 45).astype(np.float32), rs.normal(0, 0.1, 45).astype(np.float32)
    np.savez(tmp_path / "model.npz", v_template=a["v_template"], shapedirs=a["shapedirs"], J_regressor=a["J_regressor"], weights=a["lbs_weights"],
             kintree_table=np.stack([a["parents"], np.arange(J)]), f=a["faces"], posedirs=a["posedirs"].T.reshape(6, 3, -1),
             hands_meanl=hl, hands_meanr=hr)
    arrays = BM.load_body_arrays(str(tmp_path / "model.npz"), num_betas=10)
    m = BM.BodyModel.from_arrays(arrays, a["vertex_label"], device=DEV)
    assert m.num_betas == 10 and m.num_joints == J and m.num_verts == 6
    assert np.array_equal(_n(m.shapedirs), a["shapedirs"][:, :, :10]) and np.array_equal(_n(m.posedirs), a["posedirs"])
    assert np.array_equal(_n(m.pose_mean), np.concatenate([np.zeros(66, np.float32), hl, hr]))
    for k in ("v_template", "J_regressor", "lbs_weights"):
        assert np.array_equal(_n(getattr(m, k)), a[k]), k
    assert list(m.parents) == [-1] + [int(p) for p in a["parents"][1:]] and np.array_equal(_n(m.faces), a["faces"])
    with pytest.raises(ValueError, match="chumpy"):
        BM.load_body_arrays(str(tmp_path / "model.pkl"))
    np.savez(tmp_path / "object.npz", **{k: np.array([{"x": 1}], dtype=object) for k in BM.NPZ_KEYS})
    with pytest.raises(ValueError, match="object array"):
        BM.load_body_arrays(str(tmp_path / "object.npz"))
