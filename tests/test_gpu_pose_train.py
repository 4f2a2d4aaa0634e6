"""Per-frame poses learned INSIDE the training step (``AvatarTrainer(poses=PoseTable(...)).step_frames``): the small scene of
tests/test_gpu_train_loop.py with J = 24 and eight frames whose targets are rendered with the TRUE poses, the tables started from
perturbed rows, 35 Adam steps round-robin over frames 0..6 (frame 7 is held out) -- for ``optimizer="torch"`` and ``"fused"``, each eager
and replayed from a HIP graph that is captured at one frame index and replayed at all the others -- against the same Adam driven on the
CPU by the oracle chain, the pose -> A part restated in tests/pose_case.py.

Bounds (tests/test_gpu_train_loop.py's header: both sides compute in fp32 with different summation orders, Adam divides by
sqrt(v) + 1e-15): the per-step loss within 1e-4 relative of the CPU trajectory, and within 1e-4 relative between eager and graph.
The test prints the measured maxima (3.0e-5 against the CPU trajectory, at step 5, in all four runs: a third of the bound; at five
times this pose rate the difference grows with the step to 9e-5 by step 34, which left no margin).  What bites on the pose gradient itself: the first step's dense table gradients against the CPU
chain's under the bound tests/test_gpu_skinned.py sets for dL/dA through the rasterizer (the tables' gradient is a linear map of it),
and every visited frame's loss at its last visit below its first.

Bitwise: the rows of the held-out frame never move (zero gradient, zero moments: Adam's update is exactly 0), and a densify / prune in
the middle of a run leaves the pose tables and their moments as they were."""
import math

import numpy as np
import pytest
import torch

import pose_case as pc
from oracle import decode_oracle as do
from oracle import lbs_oracle as lo
from oracle import photo_loss_oracle as plo
from oracle import raster_oracle as ro
from test_gpu_train_loop import H, J, LRS, W, _CpuReference, _modules, _pick_thresholds, _scene

pytestmark = pytest.mark.gpu

STEPS, VISITED, HELD_OUT = 35, 7, 7
POSE_LRS = dict(LRS, global_orient=1e-4, body_pose=1e-4)     # lr.smpl_pose of every config the reference ships


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _pose_scene():
    """The loop test's scene + a body: rest joints, a rigid A_t2cano per joint, true axis-angle poses and translations of eight frames,
    and the perturbed 6-D rows the tables start from."""
    from oracle import rotations_oracle as rot
    sc = _scene()
    rs = np.random.RandomState(23)
    sc["joints"] = rs.normal(0, 0.25, (J, 3)).astype(np.float32) * np.array([0.45, 0.9, 0.3], np.float32)
    sc["parents"] = tuple(int(p) for p in lo.SMPL_PARENTS)
    t2c = np.tile(np.eye(4, dtype=np.float32), (J, 1, 1))
    t2c[:, :3, :3] = lo.batch_rodrigues(torch.from_numpy(rs.normal(0, 0.1, (J, 3)).astype(np.float32))).numpy()
    t2c[:, :3, 3] = rs.normal(0, 0.02, (J, 3))
    sc["post"] = np.linalg.inv(t2c.astype(np.float64)).astype(np.float32)
    aa = rs.normal(0, 0.2, (8, J, 3)).astype(np.float32)
    d6 = rot.axis_angle_to_rotation_6d(torch.from_numpy(aa)).numpy()
    sc["true_go"], sc["true_bp"] = d6[:, 0].copy(), d6[:, 1:].reshape(8, 138).copy()
    sc["start_go"] = (sc["true_go"] + 0.02 * rs.normal(0, 1, (8, 6))).astype(np.float32)
    sc["start_bp"] = (sc["true_bp"] + 0.02 * rs.normal(0, 1, (8, 138))).astype(np.float32)
    sc["transl_rows"] = (sc["transl"][None] + rs.normal(0, 0.01, (8, 3))).astype(np.float32)
    return sc


def _table(sc, dev, start=True):
    from sings_amd.pose import PoseTable
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    k = "start" if start else "true"
    return PoseTable(t(sc[k + "_go"]), t(sc[k + "_bp"]), t(sc["transl_rows"]), t(sc["joints"]), t(sc["post"]), sc["parents"])


def _trainer(sc, dev, optimizer, use_graph, lrs=POSE_LRS, poses="start"):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tri, geo, app = _modules(dev)
    mod = AvatarStep(t(sc["xyz"]), t(sc["w"]), tri, geo, app).to(dev)
    cam = sc["cam"]
    consts = dict(bg=t(sc["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    table = None if poses is None else _table(sc, dev, poses == "start")
    tr = AvatarTrainer(mod, settings, consts["bg"], lrs, smpl_scale=t(sc["smpl_scale"]), use_graph=use_graph, sh_degree=0, max_sh_degree=1,
                       optimizer=optimizer, poses=table)
    return tr, (tri, geo, app)


def _targets(sc, dev):
    """The eight frames rendered with the TRUE poses by the untrained model (the photometric loss clamps its prediction: so here)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tr, _ = _trainer(sc, dev, "torch", False, poses="true")
    gts = []
    with torch.no_grad():
        for f in range(8):
            A, row = tr.poses(f)
            _, _, ex = tr.m(A, tr.rs, torch.zeros(3, H, W, device=dev), t(sc["mask"]), tr.bg, smpl_scale=tr.smpl_scale, transl=row)
            gts.append(ex["render_raw"].clamp(0, 1).cpu().numpy())
    return gts


class _CpuPoseReference(_CpuReference):
    """tests/test_gpu_train_loop.py's CPU model with the two pose tables as parameters: A of a step is the row's, through pose_case."""

    def __init__(self, sc, tri, geo, app):
        super().__init__(sc, tri, geo, app)
        T = self.T
        self.go = T(sc["start_go"]).clone().requires_grad_(True)
        self.bp = T(sc["start_bp"]).clone().requires_grad_(True)
        self.opt.add_param_group({"params": [self.go], "lr": POSE_LRS["global_orient"]})
        self.opt.add_param_group({"params": [self.bp], "lr": POSE_LRS["body_pose"]})

    def step(self, f):
        sc, T = self.sc, self.T
        cam = sc["cam"]
        self.opt.zero_grad(set_to_none=True)
        n = self.xyz.shape[0]
        feats = do.triplane_features(self.xyz, self.grids, self.aabb)
        og = do.geometry_decoder(feats, self.sdg); oa = do.appearance_decoder(feats, self.sda)
        A, _ = pc.pose_to_A(self.go[f:f + 1], self.bp[f:f + 1], T(sc["joints"]), sc["parents"], T(sc["post"]))
        posed = lo.deform_gaussians(self.xyz + og['xyz_offsets'], torch.eye(3)[None].repeat(n, 1, 1), og['scales'], self.w, A[0],
                                    smpl_scale=T(sc["smpl_scale"]), transl=T(sc["transl_rows"][f]))
        pxyz, prot, psc, _ = posed
        o = ro.forward(pxyz.detach().numpy(), oa['opacity'].detach().numpy(), cam["world_view_transform"], cam["full_proj_transform"],
                       cam["camera_center"], W, H, math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), sc["bg"],
                       scales=psc.detach().numpy(), rotations=prot.detach().numpy(), shs=oa['shs'].detach().numpy(), sh_degree=self.sh_degree)
        img = T(o["color"]).requires_grad_(True)
        pl = plo.photometric_loss(img, T(sc["gts"][f]), T(sc["mask"]), T(sc["bg"]), 0.8, 0.2)
        loss = pl["l1"] + pl["ssim"]
        loss.backward()
        g = ro.backward(o, img.grad.numpy())
        pairs = [(pxyz, T(g["dL_dmeans3D"])), (psc, T(g["dL_dscales"])), (prot, T(g["dL_drots"])),
                 (oa['opacity'], T(g["dL_dopacity"]).reshape(n, 1)), (oa['shs'], T(g["dL_dsh"]).reshape(n, 16, 3))]
        pairs = [(a, b) for a, b in pairs if a.requires_grad]
        torch.autograd.backward([a for a, _ in pairs], [b for _, b in pairs])
        self.opt.step()
        return float(loss.detach())


def test_poses_are_learned_in_the_step_eager_and_graph_both_optimisers():
    from sings_amd import decode, rasterizer as rz
    dev = torch.device("cuda:0")
    sc = _pose_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    try:
        sc["gts"] = _targets(sc, dev)
        gts = [t(g) for g in sc["gts"]]; mask = t(sc["mask"])
        losses, tables, grads0 = {}, {}, {}
        ref = None
        for optimizer in ("torch", "fused"):
            for use_graph in (False, True):
                name = f"{optimizer}_{'graph' if use_graph else 'eager'}"
                tr, mods = _trainer(sc, dev, optimizer, use_graph)
                if ref is None:
                    ref = _CpuPoseReference(sc, *mods)                    # (every trainer starts from the same seeded modules)
                assert [g["name"] for g in tr.opt.param_groups][-2:] == ["global_orient", "body_pose"]
                assert all(any(p is q for p in tr.params) for q in (tr.poses.global_orient, tr.poses.body_pose))
                start = [p.detach().clone() for p in (tr.poses.global_orient, tr.poses.body_pose)]
                out, captured_at = [], None
                for it in range(STEPS):
                    f = it % VISITED
                    out.append(float(tr.step_frames(f, gts[f], mask)["loss"]))
                    if it == 0:                                           # (an eager step in every variant: the tables' .grad is the step's)
                        grads0[name] = [p.grad.detach().cpu().numpy().copy() for p in (tr.poses.global_orient, tr.poses.body_pose)]
                    if use_graph and tr.captured is not None and captured_at is None:
                        captured_at, graph = (it, f), tr.captured
                rz.check_deferred_overflow(dev)
                if use_graph:                                             # ONE capture, at one frame index, replayed at all the others
                    assert captured_at is not None and tr.captured is graph and STEPS - captured_at[0] > VISITED
                    print(f"{name}: captured at step {captured_at[0]} (frame {captured_at[1]}), replayed for {STEPS - captured_at[0]} steps")
                losses[name] = np.array(out)
                now = [p.detach().clone() for p in (tr.poses.global_orient, tr.poses.body_pose)]
                tables[name] = now
                for a, b in zip(start, now):
                    assert _bits_equal(a[HELD_OUT], b[HELD_OUT]), "the rows of a frame that is never visited stay bit-identical"
                    assert all(not torch.equal(a[f], b[f]) for f in range(VISITED)), "visited rows move"
                if optimizer == "fused":
                    assert tr.opt.steps == [STEPS] * 6
                rz.set_overflow_check("sync"); rz.reset_overflow_state()
                decode.set_gradient_arena(None, None)
                del tr
        c = []
        for it in range(STEPS):
            c.append(ref.step(it % VISITED))
            if it == 0:
                ref_grads0 = [p.grad.numpy().copy() for p in (ref.go, ref.bp)]
        c = np.array(c)
    finally:
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)
    print(f"loss trajectory (CPU): first {c[0]:.6f} last {c[-1]:.6f}")
    worst = {}
    for name, e in losses.items():
        rel = np.abs(e - c) / np.abs(c)
        worst[name + " vs cpu"] = (float(rel.max()), int(rel.argmax()))
        print(f"{name} vs cpu, per step: " + " ".join(f"{r:.1e}" for r in rel))
    for optimizer in ("torch", "fused"):
        e, g = losses[optimizer + "_eager"], losses[optimizer + "_graph"]
        rel = np.abs(e - g) / np.abs(e)
        worst[f"{optimizer} eager vs graph"] = (float(rel.max()), int(rel.argmax()))
    print("max relative loss difference: " + ", ".join(f"{k} {r:.2e} (step {i})" for k, (r, i) in worst.items()))
    # the learned tables against the CPU's (not bounded: Adam's sign-like first steps amplify rounding; printed for LAB.md)
    for name, (go, bp) in tables.items():
        print(f"{name}: max |table - cpu table| global_orient {float((go.cpu() - ref.go.detach()).abs().max()):.2e}, "
              f"body_pose {float((bp.cpu() - ref.bp.detach()).abs().max()):.2e}")
    # the first step's dense table gradients against the CPU chain's, before Adam's sign-like steps can amplify anything: the bound
    # tests/test_gpu_skinned.py:157 sets for dL/dA through the skinned rasterizer against this oracle (2e-3 relative + 2e-4 of the
    # largest entry); the tables' gradient is a linear map of dL/dA, so it inherits that bound
    for name, gs in grads0.items():
        for table, a, b in zip(("global_orient", "body_pose"), gs, ref_grads0):
            assert np.abs(b[0]).max() > 0 and not a[1:].any() and not b[1:].any(), (name, table)
            excess = np.abs(a - b) / (2e-3 * np.abs(b) + 2e-4 * np.abs(b).max())
            print(f"{name}: step-0 d_{table} against the CPU chain: worst entry at {excess.max():.3f} of the bound")
            assert excess.max() <= 1.0, (name, table, float(excess.max()))
    # the loop optimises: every visited frame's loss at its last visit is below its first visit's (the same frame both times)
    assert c[-1] < c[0], "the loop optimises"
    for name, e in dict(losses, cpu=c).items():
        assert e[-1] < e[0], name
        for f in range(VISITED):
            visits = e[f::VISITED]
            assert visits[-1] < visits[0], (name, f, visits)
    print("loss per frame, first -> last visit (CPU): " + ", ".join(f"{f}: {c[f]:.4f} -> {c[f::VISITED][-1]:.4f}" for f in range(VISITED)))
    for k, (r, i) in worst.items():
        assert r <= 1e-4, (k, i, r)
    assert _bits_equal(ref.go.detach()[HELD_OUT], torch.from_numpy(sc["start_go"][HELD_OUT]))


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
def test_densify_leaves_the_pose_groups_alone(optimizer):
    """Six steps, one densify / prune, six more: the remap of the anchors' moments does not touch the pose tables or their moments
    (bitwise), the graph is captured again for the new set, and training goes on."""
    from sings_amd import decode, rasterizer as rz
    from sings_amd.train_loop import densify_decision
    dev = torch.device("cuda:0")
    sc = _pose_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs = np.random.RandomState(3)
    gts = [t(rs.uniform(0, 1, (3, H, W)).astype(np.float32)) for _ in range(8)]; mask = t(sc["mask"])

    def moments(tr):
        if optimizer == "fused":
            st = tr.opt.state_dict()["state"]
            at = [i for i, p in enumerate(tr.params) if p is tr.poses.global_orient or p is tr.poses.body_pose]
            return [st[i][k].clone() for i in at for k in ("exp_avg", "exp_avg_sq")]
        return [tr.opt.state[p][k].clone() for p in (tr.poses.global_orient, tr.poses.body_pose) for k in ("exp_avg", "exp_avg_sq")]
    try:
        tr, _ = _trainer(sc, dev, optimizer, True)
        for it in range(6):
            tr.step_frames(it % 8, gts[it % 8], mask)
        old_graph = tr.captured
        assert old_graph is not None
        m = tr.m
        with torch.no_grad():
            attrs = decode.decode_attributes(m.xyz, m.triplane, m.geometry_dec, m.appearance_dec, m.thickness_factor, m.scaling_multiplier)
        max_grad, min_op = _pick_thresholds(m.xyz_gradient_accum, m.denom, attrs["opacity"])
        dec = densify_decision(m.xyz_gradient_accum, m.denom, attrs["scales"], attrs["opacity"], max_grad, 1.0, min_op, 1e9)
        rows0 = [p.detach().clone() for p in (tr.poses.global_orient, tr.poses.body_pose)]
        mom0 = moments(tr)
        assert all(float(x.abs().max()) > 0 for x in mom0)
        clone, prune, n0, n1 = tr.densify_and_prune(max_grad, 1.0, min_op, 1e9, decision=dec)
        assert n1 != n0 and tr.captured is None
        assert all(_bits_equal(a, b) for a, b in zip(rows0, [tr.poses.global_orient.detach(), tr.poses.body_pose.detach()]))
        assert all(_bits_equal(a, b) for a, b in zip(mom0, moments(tr)))
        assert all(any(p is q for p in tr.params) for q in (tr.poses.global_orient, tr.poses.body_pose))
        with pytest.raises(RuntimeError, match="capture the step again"):
            old_graph.replay()
        out = [float(tr.step_frames(it % 8, gts[it % 8], mask)["loss"]) for it in range(6, 12)]
        rz.check_deferred_overflow(dev)
        assert np.isfinite(out).all() and tr.captured is not None and tr.captured.version == tr.m.topology_version
        assert not _bits_equal(rows0[1], tr.poses.body_pose.detach()), "the tables keep learning after the change"
        assert int(tr.m.xyz.grad.shape[0]) == n1
    finally:
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)


def test_staged_backward_reaches_the_pose_tables():
    """``AvatarStep(defer_regulariser_join=True)`` stages its backward by hand: the learned pose's dL/dA and dL/dtransl are handed on
    like the decoded attributes' gradients.  Same kernels on the same inputs either way (the per-joint reduction of dL/dA is fixed-order):
    the table gradients of the staged pass equal those of one plain autograd pass to fp32 rounding of the loss terms' hand-over
    (1e-6 of the largest entry)."""
    from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField
    from sings_amd.pose import PoseTable
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm
    from sings_amd.scene import avatar_scene
    from sings_amd.train_step import AvatarStep
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    s = avatar_scene(N=5000, J=24, W=96, H=160, seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [16, 16, 16], 'multires': [1, 2]}
    tri = HexPlaneField(cfg, bounds=1.2, device=dev); geo = GeometryDecoder(64).to(dev); app = AppearanceDecoder(64).to(dev)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-4.5); geo.xyz_offsets.weight.mul_(0.01); geo.xyz_offsets.bias.zero_()
    step = AvatarStep(t(s["xyz_canon"]), t(s["lbs_weights"]), tri, geo, app, l2_norm=L2Norm(), gaussian_connect=GaussiansEdgeLoss(),
                      gaussian_connect_w=1.0).to(dev)
    cam = s["cam"]
    rset = GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=t(s["bg"]),
        scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]), projmatrix=t(cam["full_proj_transform"]), sh_degree=0,
        campos=t(cam["camera_center"]), prefiltered=False, debug=False)
    rs = np.random.RandomState(2)
    aa = rs.normal(0, 0.15, (3, 72)).astype(np.float32)
    pt = PoseTable.from_axis_angle(t(aa[:, :3]), t(aa[:, 3:]), t(np.tile(s["transl"].reshape(1, 3), (3, 1))), t(s["joints_rest"]),
                                   parents=tuple(int(p) for p in s["parents"]), learn_transl=True)
    gt = torch.rand(3, s["H"], s["W"], device=dev); ones = torch.ones(s["H"], s["W"], device=dev)
    params = [pt.global_orient, pt.body_pose, pt.transl]

    def run(defer):
        step.defer_regulariser_join = defer
        for p in list(step.parameters()) + params:
            p.grad = None
        A, row = pt(1)
        loss, ld, ex = step(A, rset, gt, ones, t(s["bg"]), smpl_scale=t(s["smpl_scale"]), transl=row)
        if loss is None:
            assert defer
            loss = step.backward(ld, ex)
        else:
            loss.backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in params]
    plain, staged = run(False), run(True)
    for p, a, b in zip(params, staged, plain):
        assert float(b[1].abs().max()) > 0 and not b[0].any() and not b[2].any()
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), tuple(p.shape)
