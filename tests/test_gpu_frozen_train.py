"""Training across the decoders' thaw (``AvatarTrainer(decoder_schedule=DecoderSchedule(...))``) on the scene and modules of
tests/test_gpu_train_loop.py: twelve steps with ``DecoderSchedule(3, 100, 6, 100)`` -- both decoders frozen for steps 0-2, the appearance
decoder alone for 3-5, everything live from 6 -- through three trainers (torch.optim.Adam eager, FusedAdam eager, FusedAdam inside the
captured graph), and the torch trainer's losses against the same optimiser driven on the CPU by the oracle chain with the frozen decoders
under ``torch.no_grad()`` (the reference's construct, sings_hybrid.py:265-277).

Bars: the loss trajectories agree pairwise, and with the oracle-driven optimiser, to 1e-4 relative at every step (test_gpu_train_loop.py's
and test_gpu_train_loop_fused.py's bar for the same comparisons).  Bitwise: a frozen group's parameters stay what they were, its moments
zero, its step count 0; a capture leaves the optimiser as it found it.  The staged and the joined loss tail of a frozen step give the
same anchor gradient to test_gpu_train_step.py's staged-versus-joined bar (1e-5 of the gradient's scale)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import decode_oracle as do
from oracle import lbs_oracle as lo
from oracle import photo_loss_oracle as plo
from oracle import raster_oracle as ro
from test_gpu_train_loop import H, LRS, W, _CpuReference, _modules, _scene
from test_gpu_train_loop_fused import _bits_equal

pytestmark = pytest.mark.gpu

STEPS = 12
SCHEDULE = (3, 100, 6, 100)
GROUPS = ("xyz", "triplane", "geometry", "appearance")


def _thaw(name):
    """the first step at which the group learns"""
    return {"xyz": 0, "triplane": 3, "geometry": 3, "appearance": 6}[name]


def _trainer(sc, dev, optimizer, use_graph):
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.train_loop import AvatarTrainer, DecoderSchedule
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
    return AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(sc["smpl_scale"]), transl=t(sc["transl"]), use_graph=use_graph,
                         sh_degree=0, max_sh_degree=1, optimizer=optimizer, decoder_schedule=DecoderSchedule(*SCHEDULE))


class _FrozenCpuReference(_CpuReference):
    """``_CpuReference.step`` with the iteration's frozen decoders under ``torch.no_grad()``; torch.optim.Adam skips what has no gradient."""

    def step(self, f, opt_geo, opt_app):
        sc, T = self.sc, self.T
        cam = sc["cam"]
        self.opt.zero_grad(set_to_none=True)
        n = self.xyz.shape[0]
        feats = do.triplane_features(self.xyz, self.grids, self.aabb)
        with torch.set_grad_enabled(opt_geo):
            og = do.geometry_decoder(feats, self.sdg)
        with torch.set_grad_enabled(opt_app):
            oa = do.appearance_decoder(feats, self.sda)
        posed = lo.deform_gaussians(self.xyz + og['xyz_offsets'], torch.eye(3)[None].repeat(n, 1, 1), og['scales'], self.w, T(sc["frames"][f]),
                                    smpl_scale=T(sc["smpl_scale"]), transl=T(sc["transl"]))
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


@pytest.fixture(scope="module")
def runs():
    """The three trainers and the oracle-driven optimiser over the twelve steps, once; what the tests below assert on is recorded here."""
    from sings_amd import decode, rasterizer as rz, train_loop
    from sings_amd.train_loop import DecoderSchedule
    dev = torch.device("cuda:0")
    sc = _scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A = [t(a) for a in sc["frames"]]; gts = [t(g) for g in sc["gts"]]; mask = t(sc["mask"])
    sched = DecoderSchedule(*SCHEDULE)
    current, rec = {}, {"losses": {}, "obs": {}, "captures": [], "flags": [sched.flags(it) for it in range(STEPS)]}

    def snapshot():
        tr = current["trainer"]
        return ([p.detach().clone() for p in tr.params], tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone(), list(tr.opt.steps))

    class Probe(train_loop.CapturedStep):
        """test_gpu_train_loop_fused.py's: the optimiser's state just before a capture and just before the first replay behind it."""

        def __init__(self, module, fn, warmup=3, device=None):
            self.before, self.first = snapshot(), True
            self.flags = (module.opt_geo, module.opt_app)
            super().__init__(module, fn, warmup=warmup, device=device)

        def replay(self):
            if self.first:
                self.first = False
                rec["captures"].append((self.flags, self.before, snapshot()))
            return super().replay()

    original = train_loop.CapturedStep
    train_loop.CapturedStep = Probe
    try:
        for name, optimizer, use_graph in (("torch", "torch", False), ("fused", "fused", False), ("fused_graph", "fused", True)):
            tr = _trainer(sc, dev, optimizer, use_graph)
            current["trainer"] = tr
            if name == "torch":
                ref = _FrozenCpuReference(sc, tr.m.triplane, tr.m.geometry_dec, tr.m.appearance_dec)
                rec["losses"]["cpu"] = []
            groups = {g["name"]: list(g["params"]) for g in tr.opt.param_groups}
            initial = {n: [p.detach().clone() for p in ps] for n, ps in groups.items()}
            out, obs = [], []
            for it in range(STEPS):
                f = it % 8
                out.append(float(tr.step(A[f], gts[f], mask)["loss"]))
                if name == "torch":
                    rec["losses"]["cpu"].append(ref.step(f, *sched.flags(it)))
                row = {"flags": (tr.m.opt_geo, tr.m.opt_app)}
                if optimizer == "fused":
                    views = dict(zip(map(id, tr.opt._params()), zip(tr.opt._moment_views(tr.opt.exp_avg), tr.opt._moment_views(tr.opt.exp_avg_sq))))
                for gi, (n, ps) in enumerate(groups.items()):
                    same = all(_bits_equal(p.detach(), p0) for p, p0 in zip(ps, initial[n]))
                    if optimizer == "fused":
                        zero = all(float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 for m, v in (views[id(p)] for p in ps))
                        count = tr.opt.steps[gi]
                    else:
                        states = [tr.opt.state.get(p, {}) for p in ps]
                        zero = all(len(s) == 0 for s in states)                   # (no state at all: Adam has skipped the parameter so far)
                        counts = {int(float(s["step"])) for s in states if s}
                        assert len(counts) <= 1
                        count = counts.pop() if counts else 0
                    row[n] = dict(same=same, zero=zero, count=count, grads=[p.grad is not None for p in ps])
                obs.append(row)
            rz.check_deferred_overflow(dev)
            rec["losses"][name], rec["obs"][name] = np.array(out), obs
            rz.set_overflow_check("sync"); rz.reset_overflow_state()
            decode.set_gradient_arena(None, None)
            del tr
    finally:
        train_loop.CapturedStep = original
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)
    rec["losses"]["cpu"] = np.array(rec["losses"]["cpu"])
    return rec


def test_frozen_groups_do_not_move_and_thaw_at_step_one(runs):
    assert runs["flags"] == [(False, False)] * 3 + [(True, False)] * 3 + [(True, True)] * 6
    for name, obs in runs["obs"].items():
        for it, row in enumerate(obs):
            assert row["flags"] == runs["flags"][it], (name, it)
            for n in GROUPS:
                o, live_steps = row[n], it + 1 - _thaw(n)
                if live_steps <= 0:                                      # still frozen after step `it`
                    assert o["same"] and o["zero"] and o["count"] == 0, (name, it, n, o)
                    assert not any(o["grads"]), (name, it, n, "a frozen parameter ended the backward with a gradient")
                else:
                    assert not o["same"] and not o["zero"] and o["count"] == live_steps, (name, it, n, o)
                    assert all(o["grads"]), (name, it, n)
        assert not obs[0]["xyz"]["same"] and obs[0]["xyz"]["count"] == 1   # the anchors move from step 0
        assert obs[3]["geometry"]["count"] == 1 and obs[6]["appearance"]["count"] == 1 and obs[3]["triplane"]["count"] == 1


def test_one_capture_per_flag_state_and_a_capture_leaves_the_optimiser_alone(runs):
    caps = runs["captures"]
    assert [c[0] for c in caps] == [(False, False), (True, False), (True, True)], "captured once per flag state"
    for _, (p0, m0, v0, s0), (p1, m1, v1, s1) in caps:
        assert s0 == s1 and _bits_equal(m0, m1) and _bits_equal(v0, v1)
        assert len(p0) == len(p1) and all(_bits_equal(a, b) for a, b in zip(p0, p1))


def test_the_three_trainers_agree(runs):
    losses, worst = runs["losses"], {}
    for a, b in (("torch", "fused"), ("torch", "fused_graph"), ("fused", "fused_graph")):
        rel = np.abs(losses[a] - losses[b]) / np.abs(losses[a])
        worst[(a, b)] = (float(rel.max()), int(rel.argmax()))
    print("loss trajectories: first %.6f last %.6f; max rel " % (losses["torch"][0], losses["torch"][-1])
          + ", ".join(f"{a}-vs-{b} {r:.2e} (step {i})" for (a, b), (r, i) in worst.items()))
    assert losses["torch"][-1] < losses["torch"][0], "the loop optimises"
    for pair, (r, i) in worst.items():
        assert r <= 1e-4, (pair, i, r)


def test_the_trajectory_follows_the_oracle_driven_optimiser(runs):
    e, c = runs["losses"]["torch"], runs["losses"]["cpu"]
    rel = np.abs(e - c) / np.abs(c)
    print(f"loss trajectory: first {c[0]:.6f} last {c[-1]:.6f}; max rel torch-trainer-vs-oracle {rel.max():.2e} (step {rel.argmax()})")
    assert rel.max() <= 1e-4, (rel.argmax(), rel.max())


def test_both_loss_tails_of_a_frozen_step_with_every_regulariser():
    """One step with both decoders frozen, L2Norm, the k-NN term and the mesh terms: the staged tail (``defer_regulariser_join``) and
    the joined one give the same anchor gradient, nothing else gets one, every regulariser's value is reported."""
    from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm
    from sings_amd.topology import MeshState
    from sings_amd.train_step import AvatarStep
    from test_gpu_mesh_terms_train import DEV, START, _cleanup, _mesh_terms, _normals, _settings, _t
    from test_gpu_subdivide_train import _mesh_scene
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topology_golden.npz"))
    sc = _mesh_scene(golden)
    bg, settings = _settings(sc)
    rs = settings(0)
    A, gt, mask = _t(sc["frames"][0]), _t(sc["gts"][0]), _t(sc["mask"])
    mesh = MeshState.from_faces(_t(sc["faces"]), _t(sc["labels"]))
    mt = _mesh_terms()
    mt.reset(mesh, _normals(_t(sc["xyz"]), mesh), _t(sc["xyz"]))
    mt.set_iteration(2 * START)
    tri, geo, app = _modules(DEV)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-4.95)
    step = AvatarStep(_t(sc["xyz"]), _t(sc["w"]), tri, geo, app, l2_norm=L2Norm(), gaussian_connect=GaussiansEdgeLoss(),
                      gaussian_connect_w=0.5, mesh_terms=mt).to(DEV)
    version = step.topology_version
    step.set_trainable(False, False)
    assert step.topology_version == version + 1 and (step.opt_geo, step.opt_app) == (False, False)
    step.set_trainable(False, False)
    assert step.topology_version == version + 1, "no change, no new version"
    params = {n: p for n, p in step.named_parameters() if p.requires_grad}

    def run(defer):
        step.defer_regulariser_join = defer
        for p in params.values():
            p.grad = None
        loss, ld, ex = step(A, rs, gt, mask, bg, smpl_scale=_t(sc["smpl_scale"]), transl=_t(sc["transl"]))
        if loss is None:
            assert defer and "loss_roots" in ex
            loss = step.backward(ld, ex)
        else:
            assert not defer
            loss.backward()
        torch.cuda.synchronize()
        assert [n for n, p in params.items() if p.grad is not None] == ["xyz"]
        for k in ("scales", "scales_aux", "xyz_offsets", "opacity", "shs"):
            assert not ex["attrs"][k].requires_grad, k
        return float(loss.detach()), {k: float(v.detach()) for k, v in ld.items()}, step.xyz.grad.clone()

    try:
        l0, d0, g0 = run(False)
        l1, d1, g1 = run(True)
    finally:
        _cleanup()
    keys = {"l2", "gaussian_connect_loss", "loss", *mt.KEYS}
    assert keys <= set(d0) and set(d0) == set(d1), (sorted(d0), sorted(d1))
    for k in d0:
        print(f"{k}: joined {d0[k]:.9g} staged {d1[k]:.9g}")
        assert abs(d1[k] - d0[k]) <= 1e-6 * abs(d0[k]) + 1e-12, (k, d1[k], d0[k])
    assert abs(l1 - l0) <= 1e-6 * abs(l0)
    err, scale = (g1 - g0).abs().max().item(), g0.abs().max().item()
    print(f"xyz.grad: staged vs joined max err {err:.3e}, scale {scale:.3e}")
    assert scale > 0 and err <= 1e-5 * scale + 1e-12
