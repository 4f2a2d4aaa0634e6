"""The training loop of tests/test_gpu_train_loop.py with the fused optimiser (``AvatarTrainer(optimizer="fused")``): three trainers --
torch.optim.Adam eager, FusedAdam eager, FusedAdam inside the captured HIP graph -- over the same 40 steps, a learning-rate schedule on
the anchors, and ONE shared densify / prune + SH-degree change at step 20.

The loss trajectories agree pairwise to 1e-4 relative at every step: that file's own bar for its eager-against-graph comparison (the
tri-plane backward adds with float atomics, so no two runs are bit-identical).  What IS bitwise: a capture leaves parameters, moments
and step counts as it found them, and a densify re-indexes the anchors' moments with the ``cat(...)[keep]`` expression."""
import math

import numpy as np
import pytest
import torch

from test_gpu_train_loop import CHANGE_AT, H, LRS, STEPS, W, _modules, _pick_thresholds, _scene

pytestmark = pytest.mark.gpu


def _trainer(sc, dev, optimizer, use_graph, schedules, fp=None):
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
    return AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(sc["smpl_scale"]), transl=t(sc["transl"]), use_graph=use_graph,
                         sh_degree=0, max_sh_degree=1, optimizer=optimizer, lr_schedules=schedules, fp=fp)


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def test_three_trainers_forty_steps_one_shared_decision(monkeypatch):
    from sings_amd import decode, rasterizer as rz, train_loop
    from sings_amd.optim import FusedAdam, expon_lr
    dev = torch.device("cuda:0")
    sc = _scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A = [t(a) for a in sc["frames"]]; gts = [t(g) for g in sc["gts"]]; mask = t(sc["mask"])
    schedule = expon_lr(LRS["xyz"], LRS["xyz"] * 0.05, max_steps=STEPS)
    current = {}

    def snapshot():
        tr = current["trainer"]
        return ([p.detach().clone() for p in tr.params], tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone(), list(tr.opt.steps))

    class Probe(train_loop.CapturedStep):
        """Records the optimiser's state just before a capture and just before the first replay that follows it."""
        log = []

        def __init__(self, module, fn, warmup=3, device=None):
            self.before, self.first = snapshot(), True
            super().__init__(module, fn, warmup=warmup, device=device)

        def replay(self):
            if self.first:
                self.first = False
                Probe.log.append((self.before, snapshot()))
            return super().replay()
    monkeypatch.setattr(train_loop, "CapturedStep", Probe)

    losses, shared, sizes = {}, {}, {}
    try:
        for name, optimizer, use_graph in (("torch", "torch", False), ("fused", "fused", False), ("fused_graph", "fused", True)):
            tr = _trainer(sc, dev, optimizer, use_graph, {"xyz": schedule})
            current["trainer"] = tr
            assert isinstance(tr.opt, FusedAdam) == (optimizer == "fused")
            assert (tr.flat is not None) == (optimizer == "fused")                # today's arguments: no arena without fp
            out = []
            for it in range(STEPS):
                f = it % 8
                if it == CHANGE_AT:
                    m = tr.m
                    if not shared:                                                     # the first trainer decides for all three
                        with torch.no_grad():
                            attrs = decode.decode_attributes(m.xyz, m.triplane, m.geometry_dec, m.appearance_dec, m.thickness_factor,
                                                             m.scaling_multiplier)
                        max_grad, min_op = _pick_thresholds(m.xyz_gradient_accum, m.denom, attrs["opacity"])
                        shared["thr"] = (max_grad, min_op)
                        shared["dec"] = train_loop.densify_decision(m.xyz_gradient_accum, m.denom, attrs["scales"], attrs["opacity"],
                                                                    max_grad, 1.0, min_op, 1e9)
                    (max_grad, min_op), dec = shared["thr"], shared["dec"]
                    if optimizer == "fused":
                        before = tr.opt.state_dict()["state"][0]
                        steps_before = list(tr.opt.steps)
                    clone, prune, n0, n1 = tr.densify_and_prune(max_grad, 1.0, min_op, 1e9, decision=dec)
                    assert n1 == n0 + int(clone.sum()) - int(prune.sum()) != n0
                    if optimizer == "fused":
                        after = tr.opt.state_dict()["state"][0]
                        for k in ("exp_avg", "exp_avg_sq"):
                            assert before[k].abs().max() > 0
                            want = torch.cat([before[k], torch.zeros_like(before[k][clone])])[~prune]
                            assert _bits_equal(after[k], want), k
                        assert tr.opt.steps == steps_before == [CHANGE_AT] * 4
                        assert tr.opt.param_groups[0]["params"][0] is tr.m.xyz and tr.opt.exp_avg.numel() == sum(p.numel() for p in tr.params)
                    tr.oneup_sh_degree()
                    assert tr.captured is None
                ld = tr.step(A[f], gts[f], mask)
                out.append(float(ld["loss"]))
                assert tr.opt.param_groups[0]["lr"] == schedule(it) and tr.opt.param_groups[1]["lr"] == LRS["triplane"]
                if optimizer == "fused":
                    assert tr.opt.steps == [it + 1] * 4
            rz.check_deferred_overflow(dev)
            losses[name], sizes[name] = np.array(out), int(tr.m.xyz.shape[0])
            if use_graph:
                assert tr.captured is not None and tr.captured.version == tr.m.topology_version
            rz.set_overflow_check("sync"); rz.reset_overflow_state()
            decode.set_gradient_arena(None, None)
            del tr
    finally:
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)
    assert len(set(sizes.values())) == 1
    # ---- a capture leaves the optimiser as it found it (its warm-up runs execute the body, the Adam launch included)
    assert len(Probe.log) == 2, "captured once for each set of Gaussians"
    for (p0, m0, v0, s0), (p1, m1, v1, s1) in Probe.log:
        assert s0 == s1 and _bits_equal(m0, m1) and _bits_equal(v0, v1)
        assert len(p0) == len(p1) and all(_bits_equal(a, b) for a, b in zip(p0, p1))
    # ---- the trajectories
    worst = {}
    for a, b in (("torch", "fused"), ("torch", "fused_graph"), ("fused", "fused_graph")):
        rel = np.abs(losses[a] - losses[b]) / np.abs(losses[a])
        worst[(a, b)] = (float(rel.max()), int(rel.argmax()))
    print("loss trajectories: first %.6f last %.6f; max rel " % (losses["torch"][0], losses["torch"][-1])
          + ", ".join(f"{a}-vs-{b} {r:.2e} (step {i})" for (a, b), (r, i) in worst.items()))
    assert losses["torch"][-1] < losses["torch"][0], "the loop optimises"
    for pair, (r, i) in worst.items():
        assert r <= 1e-4, (pair, i, r)


class _OneRank:
    """What ``AvatarTrainer`` asks of a ``FrameParallel``, on a group of one rank: the sum over ranks is the buffer itself."""

    def all_reduce_grads(self, flat):
        self.seen = flat.data_ptr()

    def reduce_densification_stats(self, accum, denom, radii):
        pass


def test_with_frame_parallel_the_launch_follows_the_all_reduce():
    """``fp`` given: the body stays without the optimiser, ``apply(sync=False)`` runs on the reduced arena.  On one rank that is the
    same computation as the fused step without ``fp``: eight steps, the same 1e-4 bar."""
    from sings_amd import decode, rasterizer as rz
    dev = torch.device("cuda:0")
    sc = _scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A = [t(a) for a in sc["frames"]]; gts = [t(g) for g in sc["gts"]]; mask = t(sc["mask"])
    out = {}
    try:
        for name in ("plain", "fp"):
            tr = _trainer(sc, dev, "fused", False, None, fp=_OneRank() if name == "fp" else None)
            out[name] = [float(tr.step(A[i], gts[i], mask)["loss"]) for i in range(8)]
            assert tr.opt.steps == [8] * 4
            if name == "fp":
                assert tr.fp.seen == tr.flat.data_ptr()
            decode.set_gradient_arena(None, None)
    finally:
        rz.set_overflow_check("sync"); rz.reset_overflow_state()
        decode.set_gradient_arena(None, None)
    a, b = np.array(out["plain"]), np.array(out["fp"])
    assert b[-1] < b[0]
    assert (np.abs(a - b) / np.abs(a)).max() <= 1e-4
