"""``AvatarTrainer.prune_and_simplify`` (the pruning half of the reference's ``hybrid`` strategy, sings_hybrid.py:1153-1257) on the trainer
of tests/test_gpu_subdivide_train.py (the 86 vertices of ``bumpy_sphere(12, 8)`` as anchors): a few steps, the simplification with
thresholds picked from the run's own statistics, a few more steps -- eager and graph-replayed, with the torch and the fused optimiser;
a call driven with the recorded decision of the reference composite (tests/golden/simplify_golden.npz, ``comp_prune``); every skip
rule; and both orders of subdivision and simplification."""
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_subdivide_train import DEV, _bits_equal, _decode, _edges_by_torch, _mesh_scene, _moments, _trainer

pytestmark = pytest.mark.gpu

STATS = ("xyz_gradient_accum", "denom", "max_radii2D")


@pytest.fixture(scope="module")
def topology_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topology_golden.npz"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simplify_golden.npz"))


def _inputs(sc):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return [t(a) for a in sc["frames"]], [t(g) for g in sc["gts"]], t(sc["mask"])


def _cleanup():
    from sings_amd import decode, rasterizer as rz
    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    decode.set_gradient_arena(None, None)


def _state(tr):
    m, mesh = tr.m, tr.mesh
    sm = m.scaling_multiplier
    return dict(xyz=m.xyz.detach().clone(), w=m.lbs_weights.clone(), labels=mesh.vertex_label.clone(), level=mesh.level_id.clone(),
                faces=mesh.faces.clone(), moments=_moments(tr), attrs=_decode(tr), stats=[getattr(m, k).clone() for k in STATS],
                sm=sm.clone() if torch.is_tensor(sm) and sm.dim() > 0 else sm)


def _thresholds(tr, attrs, q=0.9):
    """From the run's own numbers: transparent-and-small = below the q-quantile of both; big-and-dead = the largest scales among the
    Gaussians that were visible at all (dead_grad 1: every finite gradient is 'dead')."""
    op = attrs["opacity"].reshape(-1)
    s = (attrs["scales"] * tr.smpl_scale.reshape(1, -1))[:, 0]
    return dict(opacity_threshold=float(torch.quantile(op, q)), scale_threshold=float(torch.quantile(s, q)), dead_grad=1.0,
                large_scale=float(torch.quantile(s, 0.95)))


def _expected_mask(tr, before, th):
    op = before["attrs"]["opacity"].reshape(-1)
    s = (before["attrs"]["scales"] * tr.smpl_scale.reshape(1, -1))[:, 0]
    accum, denom = before["stats"][0].reshape(-1), before["stats"][1].reshape(-1)
    hands = torch.isin(before["labels"], torch.tensor([6, 7], dtype=torch.int32, device=DEV))
    return ((op < th["opacity_threshold"]) & (s < th["scale_threshold"]) | (s > th["large_scale"]) & (accum / denom < th["dead_grad"])) & ~hands


def _check_call(tr, before, result, stale):
    """What must hold after ANY prune_and_simplify that pruned: ``before`` = the state in front of the call."""
    m, mesh = tr.m, tr.mesh
    vert_mask, prune, n_old, n_new = result
    keep = ~prune
    pruned = int(prune.sum())
    assert n_old == before["xyz"].shape[0] and pruned > 0 and n_new == n_old - pruned == int(m.xyz.shape[0])
    assert not bool((prune & ~vert_mask).any())                       # only selected vertices go
    # the survivors' rows, bit for bit: anchors, weights, multipliers, both moments, all three statistics
    assert _bits_equal(m.xyz.detach(), before["xyz"][keep]) and _bits_equal(m.lbs_weights, before["w"][keep])
    if torch.is_tensor(before["sm"]):
        assert tuple(m.scaling_multiplier.shape) == (n_new, 1) and _bits_equal(m.scaling_multiplier, before["sm"][keep])
    for new, old in zip(_moments(tr), before["moments"]):
        assert float(old.abs().max()) > 0 and _bits_equal(new, old[keep])
    assert tr.opt.param_groups[0]["params"][0] is m.xyz
    for k, old in zip(STATS, before["stats"]):
        assert float(old.abs().max()) > 0 and _bits_equal(getattr(m, k), old[keep]), k
    # the mesh: faces on the new numbering, `edges` their unique sorted rows, labels masked, level ids truncated
    assert int(mesh.faces.min()) == 0 and int(mesh.faces.max()) == n_new - 1 and mesh.faces.dtype == torch.int32
    assert len(torch.unique(mesh.faces)) == n_new                    # no isolated vertex stays
    assert torch.equal(mesh.edges.cpu().long(), _edges_by_torch(mesh.faces))
    assert mesh.vertex_label.dtype == torch.int32 and torch.equal(mesh.vertex_label, before["labels"][keep])
    assert torch.equal(mesh.level_id, before["level"][:n_new]) and mesh.gs_level_mark[-1] == n_new and mesh.num_verts == n_new
    assert tr.last_simplification["skipped"] is None and tr.last_simplification["n_new"] == n_new
    assert 0 < tr.last_simplification["collapses"] <= pruned
    # opacity reset on the new set: no opacity below 0.5
    off = m.appearance_dec.opacity_offset
    assert torch.is_tensor(off) and off.shape[0] == n_new and float(_decode(tr)["opacity"].min()) >= 0.5 - 1e-6
    # the stale graph refuses; the trainer dropped it
    assert tr.captured is None
    if stale is not None:
        with pytest.raises(RuntimeError, match="capture the step again"):
            stale.replay()


@pytest.mark.parametrize("optimizer,use_graph", [("torch", False), ("torch", True), ("fused", False), ("fused", True)])
def test_steps_simplification_steps(topology_golden, optimizer, use_graph):
    from sings_amd import rasterizer as rz
    from sings_amd.train_loop import CapturedStep
    sc = _mesh_scene(topology_golden)
    A, gts, mask = _inputs(sc)
    try:
        tr = _trainer(sc, optimizer, use_graph)
        losses = [float(tr.step(A[i], gts[i], mask)["loss"]) for i in range(4)]
        stale = tr.captured
        assert (stale is not None) == use_graph and (stale is None or isinstance(stale, CapturedStep))
        before = _state(tr)
        th = _thresholds(tr, before["attrs"])
        result = tr.prune_and_simplify(**th)
        vert_mask = result[0]
        print(f"selected {int(vert_mask.sum())} of {result[2]}, edges {tr.last_simplification['selected_edges']}, collapses "
              f"{tr.last_simplification.get('collapses')}, N {result[2]} -> {result[3]}")
        assert torch.equal(vert_mask, _expected_mask(tr, before, th)) and 0 < int(vert_mask.sum()) < 86
        _check_call(tr, before, result, stale)
        losses += [float(tr.step(A[i], gts[i], mask)["loss"]) for i in range(4, 7)]
        assert all(math.isfinite(x) for x in losses), losses
        assert int(tr.m.xyz.grad.shape[0]) == result[3]
        # the survivors' statistics went on from where they were
        assert float(tr.m.denom.max()) == float(before["stats"][1].max()) + 3
        if use_graph:
            rz.check_deferred_overflow(DEV)
            assert tr.captured is not None and tr.captured.version == tr.m.topology_version
    finally:
        _cleanup()


def test_driven_with_the_reference_decision(topology_golden, golden):
    """``decision=``: the recorded vertex mask and selected edges of the reference composite, on the composite's positions (the anchors,
    with the offset head zeroed: ``xyz_canon`` is the anchor, bit for bit) -> its prune mask, its faces, its number of collapses."""
    sc = _mesh_scene(topology_golden)
    A, gts, mask = _inputs(sc)
    name = "comp_prune"
    try:
        tr = _trainer(sc, "fused", False)
        with torch.no_grad():
            tr.m.geometry_dec.xyz_offsets.weight.zero_(); tr.m.geometry_dec.xyz_offsets.bias.zero_()
        assert np.array_equal(sc["xyz"], golden[f"{name}_xyz_canon"]) and np.array_equal(sc["faces"], golden[f"{name}_faces"])
        assert np.array_equal(_decode(tr)["xyz_canon"].cpu().numpy().view(np.uint32), golden[f"{name}_xyz_canon"].view(np.uint32))
        dec = (torch.from_numpy(golden[f"{name}_vert_mask"].astype(bool)), torch.from_numpy(golden[f"{name}_selected_edges"]).long())
        vert_mask, prune, n_old, n_new = tr.prune_and_simplify(0.0, 0.0, decision=dec)
        want = golden[f"{name}_collapse_prune_mask"].astype(bool)
        assert np.array_equal(prune.cpu().numpy(), want) and n_new == n_old - int(want.sum()) == int(tr.m.xyz.shape[0])
        assert np.array_equal(tr.mesh.faces.cpu().numpy(), golden[f"{name}_collapse_new_faces_ordered"])
        assert tr.last_simplification["collapses"] == int(golden[f"{name}_collapse_collapses"])
        assert np.array_equal(tr.mesh.vertex_label.cpu().numpy(), golden[f"{name}_vertex_label"][~want])
        assert np.array_equal(tr.m.xyz.detach().cpu().numpy().view(np.uint32), golden[f"{name}_xyz_canon"][~want].view(np.uint32))
        assert torch.equal(tr.mesh.edges.cpu().long(), _edges_by_torch(tr.mesh.faces))
        ld = tr.step(A[0], gts[0], mask)
        assert math.isfinite(float(ld["loss"]))
    finally:
        _cleanup()


def test_every_skip_rule_leaves_everything_untouched(topology_golden):
    sc = _mesh_scene(topology_golden)
    A, gts, mask = _inputs(sc)
    try:
        tr = _trainer(sc, "fused", True)
        for i in range(4):
            tr.step(A[i], gts[i], mask)
        m, mesh = tr.m, tr.mesh
        assert tr.captured is not None
        th = _thresholds(tr, _decode(tr))
        objects = lambda: [m.xyz, m.lbs_weights, m.xyz_gradient_accum, m.denom, m.max_radii2D, mesh.faces, mesh.edges, mesh.vertex_label,
                           mesh.level_id, tr.opt.exp_avg, tr.opt.exp_avg_sq, tr.flat, m.appearance_dec.opacity_offset, tr.captured]
        held = objects()
        values = [x.detach().clone() for x in held[:-2]]
        version, mark = m.topology_version, list(mesh.gs_level_mark)
        none = dict(th, opacity_threshold=0.0, large_scale=1e9)
        calls = [("min_n_gs", dict(th, min_n_gs=86)), ("no_edges", none), ("too_many_edges", dict(th, prune_max_n_gs_once=0)),
                 ("no_edges", dict(none, decision=(torch.ones(86, dtype=torch.bool), torch.zeros((0, 2), dtype=torch.int64))))]
        for reason, kw in calls:
            vert_mask, prune, n_old, n_new = tr.prune_and_simplify(**kw)
            assert tr.last_simplification["skipped"] == reason, (reason, tr.last_simplification)
            assert n_old == n_new == 86 and tuple(prune.shape) == (86,) and prune.dtype == torch.bool and not bool(prune.any())
            assert all(a is b for a, b in zip(objects(), held))
            assert all(_bits_equal(a.detach(), b) for a, b in zip(held[:-2], values))
            assert m.topology_version == version and mesh.gs_level_mark == mark
        assert tr.last_simplification["selected_edges"] == 0
        # the captured graph is the one that goes on replaying
        ld = tr.step(A[4], gts[4], mask)
        assert tr.captured is held[-1] and math.isfinite(float(ld["loss"]))
    finally:
        _cleanup()


def test_subdivide_after_simplify_and_simplify_after_subdivide(topology_golden):
    sc = _mesh_scene(topology_golden)
    A, gts, mask = _inputs(sc)
    try:
        tr = _trainer(sc, "torch", False)
        losses = [float(tr.step(A[i], gts[i], mask)["loss"]) for i in range(3)]
        before = _state(tr)
        first = tr.prune_and_simplify(**_thresholds(tr, before["attrs"]))
        _check_call(tr, before, first, None)
        losses.append(float(tr.step(A[3], gts[3], mask)["loss"]))
        # every face with a corner outside the hands is split: the multiplier becomes per-Gaussian
        _, faces_idx, n1, n2 = tr.densify_and_subdivide(0.0, 0.0, max_n_gs=10 ** 6)
        assert n1 == first[3] and n2 > n1 and len(faces_idx) > 0 and tuple(tr.m.scaling_multiplier.shape) == (n2, 1)
        losses += [float(tr.step(A[i], gts[i], mask)["loss"]) for i in (4, 5)]
        before = _state(tr)
        second = tr.prune_and_simplify(**_thresholds(tr, before["attrs"]))
        print(f"N 86 -> {first[3]} -> {n2} -> {second[3]}")
        _check_call(tr, before, second, None)
        assert second[2] == n2
        losses.append(float(tr.step(A[6], gts[6], mask)["loss"]))
        assert all(math.isfinite(x) for x in losses), losses
    finally:
        _cleanup()


def test_needs_a_mesh(topology_golden):
    sc = _mesh_scene(topology_golden)
    try:
        tr = _trainer(sc, "torch", False)
        tr.mesh = None
        with pytest.raises(RuntimeError, match="mesh=MeshState"):
            tr.prune_and_simplify(1.0, 1.0)
    finally:
        _cleanup()
