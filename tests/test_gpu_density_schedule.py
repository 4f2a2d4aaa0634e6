"""``AvatarTrainer.set_density_schedule`` / ``run`` on the 86-vertex mesh scene of tests/test_gpu_subdivide_train.py, rendered at 64 x 64
from a ``FrameFeed`` of six 8-bit frames (two per step) with a ``PoseTable``: the compressed schedule of
tests/golden/density_schedule_golden.json over 16 steps -- prune at 3, 7, 11, densify at 5, 8, 11, 13, ``densify_interval`` 3 -> 4.

Thresholds under which selection is certain: a prune selects every vertex outside the hands (opacity < 2, scale < 1), a densification
every such vertex (gradient norm > -1, scale > 0); ``min_n_gaussians`` 20 keeps the floor out of the way, ``max_n_gaussians`` 400 caps
the growth.  The test asserts that a prune and a densification really changed the set.

Bounds: the statistics as tests/test_gpu_densify_stats.py (``denom`` / ``max_radii2D`` equal to the twin, ``accum`` within (K + 4) 2^-24
of it); the L2 term against ``L2Norm`` called directly 2e-6 relative (tests/test_gpu_reg.py's bound for a loss); eager against
graph-replayed losses 1e-4 relative per step, the number tests/test_gpu_train_loop.py uses for that comparison."""
import json
import math
import os

import numpy as np
import pytest
import torch

from mesh_case import bumpy_sphere
from sings_amd import density as dn
from sings_amd import frame_feed as ff
from test_gpu_pose_train import POSE_LRS, _pose_scene
from test_gpu_train_loop import _modules

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
W = H = 64
F, K, STEPS, SEED = 6, 2, 16, 3
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
THRESHOLDS = dict(prune_opacity_threshold=2.0, prune_scale_threshold=1.0, prune_max_n_gs_once=5000, min_n_gaussians=20,
                  densify_grad_threshold=-1.0, densify_scale_threshold=0.0, densify_render_size_threshold=20, max_n_gaussians=400)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reset():
    from sings_amd import decode, rasterizer as rz
    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    decode.set_gradient_arena(None, None)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "density_schedule_golden.json")) as f:
        return json.load(f)["compressed"]


@pytest.fixture(scope="module")
def scene():
    """The pose scene's body with the mesh scene's anchors, a 64 x 64 camera and six byte frames."""
    from sings_amd.camera import make_camera
    topo = np.load(os.path.join(HERE, "golden", "topology_golden.npz"))
    sc = _pose_scene()
    v, f, lab = bumpy_sphere(12, 8)
    sc["xyz"] = (v * np.array([0.2, 0.42, 0.15])).astype(np.float32)
    sc["w"], sc["faces"], sc["labels"] = topo["comp_lbs_weights"], f, lab
    sc["cam"] = make_camera(np.eye(4, dtype=np.float32), 260.0, 260.0, W / 2, H / 2, W, H)
    rs = np.random.RandomState(17)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = ((((xx - W / 2) / (W / 2.6)) ** 2 + ((yy - H / 2) / (H / 2.3)) ** 2) < 1)
    store = ff.FrameStore(rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8), np.repeat((mask * 255).astype(np.uint8)[None], F, 0),
                          device=DEV)
    return sc, store


def _schedule(golden, **kw):
    cfg = {k: v for k, v in golden["config"].items() if k != "steps"}
    return dn.HybridDensitySchedule(**cfg, **dict(THRESHOLDS, **kw))


def _l2norm():
    from sings_amd.regularizers import L2Norm
    return L2Norm(lambda_min_opacity=0.05, min_opacity_threshold=1.1)      # (every opacity is below 1.1: the opacity term is never 0)


def _trainer(scene, use_graph, schedule):
    from sings_amd.pose import PoseTable
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.topology import MeshState
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    sc, store = scene
    tri, geo, app = _modules(DEV)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-4.95)
    mod = AvatarStep(_t(sc["xyz"]), _t(sc["w"]), tri, geo, app, l2_norm=_l2norm()).to(DEV)
    feed = ff.FrameFeed(store, seed=SEED, frames_per_step=K)
    cam = sc["cam"]
    consts = dict(view=_t(cam["world_view_transform"]), proj=_t(cam["full_proj_transform"]), campos=_t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=feed.bg,
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    poses = PoseTable(_t(sc["start_go"][:F]), _t(sc["start_bp"][:F]), _t(sc["transl_rows"][:F]), _t(sc["joints"]), _t(sc["post"]),
                      sc["parents"])
    tr = AvatarTrainer(mod, settings, feed.bg, POSE_LRS, smpl_scale=_t(sc["smpl_scale"]), use_graph=use_graph, sh_degree=0,
                       max_sh_degree=3, optimizer="fused", poses=poses, mesh=MeshState.from_faces(_t(sc["faces"]), _t(sc["labels"])),
                       frames=feed)
    if schedule is not None:
        tr.set_density_schedule(schedule)
    return tr


def _stats(tr):
    return [getattr(tr.m, k).detach().clone() for k in STATS]


def _spy(tr, records):
    """Record, around every accumulation of an EAGER trainer: the iteration, the gate's word, the statistics before and after, and the
    step's screen-space gradient and radii."""
    inner = tr.m.add_densification_stats

    def wrapped(extras):
        before = _stats(tr)
        inner(extras)
        records.append(dict(t=tr.iteration, gate=None if tr.m.stats_gate is None else int(tr.m.stats_gate.item()), before=before,
                            after=_stats(tr), grad=extras["viewspace_points"].grad.detach().clone(), radii=extras["radii"].clone()))
    tr.m.add_densification_stats = wrapped


def _l2_wanted(tr):
    """L2Norm called directly on the current decode -> (without opacity, with opacity)."""
    with torch.no_grad():
        a = tr.m.decode()
        two = float(_l2norm()({k: a[k] for k in ("xyz_offsets", "scales")}))
        three = float(_l2norm()({k: a[k] for k in ("xyz_offsets", "scales", "opacity")}))
    return two, three


def _run(scene, golden, use_graph, spy=False):
    """Sixteen steps -> everything the tests below look at."""
    try:
        sch = _schedule(golden)
        tr = _trainer(scene, use_graph, sch)
        deciding = {t for t, _ in golden["events"]}
        out = dict(losses=[], l2=[], l2_wanted=[], sizes=[], degrees=[], replayed=[], unchanged=[], denom_after=[], records=[])
        if spy:
            _spy(tr, out["records"])
        for t in range(STEPS):
            assert tr.iteration == t
            out["l2_wanted"].append(_l2_wanted(tr))
            before = _stats(tr)
            out["replayed"].append(use_graph and tr.captured is not None and tr._sizing == 0)
            ld = tr.step_next() if t % 2 else tr.run(1)[0]       # (both entrances)
            out["losses"].append(float(ld["loss"])); out["l2"].append(float(ld["l2"]))
            out["sizes"].append(int(tr.m.xyz.shape[0])); out["degrees"].append(tr.sh_degree)
            after = _stats(tr)
            if t not in deciding:
                out["unchanged"].append(all(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
                                            for a, b in zip(before, after)))
            out["denom_after"].append(float(tr.m.denom.sum()))
        out.update(log=list(tr.density_log), interval=sch.densify_interval, l2_keys=tuple(tr.m.l2_keys), counter=tr.frames.counter)
        return out
    finally:
        _reset()


@pytest.fixture(scope="module")
def eager(scene, golden):
    return _run(scene, golden, False, spy=True)


@pytest.fixture(scope="module")
def replayed(scene, golden):
    return _run(scene, golden, True)


@pytest.mark.parametrize("which", ["eager", "replayed"])
def test_the_log_is_the_references_event_list(which, golden, request):
    run = request.getfixturevalue(which)
    log = run["log"]
    print([(e["t"], e["mode"], e["n_old"], e["n_new"], e["skipped"]) for e in log])
    assert [[e["t"], e["mode"]] for e in log] == golden["events"]
    assert run["interval"] == golden["densify_interval"] == 4
    assert all(set(e) == {"t", "mode", "n_old", "n_new", "skipped"} for e in log)
    # not vacuous: a prune and a densification really changed the set
    assert any(e["mode"] == "prune" and e["n_new"] < e["n_old"] and e["skipped"] is None for e in log)
    assert any(e["mode"] == "densify" and e["n_new"] > e["n_old"] and e["skipped"] is None for e in log)
    # the sizes the log names are the sizes the module had
    sizes = [86] + run["sizes"]
    for e in log:
        assert e["n_new"] == sizes[e["t"] + 1] or any(o["t"] == e["t"] and o is not e for o in log)
    assert run["sizes"][-1] == log[-1]["n_new"] and run["counter"] == STEPS * K
    assert run["degrees"] == [0] * STEPS                         # (sh_up_every = 1000)


@pytest.mark.parametrize("which", ["eager", "replayed"])
def test_statistics_move_only_on_deciding_steps(which, golden, request):
    run = request.getfixturevalue(which)
    assert len(run["unchanged"]) == STEPS - len({t for t, _ in golden["events"]}) and all(run["unchanged"])
    assert run["denom_after"][:3] == [0.0, 0.0, 0.0]             # nothing before the first decision
    assert run["denom_after"][3] > 0                             # the prune at 3 keeps the survivors' statistics of step 3
    assert run["denom_after"][13] == 0.0                         # a densification starts them at zero
    if which == "replayed":                                      # step 3 was a REPLAY of the graph captured at step 2, gate closed
        assert run["replayed"][3] and not run["replayed"][2]


def test_a_deciding_step_accumulates_that_steps_frames_alone(eager, golden):
    deciding = {t for t, _ in golden["events"]}
    records = eager["records"]
    assert [r["t"] for r in records] == list(range(STEPS))
    worst = 0.0
    for r in records:
        assert r["gate"] == int(r["t"] in deciding), r["t"]
        before, after = ([x.cpu().numpy() for x in r[k]] for k in ("before", "after"))
        if r["t"] not in deciding:
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(before, after)), r["t"]
            continue
        assert tuple(r["grad"].shape) == (K, before[2].shape[0], 3) and int((r["radii"] > 0).sum()) > 0
        want = dn.densify_stats_host(r["grad"].cpu().numpy(), r["radii"].cpu().numpy(), *before)
        assert np.array_equal(after[1].astype(np.float64), want[1]) and np.array_equal(after[2].astype(np.float64), want[2]), r["t"]
        seen = want[1].reshape(-1) > 0
        ratio = np.abs(after[0].astype(np.float64) - want[0]).reshape(-1)[seen] / ((K + 4) * 2.0 ** -24 * want[0].reshape(-1)[seen])
        worst = max(worst, float(np.nan_to_num(ratio, nan=0.0).max()))
        assert (np.abs(after[0].astype(np.float64) - want[0]) <= (K + 4) * 2.0 ** -24 * want[0]).all(), (r["t"], worst)
        assert float(after[1].sum()) > float(before[1].sum())
    print(f"worst |accum - twin| / bound over the deciding steps: {worst:.3f}")
    first = next(r for r in records if r["t"] == 3)
    assert all(float(x.abs().sum()) == 0.0 for x in first["before"])


@pytest.mark.parametrize("which", ["eager", "replayed"])
def test_the_l2_term_gains_opacity_at_step_14(which, request):
    """``l2_wanted``: ``L2Norm`` called directly on the decode in front of each step, without and with ``opacity``.  The opacity reset
    behind every change of the set puts the opacities it raises at exactly 0.5, where the term is 0: the two values may coincide on
    the step behind a reset (step 14 follows the densification at 13), so the test also asks that they differ on a step of each side."""
    run = request.getfixturevalue(which)
    differ = []
    for t, (got, (two, three)) in enumerate(zip(run["l2"], run["l2_wanted"])):
        want = three if t >= 14 else two
        assert abs(got - want) <= 2e-6 * abs(want), (t, got, two, three)
        differ.append(three > two * (1 + 1e-3))
    print("steps on which the opacity term is not 0:", [t for t, d in enumerate(differ) if d])
    assert any(differ[:14]) and any(differ[14:]), differ
    assert run["l2_keys"] == ("xyz_offsets", "scales", "opacity")


def test_eager_and_replayed_agree(eager, replayed):
    key = lambda log: [(e["t"], e["mode"], e["n_old"], e["n_new"], e["skipped"]) for e in log]
    assert key(eager["log"]) == key(replayed["log"]) and eager["sizes"] == replayed["sizes"]
    e, g = np.array(eager["losses"]), np.array(replayed["losses"])
    rel = np.abs(e - g) / np.abs(e)
    print("eager vs graph, per step: " + " ".join(f"{r:.1e}" for r in rel))
    assert np.isfinite(e).all() and rel.max() <= 1e-4, (int(rel.argmax()), float(rel.max()))


def test_the_sh_degree_rises_with_sh_up_every(scene, golden):
    try:
        tr = _trainer(scene, False, _schedule(golden, sh_up_every=5))
        degrees = []
        for _ in range(STEPS):
            tr.step_next()
            degrees.append(tr.sh_degree)
        assert degrees == [0] * 5 + [1] * 5 + [2] * 5 + [3]
        assert [[e["t"], e["mode"]] for e in tr.density_log] == golden["events"]
    finally:
        _reset()


def test_detaching_restores_the_accumulation_per_step(scene, golden):
    from sings_amd.train_loop import AvatarTrainer
    try:
        tr = _trainer(scene, False, _schedule(golden))
        assert tr.m.stats_gate is not None and tr.m.stats_gate.dtype == torch.int32 and tuple(tr.m.stats_gate.shape) == (1,)
        tr.run(2)
        assert float(tr.m.denom.sum()) == 0.0 and tr.m.l2_keys == ("xyz_offsets", "scales")
        tr.set_density_schedule(None)
        assert tr.m.stats_gate is None and tr.m.l2_keys == ("xyz_offsets", "scales", "opacity") and tr.density_schedule is None
        seen = []
        for _ in range(3):
            tr.step_next()
            seen.append(float(tr.m.denom.sum()))
        assert 0 < seen[0] < seen[1] < seen[2] and tr.density_log == [] and int(tr.m.xyz.shape[0]) == 86
        bare = _trainer(scene, False, None)
        bare.mesh = None
        with pytest.raises(ValueError, match="set_density_schedule needs mesh=MeshState"):
            bare.set_density_schedule(_schedule(golden))
        with pytest.raises(RuntimeError, match="run needs frames=FrameFeed"):
            tr.frames = None
            AvatarTrainer.run(tr, 1)
    finally:
        _reset()


@pytest.mark.parametrize("keys", [("xyz_offsets", "scales"), ("xyz_offsets", "scales", "opacity")])
def test_the_staged_backward_takes_either_key_list(scene, keys):
    """``AvatarStep`` with the k-NN regulariser, joined and deferred (the backward staged by hand): the same ``l2`` value as ``L2Norm``
    called directly on those keys, and the same parameter gradients either way (tests/test_gpu_mesh_terms_train.py's bound for that:
    1e-5 |ref| + 5e-6 max |ref|)."""
    from sings_amd.regularizers import GaussiansEdgeLoss
    try:
        tr = _trainer(scene, False, None)
        step = tr.m
        step.gaussian_connect, step.gaussian_connect_w = GaussiansEdgeLoss(), 0.5
        step.l2_keys = keys
        tr.frames.draw()
        A, transl = tr.poses(tr.frames.idx)
        _reset()                                                 # (the module alone, plain .grad: no gradient arena)
        with torch.no_grad():
            a = step.decode()
            want = float(_l2norm()({k: a[k] for k in keys}))
        params = [p for p in step.parameters() if p.requires_grad]
        grads = {}
        for defer in (False, True):
            step.defer_regulariser_join = defer
            for p in params:
                p.grad = None
            loss, ld, ex = step(A.detach(), tr.rs, tr.frames.gt, tr.frames.mask, tr.bg, smpl_scale=tr.smpl_scale, transl=transl.detach())
            if loss is None:
                assert defer
                step.backward(ld, ex)
            else:
                loss.backward()
            torch.cuda.synchronize()
            got = float(ld["l2"].detach())
            assert abs(got - want) <= 2e-6 * abs(want), (defer, got, want)
            grads[defer] = [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in params]
        for x, y in zip(grads[True], grads[False]):
            x, y = x.double().cpu().numpy(), y.double().cpu().numpy()
            assert (np.abs(x - y) <= 1e-5 * np.abs(y) + 5e-6 * (np.abs(y).max() + 1e-30)).all()
    finally:
        _reset()
