"""Checkpoint and resume of a whole ``AvatarTrainer`` run (``sings_amd.checkpoint``) on the scene of tests/test_gpu_density_schedule.py:
86 vertices, 64 x 64, six byte frames with two per step, the compressed 16-step golden schedule (prune at 3, 7, 11, densify at 5, 8, 11,
13, ``densify_interval`` 3 -> 4) under its certain-selection thresholds, ``sh_up_every`` 5.  The trainer carries every stateful part at
once: the fused optimiser, learned poses, the mesh with ``MeshTerms``, a ``DecoderSchedule`` that thaws the geometry decoder at 2 and the
appearance decoder at 6, the frame feed, and the device patch sampler with an LPIPS term (patches of 16 fit the 64 x 64 frame).

The tri-plane backward adds with float atomics, so no two runs are bit-identical (tests/test_gpu_train_loop_fused.py).  What is exact
and what is not:

    the STATE         save at iteration t, load into a fresh trainer, compare the live objects before either steps again: bits
    the next INPUTS   frame indices, background colour and patch corners of every later step: integers / bits
    the INTEGERS      density_log, N, SH degree and decoder flags of every later step, and the golden event list
    the LOSSES        resumed against uninterrupted, every later step: 1e-4 relative -- the project's bar for two executions of one
                      computation (tests/test_gpu_train_loop.py, test_gpu_train_loop_fused.py); the uninterrupted run's own spread over two
                      executions is printed beside the worst value

Cuts: t = 4 (behind a prune; the appearance decoder still frozen: its group at step 0), t = 9 (behind a densification: [N,1] multiplier,
grown ``level_id``, SH degree 1), t = 12 (behind the joint event: the interval is 4 -- a resume that loses it densifies at 14, not 13).
``MeshTerms.col`` is compared over its ``nnz`` defined entries (the buffer is sized for all edges; the same-label ones fill it).
The LPIPS term's random background is passed per iteration, as tests/test_gpu_trainer_parts.py does: torch's generator is not part of a run."""
import copy
import math
import warnings

import pytest
import torch

import lpips_case as lc
from sings_amd import checkpoint as ck
from sings_amd import export
from sings_amd import frame_feed as ff
from sings_amd import patch_sampler as ps
from test_gpu_density_schedule import F, H, K, SEED, STEPS, W, _l2norm, _reset, _schedule, _t, golden, scene  # noqa: F401 (fixtures)
from test_gpu_mesh_terms_train import _mesh_terms
from test_gpu_patch_sampler import NPATCH, PATCH
from test_gpu_pose_train import POSE_LRS
from test_gpu_train_loop import _modules

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CUTS = (4, 9, 12)
THAW = (2, 100, 6, 100)                                          # DecoderSchedule: geometry learns from 2, appearance from 6
REL = 1e-4


@pytest.fixture(scope="module")
def parts():
    """What every trainer of this file shares and never changes: the LPIPS network and the per-iteration LPIPS backgrounds."""
    from sings_amd.lpips import LPIPS
    wt = lc.make_weights(0)
    net = LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"], device=DEV)
    bgs = [torch.rand(K, 3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(100 + i)) for i in range(STEPS + 1)]
    return net, bgs


def _trainer(scene, golden, parts, use_graph=False, optimizer="fused"):
    from sings_amd.pose import PoseTable
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.topology import MeshState
    from sings_amd.train_loop import AvatarTrainer, DecoderSchedule
    from sings_amd.train_step import AvatarStep
    sc, st = scene
    tri, geo, app = _modules(DEV)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-4.95)
    mod = AvatarStep(_t(sc["xyz"]), _t(sc["w"]), tri, geo, app, l2_norm=_l2norm(), lpips=parts[0], lpips_w=1.0,
                     lpips_patch_size=PATCH).to(DEV)
    feed = ff.FrameFeed(st, seed=SEED, frames_per_step=K)
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
                       max_sh_degree=3, optimizer=optimizer, poses=poses, mesh=MeshState.from_faces(_t(sc["faces"]), _t(sc["labels"])),
                       mesh_terms=_mesh_terms(), decoder_schedule=DecoderSchedule(*THAW), frames=feed,
                       lpips_sampler=ps.DevicePatchSampler(NPATCH, PATCH, 0.9, seed=SEED + 1, device=DEV))
    tr.set_density_schedule(_schedule(golden, sh_up_every=5))
    return tr


def _bits(t):
    t = t.detach().contiguous()
    return t.cpu().reshape(-1).view(torch.uint8).clone(), t.dtype, tuple(t.shape)


def _moments(tr):
    """{group name: (step, [exp_avg bits], [exp_avg_sq bits])} of either optimiser, each parameter in its own shape."""
    out = {}
    if tr.fused:
        ms, vs = tr.opt._moment_views(tr.opt.exp_avg), tr.opt._moment_views(tr.opt.exp_avg_sq)
        k = 0
        for gi, g in enumerate(tr.opt.param_groups):
            n = len(g["params"])
            out[g["name"]] = (tr.opt.steps[gi], [_bits(x) for x in ms[k:k + n]], [_bits(x) for x in vs[k:k + n]])
            k += n
        return out
    for g in tr.opt.param_groups:
        st = [tr.opt.state.get(p) for p in g["params"]]
        steps = {int(float(s["step"])) for s in st if s} or {0}
        assert len(steps) == 1
        zero = lambda p: _bits(torch.zeros_like(p))
        out[g["name"]] = (steps.pop(), [_bits(s["exp_avg"]) if s else zero(p) for s, p in zip(st, g["params"])],
                          [_bits(s["exp_avg_sq"]) if s else zero(p) for s, p in zip(st, g["params"])])
    return out


def _live(tr, optimizer=True):
    """Everything item 1 of the module docstring names, read off the LIVE trainer (not off its state_dict): tensors as bits."""
    m, mesh, mt = tr.m, tr.mesh, tr.mesh_terms
    live = {"params": {g["name"]: [_bits(p) for p in g["params"]] for g in tr.opt.param_groups},
            "stats": [_bits(t) for t in m.stats_tensors()], "lbs_weights": _bits(m.lbs_weights),
            "opacity_offset": _bits(m.appearance_dec.opacity_offset) if torch.is_tensor(m.appearance_dec.opacity_offset) else None,
            "scaling_multiplier": _bits(m.scaling_multiplier) if torch.is_tensor(m.scaling_multiplier) else m.scaling_multiplier,
            "mesh": {k: _bits(getattr(mesh, k)) for k in ("faces", "edges", "vertex_label", "level_id")},
            "gs_level_mark": list(mesh.gs_level_mark),
            "poses": {k: _bits(getattr(tr.poses, k)) for k in ("global_orient", "body_pose", "transl")},
            "mesh_terms": {"verts": _bits(mt.verts), "normals": _bits(mt.normals), "row_ptr": _bits(mt.row_ptr), "col": _bits(mt.col[:mt.nnz]),
                           "mesh_edge": _bits(mt.mesh_edge), "nnz": mt.nnz, "V": mt.V, "E": mt.E},
            "gate": (_bits(tr._gate), tr._gate_value),
            "feed": (tr.frames.counter, tr.frames.seed), "sampler": (tr.lpips_sampler.counter, tr.lpips_sampler.seed),
            "sh_degree": tr.sh_degree, "iteration": tr.iteration, "flags": (m.opt_geo, m.opt_app), "l2_keys": tuple(m.l2_keys),
            "schedule": tr.density_schedule.state_dict(), "density_log": [dict(e) for e in tr.density_log]}
    if optimizer:
        live["moments"] = _moments(tr)
    return live


def _differs(a, b, path="live"):
    """The path of the first difference between two ``_live`` nests (tensors were taken as (bytes, dtype, shape)), or None."""
    if torch.is_tensor(a):
        return None if torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b) else path
    if isinstance(a, dict):
        if not isinstance(b, dict) or list(a) != list(b):
            return path
        return next((d for d in (_differs(a[k], b[k], f"{path}.{k}") for k in a) if d), None)
    if isinstance(a, (list, tuple)):
        if type(a) is not type(b) or len(a) != len(b):
            return path
        return next((d for d in (_differs(x, y, f"{path}[{i}]") for i, (x, y) in enumerate(zip(a, b))) if d), None)
    return None if type(a) is type(b) and a == b else path


def _step(tr, bgs):
    """One step -> what items 2-4 compare: the inputs the step drew, the integers behind it, the loss."""
    t = tr.iteration
    ld = tr.step_next(lpips_bg=bgs[t])
    return dict(t=t, loss=float(ld["loss"]), idx=tr.frames.last_indices.tolist(), bg=tr.frames.bg.view(torch.int32).cpu().tolist(),
                corners=tr.lpips_sampler.last_origins.cpu().tolist(), N=int(tr.m.xyz.shape[0]), sh=tr.sh_degree,
                flags=(tr.m.opt_geo, tr.m.opt_app))


def _uninterrupted(scene, golden, parts, use_graph, cuts=CUTS):
    try:
        tr = _trainer(scene, golden, parts, use_graph)
        out = dict(steps=[], ckpt={}, live={})
        for t in range(STEPS):
            if t in cuts:
                out["ckpt"][t] = tr.state_dict(spatial_lr_scale=2.5)
                out["live"][t] = _live(tr)
            out["steps"].append(_step(tr, parts[1]))
        out["log"] = [dict(e) for e in tr.density_log]
        return out
    finally:
        _reset()


@pytest.fixture(scope="module")
def eager(scene, golden, parts):
    return _uninterrupted(scene, golden, parts, False, cuts=(3,) + CUTS)          # (3: in front of the first change of the set)


@pytest.fixture(scope="module")
def eager_again(scene, golden, parts):
    return _uninterrupted(scene, golden, parts, False, cuts=())


@pytest.fixture(scope="module")
def replayed(scene, golden, parts):
    return _uninterrupted(scene, golden, parts, True)


def _key(log):
    return [(e["t"], e["mode"], e["n_old"], e["n_new"], e["skipped"]) for e in log]


def test_the_uninterrupted_run_is_the_golden_one(eager, replayed, golden):
    """The scene still takes the golden schedule's decisions with every part attached, and the cuts lie where the docstring says."""
    for run in (eager, replayed):
        assert [[e["t"], e["mode"]] for e in run["log"]] == golden["events"]
        assert [s["sh"] for s in run["steps"]] == [0] * 5 + [1] * 5 + [2] * 5 + [3]
        assert [s["flags"] for s in run["steps"]] == [(False, False)] * 2 + [(True, False)] * 4 + [(True, True)] * 10
    assert _key(eager["log"]) == _key(replayed["log"])
    sd4, sd9, sd12 = (eager["ckpt"][t] for t in CUTS)
    assert sd4["xyz"].shape[0] < 86 and sd4["scaling_multiplier"] is None
    n9 = sd9["xyz"].shape[0]
    assert tuple(sd9["scaling_multiplier"].shape) == (n9, 1) and tuple(sd9["level_id"].shape) == (n9,) and sd9["active_sh_degree"] == 1
    assert sd12["sings_amd"]["density_schedule"]["densify_interval"] == 4 and sd9["sings_amd"]["density_schedule"]["densify_interval"] == 3
    # the frozen appearance group has taken no step at 4, the tri-plane two (it learns with the geometry decoder, from 2)
    steps = {g["name"]: {int(float(sd4["optimizer"]["state"][i]["step"])) for i in g["params"]} for g in sd4["optimizer"]["param_groups"]}
    assert steps["appearance"] == {0} and steps["geometry"] == {2} and steps["triplane"] == {2} and steps["xyz"] == {4}


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("cut", CUTS)
def test_resume(cut, use_graph, scene, golden, parts, eager, eager_again, replayed, tmp_path):
    whole = replayed if use_graph else eager
    sd = whole["ckpt"][cut]
    # the file: the reference's keys plus one, allowed leaves only, read back with weights_only
    assert list(sd) == export.checkpoint_keys(1) + ["sings_amd"] and sd["spatial_lr_scale"] == 2.5 and sd["betas"] is None
    ck.check_leaves(sd)
    try:
        tr = _trainer(scene, golden, parts, use_graph)
        path = tmp_path / f"human_{cut:06d}.pth"
        ck.atomic_save(sd, path)
        assert ck.leaves_equal(torch.load(path, weights_only=True), sd) is None
        report = tr.load_checkpoint(path)
        assert report == {"skipped": [], "absent": [], "missing_groups": [], "dropped_groups": []}
        # 1. the state is exact: the live objects of the resumed trainer against those of the saving one, before either steps
        assert _differs(whole["live"][cut], _live(tr)) is None, _differs(whole["live"][cut], _live(tr))
        assert tr.captured is None and tr.iteration == cut
        again = tr.state_dict(spatial_lr_scale=2.5)
        assert ck.leaves_equal(again, sd) is None, ck.leaves_equal(again, sd)
        # 2.-4. every step behind the cut
        got = [_step(tr, parts[1]) for _ in range(cut, STEPS)]
        want = whole["steps"][cut:]
        for g, w in zip(got, want):
            assert g["t"] == w["t"]
            assert (g["idx"], g["bg"], g["corners"]) == (w["idx"], w["bg"], w["corners"]), g["t"]          # 2. the inputs
            assert (g["N"], g["sh"], g["flags"]) == (w["N"], w["sh"], w["flags"]), g["t"]                  # 3. the integers
        assert _key(tr.density_log) == _key(whole["log"])
        assert [[e["t"], e["mode"]] for e in tr.density_log] == golden["events"] and tr.density_schedule.densify_interval == 4
        assert tr.frames.counter == STEPS * K and tr.lpips_sampler.counter == STEPS and tr.iteration == STEPS
        rel = [abs(g["loss"] - w["loss"]) / abs(w["loss"]) for g, w in zip(got, want)]                     # 4. the losses
        own = [abs(a["loss"] - b["loss"]) / abs(a["loss"]) for a, b in zip(eager["steps"][cut:], eager_again["steps"][cut:])]
        print(f"cut {cut} graph={use_graph}: worst resumed vs uninterrupted {max(rel):.2e} (bound {REL:.0e}); two uninterrupted eager "
              f"runs over the same steps {max(own):.2e}")
        assert all(math.isfinite(g["loss"]) for g in got) and max(rel) <= REL, (rel.index(max(rel)) + cut, max(rel))
    finally:
        _reset()


def test_torch_and_fused_read_each_others_files(scene, golden, parts, eager):
    """The fused run's file at 9 into a ``"torch"`` trainer, that trainer's own file back into a fused one: moments and step counts exact
    after each load, the following steps' losses inside the bar."""
    cut, n_steps = 9, 2
    sd, want_live = eager["ckpt"][cut], eager["live"][cut]
    want = eager["steps"][cut:cut + n_steps]
    try:
        tt = _trainer(scene, golden, parts, optimizer="torch")
        tt.load_state_dict(copy.deepcopy(sd))
        live = _live(tt)
        assert _differs(want_live, live) is None, _differs(want_live, live)      # (moments per parameter, steps per group: either optimiser)
        back = tt.state_dict(spatial_lr_scale=2.5)
        assert back["sings_amd"]["optimizer_kind"] == "torch" and sd["sings_amd"]["optimizer_kind"] == "fused"
        assert ck.leaves_equal(back["optimizer"]["state"], sd["optimizer"]["state"]) is None
        got_t = [_step(tt, parts[1]) for _ in range(n_steps)]
        del tt
        _reset()
        tf = _trainer(scene, golden, parts, optimizer="fused")
        tf.load_state_dict(back)
        live = _live(tf)
        assert _differs(want_live, live) is None, _differs(want_live, live)
        got_f = [_step(tf, parts[1]) for _ in range(n_steps)]
        for name, got in (("torch", got_t), ("fused", got_f)):
            rel = [abs(g["loss"] - w["loss"]) / abs(w["loss"]) for g, w in zip(got, want)]
            print(f"fused file -> {name}: " + " ".join(f"{r:.1e}" for r in rel))
            assert max(rel) <= REL and [(g["idx"], g["corners"], g["N"]) for g in got] == [(w["idx"], w["corners"], w["N"]) for w in want]
    finally:
        _reset()


def _reference_file(sd):
    """``sd`` as the reference's ``save_ckpt`` would have written it with two levels: ``export.checkpoint_keys(2)``, unused level-1
    decoders, the reference's optimiser groups (sings_hybrid.py:750-771) with the level-1 groups between the decoders and the poses."""
    ref = {k: copy.deepcopy(sd[k]) for k in export.checkpoint_keys(1)}
    ref["geometry_dec_1"], ref["appearance_dec_1"] = copy.deepcopy(sd["geometry_dec_0"]), copy.deepcopy(sd["appearance_dec_0"])
    by = {g["name"]: g for g in sd["optimizer"]["param_groups"]}
    order = [("xyz", "xyz"), ("triplane", "v_embed"), ("geometry", "geometry_dec_0"), ("appearance", "appearance_dec_0"),
             ("geometry", "geometry_dec_1"), ("appearance", "appearance_dec_1"), ("global_orient", "global_orient"), ("body_pose", "body_pose")]
    state, groups, k = {}, [], 0
    for ours, theirs in order:
        g = by[ours]
        idx = list(range(k, k + len(g["params"])))
        for i, j in zip(idx, g["params"]):
            state[i] = copy.deepcopy(sd["optimizer"]["state"][j])
        groups.append(dict(g, name=theirs, params=idx))
        k += len(idx)
    ref["optimizer"] = {"state": state, "param_groups": groups}
    assert set(ref) == set(export.checkpoint_keys(2))
    return ref


def _render(tr, A, transl):
    from sings_amd.skinned import rasterize_skinned_gaussians
    with torch.no_grad():
        a = tr.m.decode()
        color, _ = rasterize_skinned_gaussians(a["xyz_canon"], a["rot6d_canon"], a["scales"], a["opacity"], a["shs"], tr.m.lbs_weights, A,
                                               tr.rs, smpl_scale=tr.smpl_scale, transl=transl)
    return color.clone()


def _source_image(scene, golden, parts, sd):
    """The image of the trainer ``sd`` was saved from (the resume test proves a loaded trainer IS that trainer), at frame 0's pose."""
    try:
        src = _trainer(scene, golden, parts)
        src.load_state_dict(sd)
        A, transl = (x.detach().clone() for x in src.poses(0))
        src.frames.bg.fill_(0.25)
        return A, transl, _render(src, A, transl)
    finally:
        _reset()


def test_a_reference_layout_file_loads_the_model(scene, golden, parts, eager):
    """Two files in the reference's layout.  From iteration 3 -- no change of the set yet, so the file holds the whole model: the loaded
    trainer renders the source's image.  From iteration 9 -- [N,1] multiplier, grown level ids, and an opacity offset the reference's
    layout has no key for (its own reload loses it: INTEGRATION.md 20): every entry the file has arrives bit for bit, the offset is the
    initial 0."""
    model = ("stats", "lbs_weights", "scaling_multiplier", "gs_level_mark", "sh_degree", "mesh")
    try:
        for cut in (3, 9):
            sd, want_live = eager["ckpt"][cut], eager["live"][cut]
            ref = _reference_file(sd)
            faces = sd["sings_amd"]["mesh"]["faces"]
            if cut == 3:
                assert sd["sings_amd"]["opacity_offset"] is None
                A, transl, want_img = _source_image(scene, golden, parts, sd)
            tr = _trainer(scene, golden, parts)
            before = tr.state_dict()
            with pytest.raises(ValueError, match="faces"):           # a mesh= trainer, and the file has no faces to offer
                ck.load_reference(tr, ref)
            with pytest.raises(ValueError, match="load_reference"):  # ... and the whole-run entrance says where such a file goes
                tr.load_state_dict(ref)
            assert ck.leaves_equal(tr.state_dict(), before) is None
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                report = ck.load_reference(tr, ref, faces=faces)
            assert not [w for w in seen if "pretrained optimiser" in str(w.message)]
            assert report["optimizer"] == "loaded" and report["ignored"] == ["appearance_dec_1", "geometry_dec_1"]
            assert report["dropped_groups"] == ["geometry_dec_1", "appearance_dec_1"]
            live = _live(tr)
            for name in ("xyz", "triplane", "geometry", "appearance"):   # (the pose tables are not the reference file's to give)
                assert _differs(want_live["params"][name], live["params"][name]) is None, (cut, name)
            for k in model:                                          # (the mesh: what the file's labels and the given faces make)
                assert _differs(want_live[k], live[k]) is None, (cut, k)
            for name in ("xyz", "triplane", "geometry", "appearance", "global_orient", "body_pose"):
                assert _differs(want_live["moments"][name], live["moments"][name]) is None, (cut, name)
            assert tr.iteration == 0 and tr.density_log == [] and tr.mesh_terms.V == int(tr.m.xyz.shape[0])
            assert live["opacity_offset"] is None and tr.m.appearance_dec.opacity_offset == 0
            if cut == 3:
                tr.frames.bg.fill_(0.25)
                img = _render(tr, A, transl)
                worst = float((img - want_img).abs().max())
                print(f"reference-layout file: max |image - source's| = {worst:.2e} of {float(want_img.abs().max()):.2f}")
                assert worst <= REL * float(want_img.abs().max()) and float(want_img.std()) > 0
                del tr
                _reset()
                continue
            assert want_live["opacity_offset"] is not None and tuple(tr.m.scaling_multiplier.shape) == (int(tr.m.xyz.shape[0]), 1)
            # groups that do not fit: zero moments, with the warning -- the model still loads
            bad = copy.deepcopy(ref)
            bad["optimizer"]["param_groups"][1]["name"] = "embedding"
            with pytest.warns(UserWarning, match="without a pretrained optimiser"):
                report = ck.load_reference(tr, bad, faces=faces)
            assert report["optimizer"] == "zero"
            mom = _moments(tr)
            assert all(step == 0 and all(int(b[0].max()) == 0 for b in m1 + m2) for step, m1, m2 in mom.values())
            assert _differs(want_live["params"]["xyz"], _live(tr)["params"]["xyz"]) is None
            ld = tr.step_next(lpips_bg=parts[1][0])
            assert math.isfinite(float(ld["loss"])) and tr.iteration == 1
    finally:
        _reset()


def test_a_refused_load_leaves_a_working_trainer(scene, golden, parts, eager):
    """Four refusals in a row on one trainer -- wrong N relation, a missing component, another frame store, a future version -- then a
    step: its loss against that step of an untouched twin."""
    sd = eager["ckpt"][9]
    cases = {}
    cases["lbs_weights"] = copy.deepcopy(sd)
    cases["lbs_weights"]["lbs_weights"] = torch.cat([sd["lbs_weights"], sd["lbs_weights"][:1]])
    cases["components"] = copy.deepcopy(sd)
    cases["components"]["sings_amd"]["components"]["lpips_sampler"] = False
    cases["store"] = copy.deepcopy(sd)
    cases["store"]["sings_amd"]["store"]["F"] = F + 1
    cases["version"] = copy.deepcopy(sd)
    cases["version"]["sings_amd"]["version"] = ck.FORMAT_VERSION + 1
    try:
        tr = _trainer(scene, golden, parts)
        before, version = tr.state_dict(), tr.m.topology_version
        xyz = tr.m.xyz
        for match, bad in cases.items():
            keep = copy.deepcopy(bad)
            with pytest.raises(ValueError, match=match):
                tr.load_state_dict(bad)
            assert ck.leaves_equal(bad, keep) is None
        assert tr.m.xyz is xyz and tr.m.topology_version == version and ck.leaves_equal(tr.state_dict(), before) is None
        # strict=False takes the file without the sampler's entry, and says so
        report = tr.load_state_dict(cases["components"], strict=False)
        assert report["absent"] == ["lpips_sampler"] and report["skipped"] == [] and tr.iteration == 9 and tr.lpips_sampler.counter == 0
        del tr
        _reset()
        tr = _trainer(scene, golden, parts)
        for bad in cases.values():
            with pytest.raises(ValueError):
                tr.load_state_dict(bad)
        got = _step(tr, parts[1])
        del tr
        _reset()
        twin = _step(_trainer(scene, golden, parts), parts[1])
        rel = abs(got["loss"] - twin["loss"]) / abs(twin["loss"])
        print(f"a step behind four refusals against an untouched twin: {rel:.2e}")
        assert rel <= REL and (got["idx"], got["bg"], got["corners"], got["N"]) == (twin["idx"], twin["bg"], twin["corners"], twin["N"])
    finally:
        _reset()


def test_run_until_saves_on_the_references_rule(scene, golden, parts, tmp_path):
    try:
        tr = _trainer(scene, golden, parts)
        losses = tr.run_until(5, save_every=2, save_dir=tmp_path / "ckpt")
        assert len(losses) == 6 and tr.iteration == 6             # (iterations 0 .. num_steps, as the reference's range)
        files = sorted(p.name for p in (tmp_path / "ckpt").iterdir())
        assert files == ["human_000000.pth", "human_000002.pth", "human_000004.pth", "human_000005.pth"]
        sd = torch.load(tmp_path / "ckpt" / "human_000004.pth", weights_only=True)
        assert sd["sings_amd"]["iteration"] == 5 and sd["sings_amd"]["frames"]["counter"] == 5 * K
        with pytest.raises(ValueError, match="go together"):
            tr.run_until(7, save_every=2)
    finally:
        _reset()
