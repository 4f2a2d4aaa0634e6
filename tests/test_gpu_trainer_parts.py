"""``AvatarTrainer`` with every stateful part attached at once -- the fused optimiser, learned poses, a ``FrameFeed`` of two frames per
step, a ``DevicePatchSampler`` with the module's LPIPS term and a density schedule on the anchors' mesh -- on the tiny avatar of
tests/test_gpu_pose_train.py (its H, W and eight frames) with the 86 mesh anchors of tests/test_gpu_subdivide_train.py: six eager
``step_next()`` steps against six with ``use_graph=True`` (two sizing steps, the capture with its two warm-up runs at the third,
three replays).

Each part's own test file proves "the capture's warm-up runs are not steps" for that part; this is the test that fails when a part is
missing from what ``AvatarTrainer._capture`` preserves: every counter is compared as an integer after every step.  The losses are
held to the bound tests/test_gpu_train_loop_fused.py and tests/test_gpu_pose_train.py hold the same comparison to, 1e-4 relative per
step (both sides compute in fp32, the graph's workspaces are sized by another capacity hint).  The schedule is the reference's
``human_male`` one (first decision at iteration 1998): no deciding iteration inside the run, the set never changes."""
import json
import math
import os

import numpy as np
import pytest
import torch

import lpips_case as lc
from sings_amd import frame_feed as ff
from sings_amd import patch_sampler as ps
from test_gpu_density_schedule import _schedule
from test_gpu_frame_feed_train import _quantised, _reset
from test_gpu_patch_sampler import NPATCH, PATCH
from test_gpu_pose_train import POSE_LRS, _pose_scene, _table
from test_gpu_subdivide_train import _mesh_scene
from test_gpu_train_loop import H, W, _modules

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
F, K, STEPS, SEED = 8, 2, 6, 9


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def scene():
    """The pose scene with the mesh scene's anchors, its eight target frames as bytes, and the schedule's configuration."""
    sc = _pose_scene()
    mesh = _mesh_scene(np.load(os.path.join(HERE, "golden", "topology_golden.npz")))
    sc.update({k: mesh[k] for k in ("xyz", "w", "faces", "labels")})
    try:
        store = ff.FrameStore(*_quantised(sc, DEV), device=DEV)
    finally:
        _reset()
    with open(os.path.join(HERE, "golden", "density_schedule_golden.json")) as f:
        return sc, store, json.load(f)["human_male"]


def _trainer(sc, store, golden, use_graph):
    from sings_amd.lpips import LPIPS
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.topology import MeshState
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    wt = lc.make_weights(0)
    tri, geo, app = _modules(DEV)
    mod = AvatarStep(_t(sc["xyz"]), _t(sc["w"]), tri, geo, app, lpips_w=1.0, lpips_patch_size=PATCH,
                     lpips=LPIPS.from_tensors(wt["convs"], wt["lins"], wt["shift"], wt["scale"], device=DEV)).to(DEV)
    feed = ff.FrameFeed(store, seed=SEED, frames_per_step=K)
    cam = sc["cam"]
    consts = dict(view=_t(cam["world_view_transform"]), proj=_t(cam["full_proj_transform"]), campos=_t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=feed.bg,
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    tr = AvatarTrainer(mod, settings, feed.bg, POSE_LRS, smpl_scale=_t(sc["smpl_scale"]), use_graph=use_graph, sh_degree=0,
                       max_sh_degree=1, optimizer="fused", poses=_table(sc, DEV), frames=feed,
                       mesh=MeshState.from_faces(_t(sc["faces"]), _t(sc["labels"])),
                       lpips_sampler=ps.DevicePatchSampler(NPATCH, PATCH, 0.9, seed=SEED + 1, device=DEV))
    tr.set_density_schedule(_schedule(golden))
    return tr


def test_a_capture_with_every_part_attached_counts_no_step_twice(scene):
    from sings_amd import rasterizer as rz
    sc, store, golden = scene
    bgs = [torch.rand(K, 3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(i)) for i in range(STEPS)]
    want = ff.indices_host(F, SEED, 0, STEPS * K).reshape(STEPS, K).tolist()
    eager = []
    try:
        for use_graph in (False, True):
            tr = _trainer(sc, store, golden, use_graph)
            feed, sampler, graph = tr.frames, tr.lpips_sampler, None
            for it in range(STEPS):
                loss = float(tr.step_next(lpips_bg=bgs[it])["loss"])
                assert feed.counter == K * (it + 1) and feed.last_indices.tolist() == want[it], it
                ints = dict(sampler=sampler.counter, origins=sampler.last_origins.cpu().tolist(), steps=list(tr.opt.steps),
                            gate=int(tr.m.stats_gate.item()))
                if not use_graph:
                    assert tr.captured is None
                    eager.append((loss, ints))
                    continue
                assert ints == eager[it][1], (it, ints, eager[it][1])
                if it < 2:                                       # (the two sizing steps)
                    assert tr.captured is None
                else:                                            # ONE capture, at the third step; three replays
                    graph = tr.captured if it == 2 else graph
                    assert graph is not None and tr.captured is graph
                rel = abs(loss - eager[it][0]) / abs(eager[it][0])
                print(f"step {it}: eager {eager[it][0]:.7f} graph {loss:.7f} rel {rel:.1e}")
                assert math.isfinite(loss) and rel <= 1e-4, (it, loss, eager[it][0])
            rz.check_deferred_overflow(DEV)
            assert tr.iteration == STEPS and tr.density_log == [] and int(tr.m.xyz.shape[0]) == 86
            assert eager[-1][1]["sampler"] == STEPS and eager[-1][1]["steps"] == [STEPS] * 6 and eager[-1][1]["gate"] == 0
            _reset()
            del tr
    finally:
        _reset()
