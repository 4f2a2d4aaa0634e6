"""``AvatarTrainer(frames=FrameFeed(...)).step_next()`` on the tiny avatar of tests/test_gpu_pose_train.py: eight frames rendered with
the true poses, quantised to bytes and kept in a ``FrameStore``.

Eager parity: a trainer that draws its frames and background itself against one that is handed, through ``step_frames``, the frames
the numpy twin names, out of ``store.frames``, with the twin's background copied into its background tensor -- the same kernels on the
same bits: every loss and every parameter of six steps bit-equal.  One kernel of the step does not add in a fixed order (the
tri-plane backward's float atomics), so that comparison runs with the tri-plane's learning rate at 0; with every group learning the
first step is bit-equal and the trajectory is held to the bound two runs of one trainer are held to.  Captured against eager: the bound of
tests/test_gpu_pose_train.py for the same comparison (1e-4 relative per step: both sides compute in fp32, the graph's workspaces are
sized by another capacity hint), and the frames visited are the same integers."""
import math

import numpy as np
import pytest
import torch

from sings_amd import frame_feed as ff
from test_gpu_pose_train import POSE_LRS, _bits_equal, _pose_scene, _table, _targets, _trainer
from test_gpu_train_loop import H, W, _modules

pytestmark = pytest.mark.gpu

F, SEED = 8, 5


def _quantised(sc, dev):
    """(rgb_u8 [F,H,W,3], mask_u8 [F,H,W]) of the eight target frames and the scene's mask."""
    gts = np.stack(_targets(sc, dev))
    rgb = np.rint(np.clip(gts, 0, 1) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    mask = np.repeat(((sc["mask"] > 0) * 255).astype(np.uint8)[None], F, 0)
    return np.ascontiguousarray(rgb), mask


def _feed_trainer(sc, dev, optimizer, use_graph, frames, bg=None, settings_bg=None, poses=True, lrs=POSE_LRS):
    """tests/test_gpu_pose_train.py's ``_trainer`` with ``frames=``; the feed's bg tensor is the trainer's and the settings' (or the
    tensors the caller names, for the refusals)."""
    from sings_amd.rasterizer import GaussianRasterizationSettings
    from sings_amd.train_loop import AvatarTrainer
    from sings_amd.train_step import AvatarStep
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tri, geo, app = _modules(dev)
    mod = AvatarStep(t(sc["xyz"]), t(sc["w"]), tri, geo, app).to(dev)
    cam = sc["cam"]
    bg = frames.bg if bg is None else bg
    consts = dict(bg=bg if settings_bg is None else settings_bg, view=t(cam["world_view_transform"]),
                  proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    return AvatarTrainer(mod, settings, bg, lrs, smpl_scale=t(sc["smpl_scale"]), use_graph=use_graph, sh_degree=0, max_sh_degree=1,
                         optimizer=optimizer, poses=_table(sc, dev) if poses else None, frames=frames)


def _reset():
    from sings_amd import decode, rasterizer as rz
    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    decode.set_gradient_arena(None, None)


@pytest.fixture(scope="module")
def scene():
    dev = torch.device("cuda:0")
    sc = _pose_scene()
    try:
        rgb_u8, mask_u8 = _quantised(sc, dev)
    finally:
        _reset()
    return sc, ff.FrameStore(rgb_u8, mask_u8, device=dev)


STEPS = 6
STILL_LRS = dict(POSE_LRS, triplane=0.0)                         # the tri-plane held still: see the module docstring


def _parity_run(sc, store, lrs):
    """Six eager ``step_next()`` steps, then six ``step_frames`` steps of a second trainer on the twin's frames and colours ->
    (losses of the first [step]{name: tensor}, of the second, parameters of the first, of the second, parameters at the start)."""
    dev = store.device
    try:
        feed = ff.FrameFeed(store, seed=SEED)
        tr = _feed_trainer(sc, dev, "torch", False, feed, lrs=lrs)
        assert tr.bg is feed.bg and tr.rs.bg is feed.bg
        start = [p.detach().clone() for p in tr.params]
        own, visited, colours = [], [], []
        for _ in range(STEPS):
            own.append({k: v.clone() for k, v in tr.step_next().items()})
            visited.append(int(feed.last_indices[0])); colours.append(feed.bg.cpu().numpy().copy())
        assert feed.counter == STEPS and tr.iteration == STEPS
        own_params = [p.detach().clone() for p in tr.params]
        _reset()
        del tr
        want = ff.indices_host(F, SEED, 0, STEPS)
        assert visited == want.tolist() and len(set(visited)) > 1
        ref, _ = _trainer(sc, dev, "torch", False, lrs=lrs)
        theirs = []
        for it in range(STEPS):
            gt, mask = store.frames([int(want[it])])
            ref.bg.copy_(torch.from_numpy(ff.bg_host(SEED, it)))
            assert np.array_equal(ref.bg.cpu().numpy().view(np.int32), colours[it].view(np.int32))
            theirs.append({k: v.clone() for k, v in ref.step_frames(int(want[it]), gt[0], mask[0]).items()})
        return own, theirs, own_params, [p.detach().clone() for p in ref.params], start
    finally:
        _reset()


def _assert_bit_equal(run):
    own, theirs, own_params, ref_params, _ = run
    losses = [(it, k, float(a[k]), float(b[k])) for it, (a, b) in enumerate(zip(own, theirs)) for k in a if not _bits_equal(a[k], b[k])]
    params = [(i, tuple(a.shape), float((a - b).abs().max())) for i, (a, b) in enumerate(zip(own_params, ref_params)) if not _bits_equal(a, b)]
    print(f"losses that differ (step, name, step_next, step_frames): {losses}")
    print(f"parameters that differ (index, shape, max |difference|): {params}")
    assert all(set(a) == set(b) for a, b in zip(own, theirs)) and len(own_params) == len(ref_params)
    assert not losses and not params


def test_eager_step_next_is_step_frames_on_the_twins_frames_bit_for_bit(scene):
    """Six eager ``step_next()`` steps against six ``step_frames`` steps fed the twin's indices, frames out of ``store.frames`` and
    ``bg_host`` colours: every loss and every parameter bit-equal.  The learning rates are this test's to choose, and the tri-plane's
    is 0 (``STILL_LRS``; every other group at tests/test_gpu_pose_train.py's rates): its gradient is still computed, by a backward
    that adds with float atomics (csrc/sg_decode.hip; the header of tests/test_gpu_train_loop_fused.py: "no two runs are
    bit-identical"), so with a tri-plane that moves two runs of ONE trainer, fed by hand both times, already differ in their last
    bits after the first update -- measured here with every group learning: ``ssim`` off by 1 to 6 ulp from step 2 on, after six
    steps up to 1.1e-5 in a tri-plane grid.  Held still, nothing in the step depends on the order of those additions, and a bit that
    differs is the feed's."""
    run = _parity_run(*scene, STILL_LRS)
    _assert_bit_equal(run)
    _, _, own_params, _, start = run
    for i in (0, -2, -1):                                                # (the anchors and both pose tables)
        assert not torch.equal(start[i], own_params[i]), "the run learns"
    assert all(torch.equal(a, b) for a, b in zip(start[1:7], own_params[1:7])), "the tri-plane's six grids stay"


@pytest.fixture(scope="module")
def parity(scene):
    return _parity_run(*scene, POSE_LRS)


def test_the_first_step_is_bit_equal_and_the_trajectory_within_the_bound_of_two_runs(parity):
    """With every group learning: step 0 starts from the same parameters and its forward adds in a fixed order -- bitwise.  Behind the
    first update two runs of one trainer differ by the tri-plane backward's atomics: tests/test_gpu_train_loop_fused.py's bar for that,
    1e-4 relative per step."""
    own, theirs, own_params, _, start = parity
    for k in own[0]:
        assert _bits_equal(own[0][k], theirs[0][k]), (k, float(own[0][k]), float(theirs[0][k]))
    rel = [abs(float(a["loss"]) - float(b["loss"])) / abs(float(b["loss"])) for a, b in zip(own, theirs)]
    print("step_next vs step_frames, per step: " + " ".join(f"{r:.1e}" for r in rel))
    assert max(rel) <= 1e-4
    for i in (0, -2, -1):                                                # (the anchors and both pose tables)
        assert not torch.equal(start[i], own_params[i]), "the run learns"


def test_the_body_reads_the_feeds_tensors(scene):
    """What ``step_next`` hands the module is what ``step_frames`` is handed for the same frame: the static inputs are the feed's own
    tensors (no copy), and they hold the twin's frame and colour."""
    sc, store = scene
    try:
        feed = ff.FrameFeed(store, seed=SEED)
        tr = _feed_trainer(sc, store.device, "torch", False, feed)
        tr.step_next()
        s, f = tr.inputs, int(ff.indices_host(F, SEED, 0, 1)[0])
        assert s.idx is feed.idx and s.gt.data_ptr() == feed.gt.data_ptr() and s.mask.data_ptr() == feed.mask.data_ptr()
        assert tuple(s.gt.shape) == (3, H, W) and tuple(s.mask.shape) == (H, W) and feed.last_indices.tolist() == [f]
        gt, mask = store.frames([f])
        assert _bits_equal(s.gt, gt[0]) and _bits_equal(s.mask, mask[0])
        assert np.array_equal(tr.bg.cpu().numpy().view(np.int32), ff.bg_host(SEED, 0).view(np.int32))
    finally:
        _reset()


def test_a_captured_trainer_visits_the_eager_trainers_frames(scene):
    sc, store = scene
    dev = store.device
    from sings_amd import rasterizer as rz
    # 27 draws in chunks of three: chunks straddle both epoch boundaries, and the capture (after two eager steps, at counter 6) runs
    # its warm-up over the first one -- the order they rebuild is put back with the counter
    steps, K = 9, 3
    try:
        runs = {}
        for use_graph in (False, True):
            feed = ff.FrameFeed(store, seed=SEED, frames_per_step=K)
            tr = _feed_trainer(sc, dev, "fused", use_graph, feed)
            losses, visited, captured_at = [], [], None
            for it in range(steps):
                losses.append(float(tr.step_next()["loss"]))
                visited.append(feed.last_indices.tolist())
                if use_graph and tr.captured is not None and captured_at is None:
                    captured_at, graph = it, tr.captured
                assert feed.counter == (it + 1) * K                      # (the capture's warm-up runs are not steps)
            rz.check_deferred_overflow(dev)
            if use_graph:                                                # ONE capture, replayed over an epoch boundary
                assert captured_at is not None and tr.captured is graph and steps - captured_at > F // K
            assert np.array_equal(feed.order.cpu().numpy(), ff.order_host(F, SEED, (steps * K - 1) // F))
            runs[use_graph] = (np.array(losses), visited)
            _reset()
            del tr
        want = ff.indices_host(F, SEED, 0, steps * K).reshape(steps, K).tolist()
        assert runs[False][1] == want and runs[True][1] == want
        e, g = runs[False][0], runs[True][0]
        rel = np.abs(e - g) / np.abs(e)
        print("eager vs graph, per step: " + " ".join(f"{r:.1e}" for r in rel))
        assert np.isfinite(e).all() and rel.max() <= 1e-4, (int(rel.argmax()), float(rel.max()))
    finally:
        _reset()


def test_step_and_step_frames_still_work_beside_step_next(scene):
    """A trainer with a feed keeps its other two steps: ``step_frames`` after ``step_next`` copies into tensors of its own, not into the
    feed's, and ``step_next`` then goes on with the feed's sequence."""
    sc, store = scene
    dev = store.device
    try:
        feed = ff.FrameFeed(store, seed=SEED)
        tr = _feed_trainer(sc, dev, "torch", False, feed)
        tr.step_next()
        kept = (feed.idx.clone(), feed.gt.clone(), feed.mask.clone())
        other = (int(kept[0][0]) + 3) % F
        gt, mask = store.frames([other])
        tr.step_frames(other, gt[0], mask[0])
        assert all(torch.equal(a, b) for a, b in zip(kept, (feed.idx, feed.gt, feed.mask))) and feed.counter == 1
        tr.step_next()
        assert feed.counter == 2 and feed.last_indices.tolist() == ff.indices_host(F, SEED, 1, 1).tolist()
    finally:
        _reset()


def test_the_trainers_refusals(scene):
    sc, store = scene
    dev = store.device
    try:
        feed = ff.FrameFeed(store, seed=SEED)
        with pytest.raises(ValueError, match="frames= needs poses=PoseTable"):
            _feed_trainer(sc, dev, "torch", False, feed, poses=False,
                          lrs={k: v for k, v in POSE_LRS.items() if k not in ("global_orient", "body_pose")})
        small = ff.FrameFeed(ff.FrameStore(store.data[:5, ..., :3].contiguous(), store.data[:5, ..., 3].contiguous(), device=dev))
        with pytest.raises(ValueError, match="the frame store holds 5 frames, the pose tables 8 rows"):
            _feed_trainer(sc, dev, "torch", False, small)
        elsewhere = torch.zeros(3, device=dev)
        with pytest.raises(ValueError, match="with random_bg the feed's bg tensor must be both"):
            _feed_trainer(sc, dev, "torch", False, feed, bg=elsewhere, settings_bg=feed.bg)
        with pytest.raises(ValueError, match="with random_bg the feed's bg tensor must be both"):
            _feed_trainer(sc, dev, "torch", False, feed, bg=feed.bg, settings_bg=elsewhere)
        fixed = ff.FrameFeed(store, seed=SEED, random_bg=False)          # (a fixed colour: any tensor, the caller's business)
        _feed_trainer(sc, dev, "torch", False, fixed, bg=elsewhere, settings_bg=elsewhere)
        tr, _ = _trainer(sc, dev, "torch", False)
        with pytest.raises(RuntimeError, match="step_next needs frames=FrameFeed"):
            tr.step_next()
    finally:
        _reset()
