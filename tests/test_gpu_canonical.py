"""The canonical turntable (sings_amd/canonical.py) and the trainer's opt-in outputs (sings_amd/run_outputs.py).

Turntable.  That K cameras of one set in one launch are the K single-camera renders, and that the posed side outputs of a fused call are
the posed values, is what tests/test_gpu_frames.py holds (``test_raster_frames_equal_single_camera_calls_bit_for_bit``,
``test_posed_side_outputs_of_a_k_frame_forward``).  Here, on an ``avatar_scene(N=2000, J=24)`` with 6-D rotations, five orbit cameras
at 64 x 48 and two cameras per launch (the last launch is padded): every frame of ``OrbitRenderer.render`` EQUALS the raw image of the
drop-in ``renderer.render`` for that camera on the same posed values, at ``scaling_modifier`` 1.0 and 0.5, also when the renderer starts
with a capacity far below the first launch's pair count.

Trainer.  The smallest configuration of tests/test_gpu_frame_feed_train.py (graph on, a ``FrameFeed``, the tri-plane's learning rate 0 so
that two runs are the same bits: that file's docstring): the written names are what ``due`` predicts, the training picture of step 3 is
the numpy sheet of what a second trainer stepped by hand holds at that step, and the losses are those of a run without outputs."""
import os

import numpy as np
import pytest
import torch

from sheet_case import quantise, sheets
from sings_amd import canonical as cn
from sings_amd import frame_feed as ff
from test_gpu_density_schedule import _schedule, _trainer as _density_trainer, golden, scene as density_scene      # noqa: F401
from test_gpu_frame_feed_train import SEED, STILL_LRS, _feed_trainer, _quantised, _reset
from test_gpu_pose_train import _bits_equal, _pose_scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N, J, W, H, NFRAMES, K = 2000, 24, 64, 48, 5, 2


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def orbit():
    """The scene, its posed values, the five cameras, and the drop-in renders (raw) of every camera at both modifiers."""
    from sings_amd.camera import get_rotating_camera
    from sings_amd.renderer import render
    from sings_amd.scene import avatar_scene
    s = avatar_scene(N=N, J=J, W=W, H=H, isotropic=False)
    rs = np.random.RandomState(6)
    canon = {"xyz_canon": _t(s["xyz_canon"]), "rotmat_canon": _t(rs.normal(0, 1, (N, 6)).astype(np.float32)), "scales": _t(s["scales"]),
             "opacity": _t(s["opacities"]), "shs": _t(s["shs"]), "lbs_weights": _t(s["lbs_weights"]), "active_sh_degree": 3}
    A = cn.static_A("da_pose", _t(s["joints_rest"]), torch.eye(4, device=DEV).repeat(J, 1, 1), s["parents"])
    bg = _t(np.array([0.2, 0.7, 0.4], np.float32))
    cams = get_rotating_camera(img_size=(H, W), device=DEV, nframes=NFRAMES)
    try:
        posed = cn.pose_once(canon, A, cams[0], bg)
        with torch.no_grad():
            raws = {sm: [render(posed["xyz"], posed["shs"], posed["opacity"], posed["scales"], posed["rotq"], c, scaling_modifier=sm,
                                bg_color=bg, active_sh_degree=3)["render_raw"].clone() for c in cams] for sm in (1.0, 0.5)}
    finally:
        _reset()
    return dict(canon=canon, A=A, bg=bg, cams=cams, posed=posed, raws=raws)


def _is_background(img, bg):
    return bool((img == bg[:, None, None]).all())


def test_pose_once_is_the_fused_calls_posed_values(orbit):
    from sings_amd.renderer import get_render_pkg_fused
    try:
        with torch.no_grad():
            pkg = get_render_pkg_fused(orbit["cams"][0], orbit["canon"], orbit["A"], orbit["bg"], return_posed=True)
    finally:
        _reset()
    for k in ("xyz", "rotq", "scales"):
        assert _bits_equal(orbit["posed"][k], pkg[k]) and torch.isfinite(pkg[k]).all(), k
    assert float(orbit["posed"]["xyz"].abs().max()) > 0.1 and tuple(orbit["posed"]["rotq"].shape) == (N, 4)


@pytest.mark.parametrize("capacity", [None, 256])
def test_every_orbit_frame_equals_the_drop_in_render(orbit, capacity):
    r = cn.OrbitRenderer(orbit["posed"], W, H, 16, K=K, device=DEV, capacity_pairs=capacity)
    first_cap = r.cap
    for sm in (1.0, 0.5):
        got = list(r.render(orbit["posed"], orbit["cams"], orbit["bg"], scaling_modifier=sm))
        assert [i for i, _ in got] == list(range(NFRAMES))           # (the padding of the last launch is not handed out)
        for i, img in got:
            assert tuple(img.shape) == (3, H, W) and torch.equal(img, orbit["raws"][sm][i]), (sm, i)
            assert not _is_background(img, orbit["bg"]), (sm, i)
    assert not torch.equal(orbit["raws"][1.0][0], orbit["raws"][0.5][0]) and not torch.equal(orbit["raws"][1.0][0], orbit["raws"][1.0][2])
    assert r.launches >= 2 * 3
    if capacity is not None:                                         # the first launch overflowed and was rendered again, grown
        counts = r.engine.num_rendered()
        print(f"pair counts of the last launch {counts}, capacity {first_cap} -> {r.cap}, launches {r.launches}, redone {r.redone}")
        assert max(counts) > first_cap and r.redone >= 1 and r.cap >= max(counts)
    else:
        assert r.redone == 0 and r.launches == 2 * 3


def test_render_canonical_is_the_rounded_raw_frames(orbit):
    frames = list(cn.render_canonical(orbit["canon"], orbit["A"], orbit["bg"], nframes=NFRAMES, img_size=(H, W), frames_per_launch=K))
    assert [i for i, _ in frames] == list(range(NFRAMES))
    for i, u8 in frames:
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3)
        assert np.array_equal(u8.cpu().numpy(), quantise(orbit["raws"][1.0][i].cpu().numpy(), "round").transpose(1, 2, 0)), i


def test_progress_sheet_is_the_numpy_sheet_of_the_four_renders(orbit):
    from sings_amd.camera import get_rotating_camera
    from sings_amd.renderer import render
    cams = get_rotating_camera(img_size=(H, W), device=DEV, nframes=2, angle_limit=np.pi)
    p = orbit["posed"]
    try:
        with torch.no_grad():
            four = [render(p["xyz"], p["shs"], p["opacity"], p["scales"], p["rotq"], c, scaling_modifier=sm, bg_color=orbit["bg"],
                           active_sh_degree=3)["render_raw"].cpu().numpy() for c in cams for sm in (0.5, 1.0)]
    finally:
        _reset()
    got = cn.progress_sheet(orbit["canon"], orbit["A"], orbit["bg"], nframes=2, img_size=(H, W))
    want = sheets(np.stack(four), nrow=4, padding=2, pad_value=0.0, quant="round")[0]
    assert tuple(got.shape) == (H + 4, 4 * (W + 2) + 2, 3) and np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(four[0], four[1])


# ---- the trainer's outputs ---------------------------------------------------------------------------------------------------------
STEPS, VIZ, PROGRESS, CANON = 7, 3, 2, 3


class _Quiet:
    """Outputs that write nothing: the trainer keeps the step's render as it does for ``RunOutputs``."""

    def after_step(self, trainer, t):
        pass


def _outputs(sc, logdir, written, **kw):
    from sings_amd.run_outputs import RunOutputs
    A = cn.static_A("da_pose", _t(sc["joints"]), torch.inverse(_t(sc["post"])), sc["parents"])
    ro = RunOutputs(logdir, A, _t(np.array([1.0, 1.0, 1.0], np.float32)), viz_interval=VIZ, progress_interval=PROGRESS,
                    canon_nframes=CANON, write=lambda path, array: written.__setitem__(os.path.relpath(path, logdir), array.copy()), **kw)
    ro.canon_size, ro.progress_size, ro.frames_per_launch = (48, 64), (32, 32), 2
    return ro


def _ply_rows(path):
    with open(path) as f:
        for line in f:
            if line.startswith("element vertex"):
                return int(line.split()[2])
    raise AssertionError(path)


def test_a_run_writes_what_due_predicts_and_learns_what_it_learned_without(tmp_path):
    dev = DEV
    sc = _pose_scene()
    try:
        rgb_u8, mask_u8 = _quantised(sc, dev)
        _reset()
        store = ff.FrameStore(rgb_u8, mask_u8, device=dev)
        # the run with outputs
        written = {}
        tr = _feed_trainer(sc, dev, "fused", True, ff.FrameFeed(store, seed=SEED), lrs=STILL_LRS)
        ro = _outputs(sc, str(tmp_path), written)
        tr.set_outputs(ro)
        losses, graphs = [], []
        for t in range(STEPS):
            losses.append({k: v.clone() for k, v in tr.step_next().items()})
            graphs.append(tr.captured)
        assert graphs[2] is not None and all(g is graphs[2] for g in graphs[2:]), "output events at 3, 4 and 6 kept the captured graph"
        names = set(written) | {os.path.relpath(os.path.join(d, f), str(tmp_path)) for d, _, fs in os.walk(str(tmp_path)) for f in fs}
        want = set()
        for t in range(STEPS):
            due = ro.due(t)
            if "viz" in due:
                want |= {f"train/{t:06d}.png", f"meshes/human_pcd_{t:06d}_splat.ply"} | {f"canon/{i:05d}.png" for i in range(CANON)}
            if "progress" in due:
                want.add(f"train_progress/{t:06d}.png")
        assert names == want and len(want) == 3 * 2 + CANON + 4
        n = int(tr.m.xyz.shape[0])
        assert _ply_rows(str(tmp_path / "meshes" / "human_pcd_000003_splat.ply")) == n
        Hf, Wf = int(tr.inputs.gt.shape[-2]), int(tr.inputs.gt.shape[-1])
        assert written["train/000003.png"].shape == (Hf, 2 * Wf, 3) and written["canon/00001.png"].shape == (48, 64, 3)
        assert written["train_progress/000004.png"].shape == (32 + 4, 4 * 34 + 2, 3)
        assert written["canon/00000.png"].min() < 255, "the avatar is in the turntable's view"
        picture3 = written["train/000003.png"]
        _reset()
        del tr
        # a second, identical trainer stepped by hand up to step 3: its composited ground truth and its render, through numpy
        other = _feed_trainer(sc, dev, "fused", True, ff.FrameFeed(store, seed=SEED), lrs=STILL_LRS)
        other.set_outputs(_Quiet())
        for t in range(4):
            other.step_next()
        inp = other.inputs
        composite = (inp.gt * inp.mask + other.bg[:, None, None] * (1.0 - inp.mask)).cpu().numpy()
        render = other.last_render.cpu().numpy()
        assert render.shape == composite.shape == (3, Hf, Wf)
        want3 = sheets(composite[None], render[None], tiles_per_sheet=2, nrow=2, padding=0, quant="trunc")[0]
        assert np.array_equal(picture3, want3)
        assert np.array_equal(want3[:, Wf:], quantise(np.clip(render, 0, 1), "trunc").transpose(1, 2, 0))
        _reset()
        del other
        # the same run without outputs: the same losses, bit for bit
        plain = _feed_trainer(sc, dev, "fused", True, ff.FrameFeed(store, seed=SEED), lrs=STILL_LRS)
        assert plain.outputs is None
        for t in range(STEPS):
            ld = plain.step_next()
            assert plain.last_render is None
            for k in ld:
                assert _bits_equal(ld[k], losses[t][k]), (t, k, float(ld[k]), float(losses[t][k]))
    finally:
        _reset()


def test_the_outputs_of_a_deciding_iteration_show_the_set_before_the_action(density_scene, golden, tmp_path):
    """The compressed schedule's first action is the prune at iteration 3, a ``viz`` iteration here: the splat file of that iteration
    holds the ``n_old`` rows of the log entry, and the pictures were rendered from that set."""
    try:
        sc, _ = density_scene
        tr = _density_trainer(density_scene, True, _schedule(golden))
        written = {}
        ro = _outputs(sc, str(tmp_path), written)
        ro.progress_interval = None
        tr.set_outputs(ro)
        n0 = int(tr.m.xyz.shape[0])
        tr.run(4)
        entry = tr.density_log[0]
        assert entry["t"] == 3 and entry["n_old"] == n0 and entry["n_new"] < n0 and int(tr.m.xyz.shape[0]) == entry["n_new"]
        assert _ply_rows(str(tmp_path / "meshes" / "human_pcd_000003_splat.ply")) == entry["n_old"]
        assert set(written) == {"train/000000.png", "train/000003.png"} | {f"canon/{i:05d}.png" for i in range(CANON)}
        assert written["train/000003.png"].shape == (64, 128, 3)
    finally:
        _reset()
