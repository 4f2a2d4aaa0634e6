"""The pose refinement on the GPU (``pose_refine.RefineEngine`` / ``refine_pose`` / ``refine_kit``) against the host definition, on
``pose_refine_case.kit``: the level-2 model, 24 joints, four frames of 40 x 56.  Floats follow ``body_case.held``: the device may be at
most twice as far from the fp64 twin as the fp32 twin is, both measured here.  What is bit-equal is asserted bit-equal: a replayed
graph against eager iterations, a batch run again after an overflow against one that never overflowed, the entries no gradient
reaches against the start."""
import json
import math
import os

import numpy as np
import pytest
import torch

import body_case as bc
import pose_refine_case as prc
from sings_amd import _marshal
from sings_amd import kit as KIT
from sings_amd import pose_refine as PR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SPEC = PR.RefineSpec.smpl()
_TWIN = {}


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def _targets(kit, spec):
    return PR.keypoint_targets(torch.tensor(kit["keypoints"], dtype=torch.float64), torch.tensor(kit["scores"], dtype=torch.float64), spec)


def twin_gradient(kit, spec, poses, dtype):
    """Per frame at ``poses`` [F,72] -> (terms [F,2], dkeypoint [F,72], dsilhouette [F,72]) numpy, by ``host_loss`` and autograd."""
    model = PR.host_model(kit["model"])
    target, used = _targets(kit, spec)
    terms, gk, gs = [], [], []
    for f in range(len(poses)):
        pose = torch.tensor(poses[f], dtype=dtype, requires_grad=True)
        a, b, _ = PR.host_loss(model, kit["betas"], pose, kit["transl"][f], prc.CAMERA, torch.tensor(kit["masks"][f], dtype=dtype),
                               target[f].to(dtype), used[f], spec, kit["extra"], dtype)
        ga, = torch.autograd.grad(a, pose, retain_graph=True)
        gb, = torch.autograd.grad(b, pose)
        terms.append([a.item(), b.item()]); gk.append(ga.numpy()); gs.append(gb.numpy())
    return np.array(terms), np.stack(gk), np.stack(gs)


def twin_loop(kit, spec, iterations, dtype):
    """``refine_pose_host``'s loop with every iteration's terms kept -> (pose [F,72], terms [iterations,F,2]); computed once."""
    key = (id(kit), iterations, dtype)
    if key in _TWIN:
        return _TWIN[key]
    model = PR.host_model(kit["model"])
    target, used = _targets(kit, spec)
    gm, lo, hi = PR._spec_tensors(spec, dtype, "cpu")
    F = len(kit["start"])
    out, terms = np.zeros((F, 72)), np.zeros((iterations, F, 2))
    for f in range(F):
        pose = torch.tensor(kit["start"][f], dtype=dtype, requires_grad=True)
        m, v = torch.zeros_like(pose), torch.zeros_like(pose)
        mask = torch.tensor(kit["masks"][f], dtype=dtype)
        for it in range(1, iterations + 1):
            a, b, _ = PR.host_loss(model, kit["betas"], pose, kit["transl"][f], prc.CAMERA, mask, target[f].to(dtype), used[f], spec,
                                   kit["extra"], dtype)
            g, = torch.autograd.grad(a + b, pose)
            terms[it - 1, f] = a.item(), b.item()
            with torch.no_grad():
                g = g * PR.gate(pose, gm, lo, hi)
                m = 0.9 * m + (1 - 0.9) * g
                v = 0.999 * v + (1 - 0.999) * g * g
                pose -= (spec.lr / (1 - 0.9 ** it)) * m / (v.sqrt() / math.sqrt(1 - 0.999 ** it) + 1e-8)
        out[f] = pose.detach().numpy()
    _TWIN[key] = out, terms
    return _TWIN[key]


def device_inputs(kit):
    return dict(betas=_t(kit["betas"]), global_orient=_t(kit["start"][:, :3]), body_pose=_t(kit["start"][:, 3:]), transl=_t(kit["transl"]),
                camera=prc.CAMERA, masks=_t(kit["masks"]), keypoints=_t(kit["keypoints"]), scores=_t(kit["scores"]))


def engine_for(kit, spec, K, iterations, capture, capacity=None):
    return PR.RefineEngine(kit["model"], _t(kit["betas"]), prc.CAMERA, spec, kit["extra"], K, iterations, capture, capacity)


def load(engine, kit, spec, frames):
    target, used = _targets(kit, spec)
    engine.load(kit["start"][frames], kit["transl"][frames], kit["masks"][frames], target[frames], used[frames])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("J,spec,iterations", [(24, SPEC, 0), (52, PR.RefineSpec.smplh(), 3)], ids=["smpl", "smplh"])
def test_one_iterations_gradient(J, spec, iterations):
    """dL/dpose [K,72] of both terms, each held, and their sum; for the SMPL-H preset on the 52-joint level model (the pose padded to
    156 entries) also after three iterations, at the poses the device has reached."""
    kit = prc.kit(J=J, spec=spec)
    engine = engine_for(kit, spec, 4, max(iterations, 1), False)
    load(engine, kit, spec, slice(0, 4))
    poses = kit["start"]
    for _ in range(iterations):
        engine.iterate()
        poses = engine.pose.cpu().numpy()
    terms, g_kp, g_sil = (x.cpu().numpy() for x in engine.gradient())
    t64, k64, s64 = twin_gradient(kit, spec, poses, torch.float64)
    t32, k32, s32 = twin_gradient(kit, spec, poses, torch.float32)
    what = f"J = {J}, after {iterations} iterations: "
    bc.held(terms, t32, t64, what + "terms")
    bc.held(g_kp, k32, k64, what + "dkeypoint/dpose")
    bc.held(g_sil, s32, s64, what + "dsilhouette/dpose")
    bc.held(g_kp + g_sil, k32 + s32, k64 + s64, what + "dL/dpose")
    assert np.abs(k64).max() > 0 and np.abs(s64).max() > 0


@pytest.mark.parametrize("step", [1, 7])
def test_update_launch(step):
    """Gate and Adam of ``refine_pose_host``, written out in fp32 torch on the CPU, to 2 ulp; an entry the mask or a limit closes and
    whose moments are zero keeps its bits, and so do its moments."""
    rs = np.random.RandomState(step)
    K = 3
    gm, lo, hi = PR._spec_tensors(SPEC, torch.float32, "cpu")
    pose = torch.tensor(0.3 * rs.randn(K, 72), dtype=torch.float32)
    pose[:, 12] = torch.tensor([0.5, -0.2, 3.0])                    # a knee's x inside [0, 160 deg], below and above it
    grad = torch.tensor(rs.randn(K, 72), dtype=torch.float32)
    closed = (PR.gate(pose, gm, lo, hi) == 0)
    assert closed[1, 12] and closed[2, 12] and not closed[0, 12] and closed[:, 0].all()
    m = torch.tensor(0.1 * rs.randn(K, 72), dtype=torch.float32)
    v = torch.tensor(0.01 * rs.rand(K, 72), dtype=torch.float32)
    m[closed], v[closed] = 0.0, 0.0
    m[1, 12], v[1, 12] = 0.05, 0.002                                 # closed by its limit, but still carried by its momentum
    g = grad * PR.gate(pose, gm, lo, hi)
    m_ref = 0.9 * m + (1 - 0.9) * g
    v_ref = 0.999 * v + (1 - 0.999) * g * g
    p_ref = pose - (SPEC.lr / (1 - 0.9 ** step)) * m_ref / (v_ref.sqrt() / math.sqrt(1 - 0.999 ** step) + 1e-8)
    d = lambda t: t.clone().to(DEV)
    pose_d, m_d, v_d, step_d = d(pose), d(m), d(v), torch.tensor([step - 1], dtype=torch.int32, device=DEV)
    terms, table = torch.tensor(rs.rand(K, 2), dtype=torch.float32, device=DEV), torch.zeros(8, K, 2, device=DEV)
    _marshal.sil_pose_update(SPEC.lr, pose_d, d(grad), m_d, v_d, d(gm), d(lo), d(hi), step_d, terms, table)
    assert step_d.item() == step
    assert torch.equal(table[step - 1], terms) and int((table != 0).any(-1).any(-1).sum()) == 1
    for name, dev, ref in (("pose", pose_d, p_ref), ("m", m_d, m_ref), ("v", v_d, v_ref)):
        dev = dev.cpu().numpy().astype(np.float64)
        ulp = np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(dev - ref.numpy().astype(np.float64)) / ulp).max())
        print(f"step {step}: {name} off by at most {worst:.2f} ulp")
        assert worst <= 2.0, name
    still = closed.clone(); still[1, 12] = False
    assert np.array_equal(_bits(pose_d.cpu().numpy())[still.numpy()], _bits(pose.numpy())[still.numpy()])
    assert (m_d.cpu()[still] == 0).all() and (v_d.cpu()[still] == 0).all()
    assert pose_d[1, 12].item() != pose[1, 12].item()


def test_the_loop_against_the_twin():
    """25 iterations, four frames three at a time: the second batch is one frame and two copies whose results are dropped."""
    kit, iters = prc.kit(), 25
    trace = []
    go, bp, report = PR.refine_pose(kit["model"], **device_inputs(kit), spec=SPEC, extra_joint_vertex_ids=kit["extra"], frames_per_launch=3,
                                    iterations=iters, trace=trace)
    assert [t.shape for t in trace] == [(iters, 3, 2), (iters, 1, 2)]
    terms = np.concatenate(trace, 1)
    p64, t64 = twin_loop(kit, SPEC, iters, torch.float64)
    p32, t32 = twin_loop(kit, SPEC, iters, torch.float32)
    bc.held(terms, t32, t64, "the terms of 25 iterations")
    pose = np.concatenate([go, bp], 1)
    enabled = SPEC.enabled()
    err0, err, err64 = (prc.pose_error(p, kit["true"], enabled) for p in (kit["start"], pose, p64))
    print(f"pose error over the enabled entries: start {err0}, device {err}, fp64 twin {err64}")
    assert np.allclose(err0, prc.DELTA, atol=1e-6) and (err < err0).all()
    assert np.array_equal(_bits(pose[:, ~enabled]), _bits(kit["start"][:, ~enabled]))
    assert set(report) == {"first_loss", "last_loss", "first_keypoint_term", "first_silhouette_term", "last_keypoint_term",
                           "last_silhouette_term", "keypoints_used", "max_faces_per_pixel"}
    assert np.array_equal(report["first_keypoint_term"], terms[0, :, 0]) and np.array_equal(report["last_silhouette_term"], terms[-1, :, 1])
    assert (report["last_loss"] < report["first_loss"]).all() and (report["keypoints_used"] > 0).all()
    model = PR.host_model(kit["model"])
    for f in range(4):
        vc, _ = PR.host_forward(model, kit["betas"], torch.tensor(kit["start"][f], dtype=torch.float64), kit["transl"][f], np.eye(3), kit["extra"])
        _, cnt = PR.silhouette_host(vc, model["faces"], prc.INTR, prc.H, prc.W, SPEC.sigma, return_counts=True)
        assert report["max_faces_per_pixel"][f] == int(cnt)


def test_graph_replay_is_bit_equal_to_eager():
    kit, iters = prc.kit(), 6
    out = {}
    for capture in (False, True):
        trace = []
        engine = engine_for(kit, SPEC, 3, iters, capture)
        go, bp, _ = PR.refine_pose(kit["model"], **device_inputs(kit), spec=SPEC, extra_joint_vertex_ids=kit["extra"], engine=engine, trace=trace)
        out[capture] = (go, bp, np.concatenate(trace, 1), engine)
    assert out[True][3].graph is not None and out[False][3].graph is None
    for a, b in zip(out[False][:3], out[True][:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.abs(out[True][1] - kit["start"][:, 3:]).max() > 0.01
    with pytest.raises(RuntimeError, match="only replayed"):
        out[True][3].iterate()
    out[False][3].iterate()                                          # (an engine that was never captured may)


def test_an_overflow_in_mid_batch_gives_the_same_poses():
    kit, iters = prc.kit(), 12
    target, used = _targets(kit, SPEC)
    args = (kit["start"][:3], kit["transl"][:3], kit["masks"][:3], target[:3], used[:3])
    free = engine_for(kit, SPEC, 3, iters, True)
    pose, table, _ = free.run_batch(*args)
    assert free.reruns == 0 and free.peak_pairs >= free.start_pairs > 0
    # a list that holds the starting poses' pairs exactly, when the count grows on the way; else one pair less than the start needs
    capacity = free.start_pairs if free.peak_pairs > free.start_pairs else free.start_pairs - 1
    print(f"pairs at the start {free.start_pairs}, most on the way {free.peak_pairs}; forced capacity {capacity}")
    forced = engine_for(kit, SPEC, 3, iters, True, capacity=capacity)
    pose_f, table_f, _ = forced.run_batch(*args)
    assert forced.reruns >= 1 and forced.work.capacity >= forced.peak_pairs and forced.work.guards_intact()
    assert np.array_equal(_bits(pose), _bits(pose_f)) and np.array_equal(_bits(table), _bits(table_f))


def test_refine_kit_writes_what_load_kit_reads(tmp_path):
    from PIL import Image
    kit = prc.kit()
    root = str(tmp_path)
    for d in ("images", "masks", "score_demo_video", KIT.KEYPOINT_DIR):
        os.makedirs(os.path.join(root, d))
    rgb = np.random.RandomState(2).randint(0, 256, (4, prc.H, prc.W, 3)).astype(np.uint8)
    for f in range(4):
        Image.fromarray(rgb[f], "RGB").save(os.path.join(root, "images", f"{f:06d}.png"))
        Image.fromarray((kit["masks"][f] * 255).astype(np.uint8), "L").save(os.path.join(root, "masks", f"{f:06d}.png"))
        with open(os.path.join(root, KIT.KEYPOINT_DIR, f"{f:06d}.json"), "w") as fh:
            json.dump({"instance_info": [{"keypoints": [[float(x), float(y)] for x, y in kit["keypoints"][f]],
                                          "keypoint_scores": [float(s) for s in kit["scores"][f]]}]}, fh)
    np.savez(os.path.join(root, "score_demo_video", "cameras.npz"), intrinsic=prc.CAMERA["cam_intrinsics"], extrinsic=np.eye(4),
             height=np.int64(prc.H), width=np.int64(prc.W))
    np.savez(os.path.join(root, "score_demo_video", "poses.npz"), betas=kit["betas"], global_orient=kit["start"][:, :3],
             body_pose=kit["start"][:, 3:], transl=kit["transl"])
    spec = PR.RefineSpec(SPEC.keypoint_map, SPEC.n_joint_rows, SPEC.grad_mask, SPEC.limits, SPEC.lr, 5)
    path, report = PR.refine_kit(root, kit["model"], kit["extra"], spec, frames_per_launch=3)
    assert path == os.path.join(root, "score_demo_video", "poses_optimized.npz") and os.path.exists(path)
    go, bp, _ = PR.refine_pose(kit["model"], **device_inputs(kit), spec=spec, extra_joint_vertex_ids=kit["extra"], frames_per_launch=3)
    loaded = KIT.load_kit(root, "train+val")
    assert np.array_equal(_bits(loaded.smpl["global_orient"].cpu().numpy()), _bits(go))
    assert np.array_equal(_bits(loaded.smpl["body_pose"].cpu().numpy()), _bits(bp))
    assert np.array_equal(loaded.smpl["transl"].cpu().numpy(), kit["transl"]) and np.array_equal(loaded.smpl["betas"].cpu().numpy()[0], kit["betas"])
    assert np.abs(bp - kit["start"][:, 3:]).max() > 0.01
    with pytest.raises(FileExistsError):
        PR.refine_kit(root, kit["model"], kit["extra"], spec)
    # replacing it starts from poses.npz again, not from the refined poses: the same file
    before = open(path, "rb").read()
    PR.refine_kit(root, kit["model"], kit["extra"], spec, frames_per_launch=3, overwrite=True)
    assert np.array_equal(np.load(path)["body_pose"], bp) and len(before) > 0
