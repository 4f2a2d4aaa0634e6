"""Times a scene of avatars on the GPU box:  python tools/scene_anim_time.py [--reps N] [--frames F] [--out FILE]

Three avatars of 150 000 Gaussians (J = 52, 52, 24; ``scene.avatar_scene``, side by side) at 512 x 896, F frames with their own poses
and translations, 8-bit BGR frames out:

    scene_K1 / scene_K8   ``scene_anim.SceneAnimator.render_frames_batched`` with 1 and 8 frames per launch (2 streams): the avatars
                          stay canonical, one fused preprocess skins all of them into one set of records;
    posed_then_raster     what the tree offered before for the same frames: ``posed.forward_chunk`` per avatar (chunks of 8 frames),
                          then ``renderer.get_render_pkgs`` per frame -- the posed sets and their SH blocks concatenated, one plain
                          raster call -- and ``frames_to_u8``.

The three arms give the same bytes (asserted before anything is timed).  Every timed block renders the F frames, starts and ends in a
device synchronise and is bracketed by HIP events; warm-up first; the arms ALTERNATE block by block; medians over ``--reps`` (>= 5)
blocks with min and max, and a difference counts as resolved only when the two arms' [min, max] ranges do not overlap.  Writes
profiles/scene_anim_time.json (``--out``).

``--trace-workload``: no timing -- 20 K = 8 forwards each of ``SkinnedFramesEngine`` and of a one-avatar ``SceneFramesEngine`` on the
same 150 000 Gaussians, in turn, for a kernel trace (``rocprofv3 --kernel-trace --stats -- python tools/scene_anim_time.py
--trace-workload``): sg_scene_fwd_kernel against sg_skin_fwd_kernel at the same P."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

W, H, N = 512, 896, 150000
JOINTS = (52, 52, 24)
OFFSETS = ((-0.25, 0.0, 0.0), (0.0, 0.0, 0.15), (0.25, 0.0, -0.15))


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), res


def alternate(arms, reps, warmup=2):
    """{name: fn} -> {name: {median_ms, min, max}}: every arm warmed up, then ``reps`` rounds of one block per arm, in turn."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(timed(fn)[0])
    return {k: {"median_ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}


def verdict(res, fast, slow):
    """The ratio of the medians and whether the blocks' spread resolves it."""
    f, s = res[fast], res[slow]
    return {"ratio": s["median_ms"] / f["median_ms"], "resolved": bool(f["max"] < s["min"] or s["max"] < f["min"]),
            "faster": fast if f["median_ms"] < s["median_ms"] else slow}


def build_scene(dev, F, n=N):
    """-> (canons, per-avatar A [F,J,4,4], per-avatar transl [F,3], camera dict, bg)."""
    from sings_amd.body import joint_transforms
    from sings_amd.scene import avatar_scene
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    canons, As, transls, cam = [], [], [], None
    for i, (J, off) in enumerate(zip(JOINTS, OFFSETS)):
        s = avatar_scene(N=n, J=J, W=W, H=H, seed=4 + i)
        rs = np.random.RandomState(40 + i)
        jr = t(s["joints_rest"])
        As.append(torch.stack([joint_transforms(t(rs.normal(0, 0.2, J * 3).astype(np.float32)), jr, tuple(s["parents"]))
                               for _ in range(F)]).reshape(F, J, 4, 4).contiguous())
        transls.append(t((s["transl"][None] + np.asarray(off)[None] + rs.normal(0, 0.03, (F, 3))).astype(np.float32)))
        canons.append(dict(xyz_canon=t(s["xyz_canon"]), rotmat_canon=None, scales=t(s["scales"]), opacity=t(s["opacities"]),
                           shs=t(s["shs"]), lbs_weights=t(s["lbs_weights"]), active_sh_degree=0))
        if cam is None:
            cam = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in s["cam"].items()}
            cam.update(image_width=W, image_height=H)
    return canons, As, transls, cam, torch.ones(3, device=dev)


def scene_frames(animator, As, transls, cam, bg, K):
    F = int(As[0].shape[0])
    jobs = ((cam, [(A[f], tr[f], None, None) for A, tr in zip(As, transls)]) for f in range(F))
    return [img for _, img in animator.render_frames_batched(jobs, bg, frames_per_launch=K, out="bgr8")]


def posed_then_raster(canons, As, transls, cam, bg, chunk=8):
    """posed.forward_chunk per avatar, renderer.get_render_pkgs per frame, frames_to_u8 per frame."""
    from sings_amd.posed import forward_chunk, frames_to_u8
    from sings_amd.renderer import get_render_pkgs
    F = int(As[0].shape[0])
    zero = torch.zeros(3, device=bg.device)
    out = []
    with torch.no_grad():
        for c0 in range(0, F, chunk):
            posed = [forward_chunk(dict(xyz_canon=c["xyz_canon"], xyz_offsets=None, rot6d_canon=None, scales=c["scales"], opacity=c["opacity"],
                                        shs=c["shs"]), c["lbs_weights"], A[c0:c0 + chunk], transl=tr[c0:c0 + chunk], isotropic=True)
                     for c, A, tr in zip(canons, As, transls)]
            for i in range(int(posed[0]["xyz"].shape[0])):
                frame = [dict(xyz=p["xyz"][i], shs=p["shs"][i], opacity=p["opacity"][i], scales=p["scales"][i], rotq=p["rotq"][i],
                              active_sh_degree=0) for p in posed]
                pkg = get_render_pkgs(cam, frame, [zero] * len(frame), [None] * len(frame), bg)
                out.append(frames_to_u8(pkg["render"], bgr=True))
    return out


def trace_workload(dev, K=8, rounds=20):
    from sings_amd.engine import SkinnedFramesEngine
    from sings_amd.renderer import _settings
    from sings_amd.scene_anim import SceneFramesEngine
    canons, As, transls, cam, bg = build_scene(dev, K)
    c, A, tr = canons[0], As[0], transls[0]
    cap = 16 * N
    rs = _settings(cam, bg, 1.0, 0)
    one = SkinnedFramesEngine(N, JOINTS[0], W, H, 16, K, dev, cap)
    one.set_camera(rs)
    one.set_frames(c["xyz_canon"], None, c["lbs_weights"], A, None, tr)
    scene = SceneFramesEngine([(N, JOINTS[0], None)], W, H, 16, K, dev, cap)
    scene.set_camera(rs)
    scene.set_frames([dict(canon=c, A=A, transl=tr)])
    for _ in range(rounds):
        Rs = one.forward(c["shs"], c["opacity"], c["scales"], sync_num_rendered=True)
        Rq = scene.forward(sync_num_rendered=True)
        assert Rs == Rq and max(Rs) <= cap, (Rs, Rq)
    assert torch.equal(one.color, scene.color)
    print(json.dumps({"trace_workload": {"K": K, "rounds": rounds, "P": N, "pairs_per_frame": Rs}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--gaussians", type=int, default=N, help="per avatar (the figures of LAB.md: the default)")
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_anim_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "scene_anim_time.py needs the GPU"
    dev = torch.device("cuda:0")
    if a.trace_workload:
        return trace_workload(dev)
    from sings_amd import rasterizer as rz
    from sings_amd.scene_anim import SceneAnimator
    canons, As, transls, cam, bg = build_scene(dev, a.frames, a.gaussians)
    rz.set_overflow_check("sync"); rz.reset_overflow_state()
    animators = {K: SceneAnimator(canons, streams=2) for K in (1, 8)}
    arms = {"scene_K1": lambda: scene_frames(animators[1], As, transls, cam, bg, 1),
            "scene_K8": lambda: scene_frames(animators[8], As, transls, cam, bg, 8),
            "posed_then_raster": lambda: posed_then_raster(canons, As, transls, cam, bg)}
    frames = {k: torch.stack(fn()) for k, fn in arms.items()}
    ref = frames["posed_then_raster"]
    out = {"reps": a.reps, "frames": a.frames, "avatars": [{"P": a.gaussians, "J": J} for J in JOINTS], "W": W, "H": H,
           "device_name": torch.cuda.get_device_name(0), "bytes": int(ref.numel()), "not_background": bool((ref != 255).any()),
           "bytes_that_differ": {k: int((v != ref).sum()) for k, v in frames.items() if k != "posed_then_raster"}}
    assert out["not_background"] and not any(out["bytes_that_differ"].values()), out
    del frames, ref
    res = alternate(arms, a.reps)
    for k in arms:
        res[k]["frames_per_s"] = a.frames / (res[k]["median_ms"] * 1e-3)
        res[k]["ms_per_frame"] = res[k]["median_ms"] / a.frames
    res["posed_then_raster_over_scene_K8"] = verdict(res, "scene_K8", "posed_then_raster")
    res["posed_then_raster_over_scene_K1"] = verdict(res, "scene_K1", "posed_then_raster")
    res["scene_K1_over_scene_K8"] = verdict(res, "scene_K8", "scene_K1")
    out["times"] = res
    out["pair_capacity"] = {str(K): an.cap for K, an in animators.items()}
    out["long_rows_hint_kept"] = {str(K): bool(an.long_rows) for K, an in animators.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
