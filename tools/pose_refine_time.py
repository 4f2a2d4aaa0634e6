"""Times the pose refinement on the GPU box, ONE MODE PER PROCESS:  python tools/pose_refine_time.py --mode {kernels,eager,graph}

The case is a kit's: 512 x 896, a body-sized closed mesh (an octahedron subdivided five times onto a bumpy ellipsoid: 4 098 vertices,
8 192 faces, 24 joints of seeded attributes; there is no SMPL file here), about 415 pixels tall, K = 1 and K = 8 frames per launch.

    kernels   the soft silhouette alone: forward, and forward + backward, per launch and per frame
    eager     the loop without a graph: one iteration, and a batch of 100 iterations (``RefineEngine.run_batch``, host reads included)
    graph     the same with the iteration recorded as a HIP graph: one replay, and a batch of 100

An engine that has been captured is only replayed, so the eager and the replayed loop never share buffers: they are different
processes.  Times are host-clock times around work that ends in a device synchronise, medians over ``--reps`` blocks with the blocks'
spread.  There is nothing to compare with (the reference's loop needs pytorch3d's CUDA rasterizer; the host twin cannot run at this
size): absolute times only.  Each mode merges its results into profiles/pose_refine_time.json (``--out``).

Before anything is launched the host twin counts the case (``pair_counts_host``, ``workspace_plan``) and the numbers are printed beside
what the engine allocates."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from sings_amd import _marshal                                    # noqa: E402
from sings_amd import body_model as BM                            # noqa: E402
from sings_amd import pose_refine as PR                           # noqa: E402
from sings_amd import silhouette as S                             # noqa: E402

W, H = 512, 896
INTR = (600.0, 600.0, 256.0, 448.0)
CAMERA = {"cam_intrinsics": np.array([[INTR[0], 0, INTR[2]], [0, INTR[1], INTR[3]], [0, 0, 1.0]]), "image_height": H, "image_width": W,
          "world_view_transform": np.eye(4, dtype=np.float32)}
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)


def body_arrays(levels=5, J=24, B=10, seed=0):
    v, f = OCTA_V, OCTA_F
    for _ in range(levels):
        v, f, _, _ = BM.subdivide_host(v, f, {})
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    bump = 1 + 0.05 * np.sin(5 * v[:, 0]) * np.cos(4 * v[:, 1]) + 0.03 * np.sin(7 * v[:, 2])
    v = (v * bump[:, None] * np.array([0.3, 0.9, 0.2])).astype(np.float32)
    V, rs = len(v), np.random.RandomState(seed)
    # joints along the long axis, each vertex weighted to the two nearest: a pose bends the mesh, it does not tear it
    jy = np.linspace(-0.8, 0.8, J)
    d = np.abs(v[:, 1:2] - jy[None])
    w = np.exp(-(d / 0.08) ** 2).astype(np.float32) + 1e-6
    Jr = np.exp(-(d.T / 0.05) ** 2).astype(np.float32) + 1e-9
    return dict(v_template=v, faces=f, shapedirs=rs.normal(0, 0.003, (V, 3, B)).astype(np.float32), J_regressor=Jr / Jr.sum(1, keepdims=True),
                lbs_weights=w / w.sum(1, keepdims=True), parents=np.array([-1] + list(range(J - 1))), vertex_label=np.zeros(V, np.int64))


def case(frames, dev, seed=1):
    """-> (body, inputs of ``refine_pose`` for ``frames`` frames, extra ids): masks and keypoints from a seeded true pose, the start 0.15
    rad off on the entries the SMPL preset moves."""
    spec = PR.RefineSpec.smpl()
    body = BM.BodyModel(device=dev, **body_arrays())
    rs = np.random.RandomState(seed)
    extra = tuple(int(i) for i in (97 * np.arange(1, 22)) % body.num_verts)
    true = (0.02 * rs.randn(frames, 72)).astype(np.float32)
    start = true.copy()
    en = np.nonzero(spec.enabled())[0]
    start[:, en] += (0.15 * np.where(rs.rand(frames, len(en)) < 0.5, -1, 1)).astype(np.float32)
    transl = np.stack([[0.02 * f, 0.01 * f, 2.6] for f in range(frames)]).astype(np.float32)
    betas = torch.zeros(10, device=dev)
    eng = PR.RefineEngine(body, betas, CAMERA, spec, extra, frames, 1, False)
    eng.transl.copy_(torch.from_numpy(transl).to(dev))
    with torch.no_grad():
        verts_cam, rows = eng._forward(torch.from_numpy(true).to(dev))
        masks = (S.soft_silhouette(verts_cam.contiguous(), body.faces, INTR, H, W, spec.sigma) > 0.5).float()
        proj = PR.project_joints(rows, INTR, H, W).cpu().numpy()
    kp = np.zeros((frames, 133, 2), np.float32)
    for coco, row in spec.keypoint_map:
        kp[:, coco] = proj[:, row]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    inputs = dict(betas=betas, global_orient=t(start[:, :3]), body_pose=t(start[:, 3:]), transl=t(transl), camera=CAMERA, masks=masks,
                  keypoints=t(kp), scores=torch.ones(frames, 133, device=dev))
    return body, spec, inputs, extra, verts_cam.contiguous()


def timed(fn, calls, reps, warmup=2):
    out = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3 / calls)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "blocks": out}


def mode_kernels(K, dev, reps):
    body, spec, inputs, extra, verts_cam = case(K, dev)
    faces_h = body.faces.cpu().numpy()
    pairs, lengths = S.pair_counts_host(verts_cam.cpu().numpy(), faces_h, INTR, H, W, spec.sigma)
    capacity = 2 * int(pairs.sum())
    plan = S.workspace_plan(K, body.num_verts, len(faces_h), H, W, capacity)
    work = S.SilhouetteWorkspace(K, body.num_verts, body.faces, H, W, capacity, dev)
    out = {"pairs_per_frame_host": [int(p) for p in pairs], "tiles_in_use": int((lengths > 0).sum()), "longest_list": int(lengths.max()),
           "capacity": capacity, "workspace_bytes_plan": plan["bytes"], "workspace_bytes_allocated": int(work.ws.numel())}
    print(json.dumps(out), flush=True)
    alpha = torch.empty((K, H, W), device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    _marshal.sil_forward(verts_cam, body.faces, INTR, H, W, spec.sigma, capacity, work.ws, alpha, counts)
    over, total, per_frame = work.info()
    assert not over and [int(p) for p in per_frame] == out["pairs_per_frame_host"]
    out["max_faces_per_pixel"] = [int(c) for c in counts.cpu().numpy()]
    dalpha = (2 * (alpha - inputs["masks"]) / (H * W)).contiguous()
    dverts = torch.empty_like(verts_cam)
    fwd = lambda: _marshal.sil_forward(verts_cam, body.faces, INTR, H, W, spec.sigma, capacity, work.ws, alpha)

    def both():
        fwd()
        _marshal.sil_backward(verts_cam, body.faces, INTR, H, W, spec.sigma, capacity, work.ws, dalpha, work.row_ptr, work.corner, dverts)

    out["forward"] = timed(fwd, 50, reps)
    out["forward_backward"] = timed(both, 50, reps)
    for k in ("forward", "forward_backward"):
        out[k]["per_frame_median_ms"] = out[k]["median_ms"] / K
    assert work.guards_intact() and bool(torch.isfinite(dverts).all())
    return out


def mode_loop(K, dev, reps, capture, iterations=100):
    body, spec, inputs, extra, _ = case(K, dev)
    engine = PR.RefineEngine(body, inputs["betas"], CAMERA, spec, extra, K, iterations, capture)
    target, used = PR.keypoint_targets(inputs["keypoints"], inputs["scores"], spec)
    start = torch.cat([inputs["global_orient"], inputs["body_pose"]], 1)
    args = (start, inputs["transl"], inputs["masks"], target, used)
    t0 = time.perf_counter()
    pose, table, faces_max = engine.run_batch(*args)                # (the first batch: allocations, and the capture in graph mode)
    first = (time.perf_counter() - t0) * 1e3
    out = {"first_batch_ms": first, "pairs_at_start": engine.start_pairs, "most_pairs": engine.peak_pairs, "capacity": engine.work.capacity,
           "workspace_bytes": int(engine.work.ws.numel()), "reruns": engine.reruns, "max_faces_per_pixel": [int(c) for c in faces_max],
           "first_loss": [float(x) for x in table[0].sum(-1)], "last_loss": [float(x) for x in table[-1].sum(-1)]}
    print(json.dumps(out), flush=True)
    out["batch_of_100"] = timed(lambda: engine.run_batch(*args), 1, reps, warmup=1)
    out["batch_of_100"]["per_frame_median_ms"] = out["batch_of_100"]["median_ms"] / K
    # one iteration on its own: the state it leaves is of no interest here, only its time
    engine.load(*args)
    one = (lambda: engine.graph.replay()) if capture else engine.iterate
    out["one_iteration"] = timed(one, 50, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("kernels", "eager", "graph"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pose_refine_time.py needs the GPU"
    dev = torch.device("cuda:0")
    res = {}
    for K in a.frames:
        res[f"K{K}"] = mode_kernels(K, dev, a.reps) if a.mode == "kernels" else mode_loop(K, dev, a.reps, a.mode == "graph")
        print(a.mode, f"K = {K}", json.dumps({k: (v["median_ms"], v["min_ms"], v["max_ms"]) for k, v in res[f"K{K}"].items()
                                               if isinstance(v, dict)}), flush=True)
    whole = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            whole = json.load(fh)
    whole.update({"case": {"W": W, "H": H, "faces": 8192, "vertices": 4098, "joints": 24, "sigma": 1e-4, "reps": a.reps,
                           "device_name": torch.cuda.get_device_name(0)}, a.mode: res})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(whole, fh, indent=1)


if __name__ == "__main__":
    main()
