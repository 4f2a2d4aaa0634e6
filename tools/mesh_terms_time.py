"""Times the mesh terms of the training step on the GPU box:  python tools/mesh_terms_time.py [--reps N] [--calls K] [--steps S] [--out FILE]

On an SMPL-sized synthetic mesh (``bumpy_sphere(114, 57)`` subdivided twice with ``topology.subdivide_meshes``: 102 146 vertices, eight
longitude sectors as labels -- the size tools/init_time.py uses):

    the terms     ``MeshTerms.__call__`` + backward (three launches, buffers owned by the module) against the composition the tree offered
                  before: two ``RegionLaplacianLoss_v2``, ``forward_hands`` and the anchor formed with torch ops, differentiated through
                  autograd.  Blocks of ``--calls`` calls between two HIP events, the two ALTERNATING, ``--reps`` blocks each; reported:
                  the median per call and the spread (min .. max) of the blocks.  The fused call beats the composition when the
                  difference of the medians exceeds the blocks' spread; otherwise the two are NOT RESOLVED from each other.
    the build     ``MeshTerms.reset`` (device build of both CSRs + the constant edge term + one 16-byte host read) against
                  ``RegionLaplacianLoss_v2.reset_laplacians`` on the same mesh (device-to-host copy of edges and labels, numpy CSR, upload)
                  -- wall time per call, ending in a device synchronise.
    the step      ``AvatarTrainer.step`` replayed from a HIP graph (L2Norm + k-NN edge loss, deferred join, fused optimiser) on the
                  mesh's vertices as anchors, with and without ``mesh_terms``: blocks of ``--steps`` steps; the two trainers are built
                  twice each, in alternation.

Writes profiles/mesh_terms_time.json (``--out``)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from mesh_case import bumpy_sphere                                # noqa: E402
from sings_amd import avatar_init, grad_arena, overflow, topology # noqa: E402
from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField      # noqa: E402
from sings_amd.mesh_terms import MeshTerms                        # noqa: E402
from sings_amd.rasterizer import GaussianRasterizationSettings   # noqa: E402
from sings_amd.regularizers import GaussiansEdgeLoss, L2Norm, RegionLaplacianLoss_v2      # noqa: E402
from sings_amd.scene import avatar_scene                          # noqa: E402
from sings_amd.train_loop import AvatarTrainer                    # noqa: E402
from sings_amd.train_step import AvatarStep                       # noqa: E402

LRS = {"xyz": 3.2e-4, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}
W_POS = [0.5, 0.75, 1.0, 1.0, 1.0, 1.5, 1.5, 1.5]
W_COL = [0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5]
ALPHA, BETA = 1000.0, 10.0


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def block(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternating(fns, n, reps, warmup=2):
    """{name: per-call ms of each block}: the blocks of the candidates alternate, so that a drift of the box hits all of them."""
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            ms = block(fn, n)
            if r >= warmup:
                out[k].append(ms)
    return out


def verdict(a, b):
    """a against b (per-call ms of alternating blocks): resolved when the medians differ by more than the larger spread."""
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = statistics.median(b) - statistics.median(a)
    return {"difference_ms": diff, "spread_ms": spread, "resolved": abs(diff) > spread}


def build_trainer(dev, verts, mesh, with_terms):
    V = int(verts.shape[0])
    s = avatar_scene(N=V, J=52)
    W, H = s["W"], s["H"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cam = s["cam"]
    consts = dict(bg=t(s["bg"]), view=t(cam["world_view_transform"]), proj=t(cam["full_proj_transform"]), campos=t(cam["camera_center"]))

    def settings(deg):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), bg=consts["bg"],
            scale_modifier=1.0, viewmatrix=consts["view"], projmatrix=consts["proj"], sh_degree=deg, campos=consts["campos"],
            prefiltered=False, debug=False)
    torch.manual_seed(0)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [64, 64, 64], 'multires': [1, 2, 4]}
    tri = HexPlaneField(cfg, bounds=1.2, device=dev, feature_minor=True)
    geo = GeometryDecoder(96).to(dev); app = AppearanceDecoder(96).to(dev)
    with torch.no_grad():
        geo.scales[2].bias.fill_(-5.3); geo.scales[2].weight.mul_(0.1)
        geo.xyz_offsets.weight.mul_(0.01); geo.xyz_offsets.bias.zero_()
    mod = AvatarStep(verts, t(s["lbs_weights"]), tri, geo, app, l2_norm=L2Norm(), gaussian_connect=GaussiansEdgeLoss(),
                     gaussian_connect_w=1.0, defer_regulariser_join=True).to(dev)
    A = torch.eye(4, device=dev).repeat(52, 1, 1).contiguous()
    gt = torch.rand((3, H, W), device=dev)
    mask = torch.ones((H, W), device=dev)
    terms = MeshTerms(W_POS, W_COL, 1.0, ALPHA, BETA, 1) if with_terms else None
    tr = AvatarTrainer(mod, settings, consts["bg"], LRS, smpl_scale=t(s["smpl_scale"]), transl=t(s["transl"]), use_graph=True,
                       sh_degree=0, max_sh_degree=0, optimizer="fused", mesh=mesh, mesh_terms=terms)
    tr.iteration = 10                                             # past the ramp: alpha at full strength
    return tr, A, gt, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nu", type=int, default=114)
    ap.add_argument("--nv", type=int, default=57)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_terms_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "mesh_terms_time.py needs the GPU"
    dev = torch.device("cuda:0")
    v, f, lab = bumpy_sphere(a.nu, a.nv)
    verts = torch.from_numpy(v * np.array([0.28, 0.85, 0.16], np.float32)).to(dev)
    faces, labels = torch.from_numpy(f).to(dev), torch.from_numpy(lab).to(dev, torch.int32)
    while verts.shape[0] < 100000:
        verts, faces, attr = topology.subdivide_meshes(verts, faces, None, {"vertex_label": labels})
        labels = attr["vertex_label"]
    V = int(verts.shape[0])
    mesh = topology.MeshState.from_faces(faces, labels)
    normals = avatar_init.initial_attributes(verts, mesh.faces, mesh.edges)["normals"]
    out = {"vertices": V, "faces": int(mesh.faces.shape[0]), "edges": int(mesh.edges.shape[0]), "reps": a.reps, "calls_per_block": a.calls,
           "steps_per_block": a.steps, "device_name": torch.cuda.get_device_name(0)}

    # ---- the terms: fused against the stand-alone composition
    g = torch.Generator().manual_seed(0)
    xyz = (verts + 0.002 * torch.randn(V, 3, generator=g).to(dev)).requires_grad_(True)
    scales = torch.exp(torch.randn(V, 3, generator=g) * 0.3 - 4.9).to(dev).requires_grad_(True)
    shs = torch.rand(V, 16, 3, generator=g).to(dev).requires_grad_(True)
    mt = MeshTerms(W_POS, W_COL, 1.0, ALPHA, BETA, 1)
    mt.reset(mesh, normals, verts)
    mt.set_iteration(10)
    out["same_label_entries"] = mt.nnz
    pos = RegionLaplacianLoss_v2(verts=verts, edges=mesh.edges, vertex_labels=mesh.vertex_label, region_weights=W_POS)
    col = RegionLaplacianLoss_v2(verts=verts, edges=mesh.edges, vertex_labels=mesh.vertex_label, region_weights=W_COL)
    leaves = [xyz, scales, shs]

    def fused():
        o = mt({"xyz_canon": xyz, "scales": scales, "shs": shs})
        return torch.autograd.grad(o["region_mesh_lap"] + o["region_mesh_lap_color"] + o["hand_lap"], leaves)

    def fused_kernels_only():                                     # as the deferred step uses it: values and last_grads, no autograd
        with torch.enable_grad():
            mt({"xyz_canon": xyz.detach(), "scales": scales.detach(), "shs": shs.detach()})

    def standalone():
        anchor = xyz + scales.mean(dim=-1, keepdim=True) * normals / 2.0
        loss = ALPHA * pos(anchor) + BETA * col(shs[:, 0].contiguous()) + 1e-5 * pos.forward_hands(xyz)
        return torch.autograd.grad(loss, leaves)

    ga, gb = fused(), standalone()
    out["max_rel_difference_of_gradients"] = [float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(ga, gb)]
    t = alternating({"fused": fused, "fused_kernels_only": fused_kernels_only, "standalone": standalone}, a.calls, a.reps)
    out["terms_ms"] = {k: stats(x) for k, x in t.items()}
    out["terms_fused_against_standalone"] = verdict(t["fused"], t["standalone"])
    out["terms_kernels_only_against_standalone"] = verdict(t["fused_kernels_only"], t["standalone"])

    # ---- the build: device against host
    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    builds = {"device_reset": lambda: mt.reset(mesh, normals, verts),
              "host_reset_laplacians": lambda: pos.reset_laplacians(verts, mesh.edges, mesh.vertex_label)}
    for r in range(a.reps + 2):
        for k, fn in builds.items():
            ms = wall(fn)
            if r >= 2:
                out.setdefault("build_ms", {}).setdefault(k, []).append(ms)
    out["build_ms"] = {k: stats(x) for k, x in out["build_ms"].items()}
    out["build_host_over_device"] = out["build_ms"]["host_reset_laplacians"]["median"] / out["build_ms"]["device_reset"]["median"]

    # ---- the captured step with and without the terms: one trainer at a time (they share the module-level gradient arena), built twice
    #      each in alternation; every block is `--steps` replayed steps
    if not a.skip_step:
        steps = {"without": [], "with_mesh_terms": []}
        try:
            for _ in range(2):
                for k in steps:
                    tr, A, gt, mask = build_trainer(dev, verts, mesh, k == "with_mesh_terms")
                    for _ in range(6):                            # sizing steps, the capture, two replays
                        tr.step(A, gt, mask)
                    assert tr.captured is not None
                    steps[k] += [block(lambda: tr.step(A, gt, mask), a.steps) for _ in range(a.reps)]
                    del tr
                    overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
                    grad_arena.set_gradient_arena(None, None)
            out["captured_step_ms"] = {k: stats(x) for k, x in steps.items()}
            out["captured_step_terms_cost"] = verdict(steps["without"], steps["with_mesh_terms"])
        finally:
            overflow.set_overflow_check("sync"); overflow.reset_overflow_state()
            grad_arena.set_gradient_arena(None, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
