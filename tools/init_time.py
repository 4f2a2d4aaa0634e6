"""Times the start of a training run on the GPU box:  python tools/init_time.py [--reps N] [--steps S] [--out FILE]

On an SMPL-sized synthetic mesh (``bumpy_sphere(114, 57)`` subdivided twice with ``topology.subdivide_meshes``: 102 146 vertices,
204 288 faces, 306 432 edges):

    initial values   ``avatar_init.initial_attributes`` (csrc/sg_init.hip: a handful of launches and one host read) against the same
                     rule written with torch ops on the same GPU, WITHOUT the reference's Python loop over the vertices (its loop, a
                     scan of the edge list and several host reads per vertex, is not run: at this size it takes minutes): the two
                     smallest incident rows by ``scatter_reduce(amin)``, the scale rule, angle-weighted normals by ``index_add_``, the
                     rotation.  Both end in one host read (the error flags / a count).
    the pre-fit      ``fit_initial_attributes`` at the shipped decoder sizes (tri-plane 64^3 x 32 features x 3 scales, decoders of 96
                     inputs; human_complex.yaml:38-43), ``--steps`` steps (500: the reference's ``init_steps``): eager, replayed from
                     a HIP graph, and the torch-ops twin -- six ``mse_loss`` terms, ``torch.optim.Adam``, torch's ``ReduceLROnPlateau``
                     fed with ``loss.item()``: a host read per step, as the reference's loop has.

Every timed block starts and ends in a device synchronise and is bracketed by CUDA events; the fit contains host work per step
(``FusedAdam.advance()`` / the twin's host read), so the events measure the wall time of the block as the device sees it.  Warm-up
first, medians over ``--reps`` (>= 5) runs and their spread.  Every fit starts from the same initial parameters.  Writes
profiles/init_time.json (``--out``)."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402

from mesh_case import bumpy_sphere                                # noqa: E402
from sings_amd import avatar_init, topology                       # noqa: E402
from sings_amd.decode import AppearanceDecoder, GeometryDecoder, HexPlaneField      # noqa: E402

LRS = {"xyz": 0.00016 * 2.0, "triplane": 1e-3, "geometry": 1e-3, "appearance": 1e-3}      # cfg.human.lr


def torch_initial_values(verts, faces, edges, mult=0.8, thickness=1.0):
    """The rule of ``initial_attributes`` with torch ops (fp32), no loop over the vertices."""
    V, E = verts.shape[0], edges.shape[0]
    e = edges.long()
    rows = torch.arange(E, device=verts.device).repeat_interleave(2)
    big = torch.full((V,), E, dtype=torch.int64, device=verts.device)
    first = big.scatter_reduce(0, e.reshape(-1), rows, "amin")
    later = torch.where(rows == first[e.reshape(-1)], torch.full_like(rows, E), rows)
    second = big.scatter_reduce(0, e.reshape(-1), later, "amin")
    lonely = int((second == E).sum())                             # the one host read
    e0, e1 = e[first], e[second]
    length = mult * torch.maximum(torch.norm(verts[e0[:, 0]] - verts[e1[:, 0]], dim=-1), torch.norm(verts[e0[:, 1]] - verts[e1[:, 1]], dim=-1))
    scales = torch.log(length).unsqueeze(1).repeat(1, 3)
    scales[:, 2] *= thickness
    scales = torch.exp(scales)
    aux = torch.log(torch.exp(scales) - 1)
    f = faces.long()
    tri = verts[f]
    fn = torch.nn.functional.normalize(torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1), dim=-1)
    acc = torch.zeros_like(verts)
    for k in range(3):
        u = torch.nn.functional.normalize(tri[:, (k + 1) % 3] - tri[:, k], dim=-1)
        w = torch.nn.functional.normalize(tri[:, (k + 2) % 3] - tri[:, k], dim=-1)
        acc.index_add_(0, f[:, k], fn * torch.acos(torch.clamp((u * w).sum(-1), -1, 1)).unsqueeze(1))
    n = torch.nn.functional.normalize(acc, dim=-1)
    fac = 1.0 / (1.0 + n[:, 2])
    R = torch.stack([1 - fac * n[:, 0] ** 2, -fac * n[:, 0] * n[:, 1], n[:, 0], -fac * n[:, 0] * n[:, 1], 1 - fac * n[:, 1] ** 2, n[:, 1],
                     -n[:, 0], -n[:, 1], 1 - fac * (n[:, 0] ** 2 + n[:, 1] ** 2)], 1)
    return {"scales": scales, "scales_aux": aux, "normals": n, "rot6d_canon": R[:, :6].clone(), "lonely": lonely}


def torch_fit(module, targets, steps, patience=100, factor=0.5):
    groups = [{"params": [module.xyz], "lr": LRS["xyz"]}, {"params": list(module.triplane.parameters()), "lr": LRS["triplane"]},
              {"params": list(module.geometry_dec.parameters()), "lr": LRS["geometry"]},
              {"params": list(module.appearance_dec.parameters()), "lr": LRS["appearance"]}]
    opt = torch.optim.Adam(groups, betas=(0.9, 0.999), eps=1e-15)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=patience, factor=factor)
    last = None
    for _ in range(steps):
        out = module.decode()
        loss = sum(torch.nn.functional.mse_loss(out[k], targets[k]) for k in avatar_init.ATTR_KEYS if out.get(k) is not None)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        last = loss.item()                                        # the host read per step
        sch.step(last)
    opt.zero_grad(set_to_none=True)
    return last


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--nu", type=int, default=114)
    ap.add_argument("--nv", type=int, default=57)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "init_time.py needs the GPU"
    dev = torch.device("cuda:0")
    v, f, _ = bumpy_sphere(a.nu, a.nv)
    verts, faces = torch.from_numpy(v * np.float32(0.9)).to(dev), torch.from_numpy(f).to(dev)
    while verts.shape[0] < 100000:
        verts, faces, _ = topology.subdivide_meshes(verts, faces, None, {})
    V = int(verts.shape[0])
    mesh = topology.MeshState.from_faces(faces, torch.zeros(V, dtype=torch.int32, device=dev))
    out = {"vertices": V, "faces": int(mesh.faces.shape[0]), "edges": int(mesh.edges.shape[0]), "steps": a.steps, "reps": a.reps,
           "device_name": torch.cuda.get_device_name(0)}

    # ---- initial values: the two agree (fp32 torch against the kernels' rounded fp64) and every shape is warm
    ours = avatar_init.initial_attributes(verts, mesh.faces, mesh.edges)
    theirs = torch_initial_values(verts, mesh.faces, mesh.edges)
    near = (1.0 + ours["normals"][:, 2]) >= 0.05
    for k in ("scales", "scales_aux", "normals", "rot6d_canon"):
        rows = near if k == "rot6d_canon" else torch.ones_like(near)
        out[f"max_abs_difference_{k}"] = float((ours[k][rows] - theirs[k][rows]).abs().max())
    init = {"device": lambda: avatar_init.initial_attributes(verts, mesh.faces, mesh.edges),
            "torch": lambda: torch_initial_values(verts, mesh.faces, mesh.edges)}
    for name, fn in init.items():
        ms = [timed(fn)[0] for _ in range(a.reps + 2)][2:]
        out[f"initial_values_ms_{name}"] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}
    out["initial_values_torch_over_device"] = out["initial_values_ms_torch"]["median"] / out["initial_values_ms_device"]["median"]

    # ---- the pre-fit at the shipped decoder sizes
    torch.manual_seed(0)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 3, 'output_coordinate_dim': 32, 'resolution': [64, 64, 64], 'multires': [1, 2, 4]}
    tri = HexPlaneField(cfg, bounds=1.2, device=dev); geo = GeometryDecoder(96).to(dev); app = AppearanceDecoder(96).to(dev)
    w = torch.full((V, 1), 1.0, dtype=torch.float32, device=dev)
    module = avatar_init.AvatarStep(verts, w, tri, geo, app, scaling_multiplier=torch.ones((V, 1), dtype=torch.float32, device=dev)).to(dev)
    start = copy.deepcopy(module.state_dict())

    def fresh():
        module.load_state_dict(start)
        return module

    fits = {"eager": lambda: avatar_init.fit_initial_attributes(fresh(), ours, LRS, init_steps=a.steps, use_graph=False)["losses"][-1, -1],
            "graph": lambda: avatar_init.fit_initial_attributes(fresh(), ours, LRS, init_steps=a.steps, use_graph=True)["losses"][-1, -1],
            "torch": lambda: torch_fit(fresh(), ours, a.steps)}
    for name, fn in fits.items():
        runs = [timed(fn) for _ in range(a.reps + 1)][1:]
        ms = [r[0] for r in runs]
        out[f"fit_ms_{name}"] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms,
                                 "per_step_ms": statistics.median(ms) / a.steps, "last_loss": float(runs[-1][1])}
    out["fit_torch_over_graph"] = out["fit_ms_torch"]["median"] / out["fit_ms_graph"]["median"]
    out["fit_eager_over_graph"] = out["fit_ms_eager"]["median"] / out["fit_ms_graph"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
