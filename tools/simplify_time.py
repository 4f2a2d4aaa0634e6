"""Times the mesh half of the hybrid pruner on the GPU box:  python tools/simplify_time.py [--reps N] [--calls K] [--out FILE]

On an SMPL-sized synthetic mesh (``bumpy_sphere(470, 235)``: 109 982 vertices, 219 960 faces, J = 52 skinning-weight rows) one
SIMPLIFICATION'S mesh work -- ``collapse_edges`` at the reference's rate 0.5, then the unique edges of the new faces -- for a band of 5
and of 8 vertex rows selected (5 170 and 9 400 edges that two selected faces share: about half of and just under the reference's
limit of 10 000), two ways, taking turns in blocks:

    device       ``sings_amd.topology`` (csrc/sg_mesh.hip): the whole collapse loop in ONE launch of one workgroup, the map, the face
                 filter and the compaction in ordinary kernels, one host read of three counts
    torch        the reference's loop restated with torch ops on the same GPU: per collapse a length per live edge, ``argmax``, the
                 host read of the chosen row, a masked assign over all V, a relabel, a filter, ``sort`` + ``unique(dim=0)``.  Its face
                 filter is VECTORISED (the reference loops over the faces in Python, one ``torch.unique`` each, and deduplicates on the
                 host): generous to the baseline

``device_rate0`` is the device path with ``collapse_rate=0`` -- everything but the iterations -- so (device - device_rate0) / collapses
is the loop's cost per iteration.  The outputs are compared first (prune mask, faces, edges: exactly); for that run the baseline forms
the squared length ``(dx*dx + dy*dy) + dz*dz`` as the kernel does, so that equality can be demanded; the TIMED baseline calls
``torch.linalg.norm`` as the reference does.  A call ends in a device synchronise and is timed with the host clock.  The baseline is
slow: ``--calls`` applies to the device paths, the baseline runs one call per block.  Medians over ``--reps`` blocks and their spread;
writes profiles/simplify_time.json (``--out``)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                                      # noqa: E402

from mesh_case import bumpy_sphere                                # noqa: E402
from sings_amd import topology                                    # noqa: E402


def torch_edges(faces):
    return torch.unique(torch.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0], dim=0)


def band_edges(faces, nu, first_row, rows):
    """sings_hybrid.py:1203-1210 for the vertices of ``rows`` consecutive rings of the sphere"""
    V = int(faces.max()) + 1
    mask = torch.zeros(V, dtype=torch.bool, device=faces.device)
    mask[1 + first_row * nu:1 + (first_row + rows) * nu] = True
    e = torch.sort(faces[mask[faces].all(dim=1)][:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    unique, counts = torch.unique(e, dim=0, return_counts=True)
    return unique[counts == 2]


def torch_collapse(verts, attr, edges, faces, rate=0.5, exact=False):
    """geometry_ops.collapse_edges' operation, written fresh with torch ops (the face filter vectorised)."""
    V = verts.shape[0]
    cmap = torch.arange(V, device=verts.device)
    num = int(torch.unique(edges).shape[0] * rate)
    for _ in range(num):
        if edges.shape[0] == 0:
            break
        d = verts[edges[:, 0]] - verts[edges[:, 1]]
        if exact:
            lengths = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        else:
            lengths = torch.linalg.norm(d, dim=1)
        v1, v2 = edges[torch.argmax(lengths)].tolist()
        cmap[cmap == v2] = v1
        edges = torch.where(edges == v2, v1, edges)
        edges = edges[edges[:, 0] != edges[:, 1]]
        edges = torch.unique(torch.sort(edges, dim=1)[0], dim=0)
    mapped = cmap[faces]
    mapped = mapped[(mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])]
    _, inverse = torch.unique(torch.sort(mapped, dim=1)[0], dim=0, return_inverse=True)
    first = torch.full((int(inverse.max()) + 1,), mapped.shape[0], device=faces.device, dtype=torch.int64)
    first.scatter_reduce_(0, inverse, torch.arange(mapped.shape[0], device=faces.device), "amin")
    kept = mapped[torch.sort(first)[0]]
    used = torch.zeros(V, dtype=torch.bool, device=faces.device)
    used[kept.reshape(-1)] = True
    renumber = torch.cumsum(used, 0) - 1
    return verts[used], renumber[kept], attr[used], ~used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--nu", type=int, default=470)
    ap.add_argument("--nv", type=int, default=235)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "simplify_time.py needs the GPU"
    dev = torch.device("cuda:0")
    v, f, _ = bumpy_sphere(a.nu, a.nv)
    V, F, J = len(v), len(f), 52
    g = torch.Generator().manual_seed(0)
    w = torch.rand(V, J, generator=g) ** 6
    verts, faces, attr = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), (w / w.sum(1, keepdim=True)).to(dev)
    out = {"vertices": V, "faces": F, "J": J, "reps": a.reps, "calls_per_block": a.calls, "baseline_calls_per_block": 1,
           "max_edges": topology.collapse_max_edges(), "device_name": torch.cuda.get_device_name(0), "sizes": {}}
    for rows in (5, 8):
        sel = band_edges(faces, a.nu, a.nv // 2 - rows // 2, rows)

        def device(rate=0.5):
            nv, nf, na, prune, n = topology.collapse_edges(verts, attr, sel, faces, collapse_rate=rate, return_collapses=True)
            return nv, nf, na, prune, topology.unique_edges(nf, nv.shape[0])[0], n

        def torch_gpu(exact=False):
            nv, nf, na, prune = torch_collapse(verts, attr, sel, faces, exact=exact)
            return nv, nf, na, prune, torch_edges(nf)

        # ---- the two compute the same thing (and every shape is warm afterwards)
        ours, ref = device(), torch_gpu(exact=True)
        device(0.0)
        torch.cuda.synchronize()
        assert torch.equal(ours[3], ref[3]) and torch.equal(ours[1], ref[1]) and torch.equal(ours[4].long(), ref[4])
        assert torch.equal(ours[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(ours[2].view(torch.int32), ref[2].view(torch.int32))
        r = {"selected_edges": int(sel.shape[0]), "collapses": int(ours[5]), "pruned": int(ours[3].sum()), "new_faces": int(ours[1].shape[0]),
             "new_edges": int(ours[4].shape[0]), "outputs_equal": True}
        del ours, ref
        paths = {"device": (device, a.calls), "device_rate0": (lambda: device(0.0), a.calls), "torch": (torch_gpu, 1)}
        blocks = {k: [] for k in paths}
        for rep in range(a.reps + 1):
            for name, (fn, calls) in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                if rep >= 1:
                    blocks[name].append((time.perf_counter() - t0) * 1e3 / calls)
        for name, b in blocks.items():
            r[f"call_ms_{name}"] = {"median": statistics.median(b), "min": min(b), "max": max(b), "blocks": b}
        med = lambda k: r[f"call_ms_{k}"]["median"]
        r["loop_us_per_collapse_device"] = (med("device") - med("device_rate0")) * 1e3 / r["collapses"]
        r["loop_us_per_collapse_torch"] = med("torch") * 1e3 / r["collapses"]
        r["torch_over_device"] = med("torch") / med("device")
        out["sizes"][f"rows_{rows}"] = r
        print(f"rows {rows}: {json.dumps({k: v for k, v in r.items() if not k.startswith('call_ms')})}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
