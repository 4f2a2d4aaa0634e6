"""Times the mesh half of the hybrid densifier on the GPU box:  python tools/subdivide_time.py [--reps N] [--calls K] [--out FILE]

On an SMPL-sized synthetic mesh (``bumpy_sphere(470, 235)``: 109 982 vertices, 219 960 faces; the first third of the faces selected,
J = 52 skinning-weight rows, labels, a scale per vertex) one DENSIFICATION'S mesh work -- ``subdivide_meshes`` with the three
attributes, then the unique edges of the new faces -- three ways, taking turns in blocks of ``--calls`` calls:

    device       ``sings_amd.topology`` (csrc/sg_mesh.hip): counting + scans + rank by counting, two host reads of two counts
    torch        the same operation written with torch ops on the same GPU: ``torch.unique(dim=0, return_inverse=True, return_counts=True)``
                 plus gathers, twice (the subdivision, then the new faces' edges)
    torch_host   the torch subdivision on the GPU, then what the reference pays for its edge list: vertices and faces copied to the
                 host, the unique edges found there, the edges copied back.  ``trimesh`` is not installed here: its ``edges_unique`` hashes
                 each sorted row into one integer and runs a 1-D ``numpy.unique`` over the hashes (``grouping.unique_rows``), and that is
                 what stands in for it -- without the vertex merging and the caches the ``Trimesh`` constructor also builds

A call ends in a device synchronise and is timed with the host clock (the device path contains host reads).  Outputs of the three are
compared first: indices exactly, floats bit for bit.  Medians over ``--reps`` blocks and their spread; writes profiles/subdivide_time.json
(``--out``)."""
import argparse
import json
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
from sings_amd import topology                                    # noqa: E402


def torch_subdivide(vertices, faces, face_index, attrs):
    """geometry_ops.subdivide_meshes' operation, written fresh with torch ops."""
    mask = torch.zeros(faces.shape[0], dtype=torch.bool, device=faces.device)
    mask[face_index] = True
    sub = faces[mask]
    e = torch.sort(sub[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    rows, inv = torch.unique(e, dim=0, return_inverse=True)
    mid = inv.reshape(-1, 3) + vertices.shape[0]
    kids = torch.stack([sub[:, 0], mid[:, 0], mid[:, 2], mid[:, 0], sub[:, 1], mid[:, 1], mid[:, 2], mid[:, 1], sub[:, 2],
                        mid[:, 0], mid[:, 1], mid[:, 2]], 1).reshape(-1, 3)
    new_faces = torch.cat([faces[~mask], kids])
    new_vertices = torch.cat([vertices, vertices[rows].mean(1)])
    out = {k: torch.cat([v, v[rows[:, 0]] if k == "vertex_label" else v[rows].mean(1)]) for k, v in attrs.items()}
    return new_vertices, new_faces, out


def torch_edges(faces):
    return torch.unique(torch.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0], dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--nu", type=int, default=470)
    ap.add_argument("--nv", type=int, default=235)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subdivide_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "subdivide_time.py needs the GPU"
    dev = torch.device("cuda:0")
    v, f, lab = bumpy_sphere(a.nu, a.nv)
    V, F, J = len(v), len(f), 52
    g = torch.Generator().manual_seed(0)
    w = torch.rand(V, J, generator=g) ** 6
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    attrs = {"vertex_label": torch.from_numpy(lab).to(dev), "lbs_weights": (w / w.sum(1, keepdim=True)).to(dev),
             "scales": (0.004 + 0.008 * torch.rand(V, generator=g)).to(dev)}
    face_index = torch.arange(F // 3, device=dev)

    def device():
        nv, nf, na = topology.subdivide_meshes(verts, faces, face_index, attrs)
        return nv, nf, na, topology.unique_edges(nf, nv.shape[0])[0]

    def torch_gpu():
        nv, nf, na = torch_subdivide(verts, faces, face_index, attrs)
        return nv, nf, na, torch_edges(nf)

    def torch_host():
        nv, nf, na = torch_subdivide(verts, faces, face_index, attrs)
        nv.cpu()                                                  # (trimesh.Trimesh takes the vertices too)
        fh = nf.cpu().numpy()
        e = np.sort(fh[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
        key = np.unique(e[:, 0] << 32 | e[:, 1])                  # (one integer per row: ascending keys = lexicographic rows)
        return nv, nf, na, torch.from_numpy(np.stack([key >> 32, key & 0xffffffff], 1)).to(dev)

    paths = {"device": device, "torch": torch_gpu, "torch_host": torch_host}
    # ---- the three compute the same thing (and every shape is warm afterwards)
    outs = {k: fn() for k, fn in paths.items()}
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t.long()
    ref = outs["torch"]
    for k, o in outs.items():
        assert torch.equal(bits(o[0]), bits(ref[0])) and torch.equal(o[1], ref[1]) and torch.equal(o[3].long(), ref[3]), k
        for name in attrs:
            assert torch.equal(bits(o[2][name]), bits(ref[2][name])), (k, name)
    out = {"vertices": V, "faces": F, "selected_faces": int(face_index.numel()), "new_vertices": int(ref[0].shape[0]) - V,
           "new_faces": int(ref[1].shape[0]), "new_edges": int(ref[3].shape[0]), "J": J, "reps": a.reps, "calls_per_block": a.calls,
           "device_name": torch.cuda.get_device_name(0), "outputs_equal": True}
    del outs, ref
    blocks = {k: [] for k in paths}
    for rep in range(a.reps + 2):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            if rep >= 2:
                blocks[name].append((time.perf_counter() - t0) * 1e3 / a.calls)
    for name, b in blocks.items():
        out[f"call_ms_{name}"] = {"median": statistics.median(b), "min": min(b), "max": max(b), "blocks": b}
    med = lambda k: out[f"call_ms_{k}"]["median"]
    out["torch_over_device"] = med("torch") / med("device")
    out["torch_host_over_device"] = med("torch_host") / med("device")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
