"""Times the body model on the GPU box:  python tools/body_time.py [--reps N] [--out FILE]

There is no SMPL file here (the model is licensed): the mesh is a closed synthetic one of the same order -- an octahedron subdivided
five times onto a slightly bumpy sphere, 4 098 vertices, taken two more levels by the code under test to 65 538 -- with J = 52 joints and
B = 10 betas of seeded attributes (``oracle.lbs_oracle.synthetic_body_model``'s recipe).  Three things, each against what stands for the
reference, taking turns in blocks:

    subdivided(2)        ``BodyModel.subdivided(2)`` (csrc/sg_mesh.hip + sg_body.hip: subdivision, regressor, filter, all on the device)
                         against a twin of the same definition from torch ops on the same GPU for the subdivision and numpy + scipy.sparse
                         on the host for the filter (what trimesh does it with; trimesh itself is not installed here)
    joints_rest(betas)   the [3J, B] product on the cached basis against what the reference's forward does per call for its joints:
                         ``blend_shapes`` + ``vertices2joints`` in torch ops on the same GPU, over all 65 538 vertices
    canonical(betas)     the whole canonical-pose mesh; nothing to compare it with (the reference needs smplx for it): its time alone

A call ends in a device synchronise and is timed with the host clock (the paths contain host reads).  Medians over ``--reps`` (>= 5)
blocks with their spread; a difference counts as resolved when the medians differ by more than the larger spread.  Outputs are compared
first.  Writes profiles/body_time.json (``--out``)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402
import scipy.sparse as sp                                         # noqa: E402
import torch                                                      # noqa: E402

from sings_amd import body_model as BM                            # noqa: E402

OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)


def base_mesh(levels=5):
    v, f = OCTA_V, OCTA_F
    for _ in range(levels):
        v, f, _, _ = BM.subdivide_host(v, f, {})
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    bump = 1 + 0.05 * np.sin(5 * v[:, 0]) * np.cos(4 * v[:, 1]) + 0.03 * np.sin(7 * v[:, 2])
    return (v * bump[:, None] * np.array([0.3, 0.9, 0.2])).astype(np.float32), f


def model_arrays(V, J=52, B=10, seed=0):
    rs = np.random.RandomState(seed)
    Jr = rs.rand(J, V).astype(np.float32) ** 8
    w = rs.rand(V, J).astype(np.float32) ** 6
    w[w < 0.05] = 0
    w[np.arange(V), rs.randint(0, J, V)] += 0.5
    return dict(shapedirs=rs.normal(0, 0.01, (V, 3, B)).astype(np.float32), J_regressor=Jr / Jr.sum(1, keepdims=True),
                lbs_weights=(w / w.sum(1, keepdims=True)).astype(np.float32),
                parents=np.array([-1] + [int(rs.randint(0, i)) for i in range(1, J)]), vertex_label=rs.randint(0, 15, V))


def scipy_filter(verts, faces, edges, lamb=0.5, iterations=5):
    """``smooth_host``'s definition with the operators a host mesh library builds it from: a sparse umbrella matrix, bincounts."""
    x = verts.astype(np.float64)
    V = len(x)
    src, dst = np.concatenate([edges[:, 0], edges[:, 1]]), np.concatenate([edges[:, 1], edges[:, 0]])
    L = sp.coo_matrix((np.ones(len(src)), (src, dst)), shape=(V, V)).tocsr()
    L = sp.diags(1.0 / np.asarray(L.sum(axis=1)).ravel()) @ L
    vol = lambda x: (x[faces[:, 0]] * np.cross(x[faces[:, 1]], x[faces[:, 2]])).sum() / 6
    fn = np.cross(x[faces[:, 1]] - x[faces[:, 0]], x[faces[:, 2]] - x[faces[:, 0]])
    nn = np.linalg.norm(fn, axis=1)
    unit = fn / nn[:, None]
    n = np.stack([sum(np.bincount(faces[:, k], unit[:, d], V) for k in range(3)) for d in range(3)], 1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    eps, vol0, slope = 0.01 * np.sqrt(0.5 * nn.max()), vol(x), 0.0
    for i in range(iterations):
        Lx = L @ x
        a = 1.0 / np.maximum(1e-12, np.abs((n * (x - Lx)).sum(1)))
        x = x + np.maximum(0.2 * lamb, np.minimum(1.0, lamb * a / a.mean()))[:, None] * (Lx - x)
        if i == 0:
            slope = eps / (vol(x + eps * n) - vol(x))
        x = x + n * (slope * (vol0 - vol(x)))
    return x


def torch_subdivided(m, n):
    """The loop of smpl_layer.py:306-351 from torch ops on the GPU, the filter on the host -> (v_template, J_regressor)."""
    v, f, Jr, w, sd, lab = m.v_template, m.faces.long(), m.J_regressor, m.lbs_weights, m.shapedirs, m.vertex_label
    for _ in range(n):
        e = torch.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
        rows, inv = torch.unique(e, dim=0, return_inverse=True)
        mid = inv.reshape(-1, 3) + v.shape[0]
        f = torch.stack([f[:, 0], mid[:, 0], mid[:, 2], mid[:, 0], f[:, 1], mid[:, 1], mid[:, 2], mid[:, 1], f[:, 2], mid[:, 0], mid[:, 1],
                         mid[:, 2]], 1).reshape(-1, 3)
        mean = lambda a: torch.cat([a, a[rows].mean(1)])
        v, w, sd, Jt = mean(v), mean(w), mean(sd.reshape(sd.shape[0], -1)), mean(Jr.t())
        lab = torch.cat([lab, lab[rows[:, 0]]])
        Jr = Jt.t() / Jt.t().sum(dim=1, keepdim=True)
        fh = f.cpu().numpy()
        eh = torch.unique(torch.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0], dim=0).cpu().numpy()
        v = torch.from_numpy(scipy_filter(v.cpu().numpy(), fh, eh).astype(np.float32)).to(v.device)
    return v, Jr


def verdict(a, b):
    """a against b (per-call ms of alternating blocks): resolved when the medians differ by more than the larger spread."""
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = statistics.median(b) - statistics.median(a)
    return {"difference_ms": diff, "spread_ms": spread, "resolved": abs(diff) > spread}


def blocks(fns, calls, reps, warmup=2):
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            if r >= warmup:
                out[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_time.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    assert torch.cuda.is_available(), "body_time.py needs the GPU"
    dev = torch.device("cuda:0")
    v, f = base_mesh()
    J, B = 52, 10
    base = BM.BodyModel(v_template=v, faces=f, device=dev, **model_arrays(len(v), J, B))
    fine = base.subdivided(2)
    out = {"vertices": base.num_verts, "vertices_after": fine.num_verts, "faces_after": int(fine.faces.shape[0]), "J": J, "B": B,
           "reps": a.reps, "device_name": torch.cuda.get_device_name(0), "mesh": "synthetic (no SMPL file here)"}
    # ---- the outputs agree first
    tv, tJ = torch_subdivided(base, 2)
    out["subdivided_max_abs_diff_verts"] = float((tv - fine.v_template).abs().max())
    out["subdivided_max_abs_diff_regressor"] = float((tJ - fine.J_regressor).abs().max())
    # What the difference of the vertices has to be read against: the filter's own response to one fp32 ulp.  At this resolution
    # a = 1 / max(1e-12, d) spans many decades and mean(a) hangs on the few vertices whose d nearly cancels, so lambda of EVERY vertex
    # answers to the last bits of a few; two fp64 evaluations with different summation orders differ after the first level's fp32
    # rounding by an ulp in some coordinates, and the second level sees that as this perturbation.
    mid = base.subdivided(1)
    x = BM.smooth_filter(mid.v_template, mid.faces, mid.edges)
    bumped = mid.v_template.clone()
    rows = torch.from_numpy(np.random.RandomState(0).randint(0, mid.num_verts, 50)).to(dev)
    bumped[rows, 0] = torch.nextafter(bumped[rows, 0], torch.full_like(bumped[rows, 0], 2.0))
    out["filter_response_to_one_ulp_in_50_coordinates"] = float((BM.smooth_filter(bumped, mid.faces, mid.edges) - x).abs().max())
    out["filter_largest_move"] = float((x - mid.v_template).abs().max())
    # and the device against the fp64 numpy twin on the SAME input, one level at a time (16 386 and 65 538 vertices): fp64 against fp64
    for name, parent in (("16k", base), ("65k", mid)):
        raw = parent.subdivided(1, smooth=False)
        got = BM.smooth_filter(raw.v_template, raw.faces, raw.edges).cpu().numpy().astype(np.float64)
        want = BM.smooth_host(raw.v_template.cpu().numpy(), raw.faces.cpu().numpy(), raw.edges.cpu().numpy())
        out[f"filter_device_vs_fp64_twin_{name}"] = float(np.abs(got - want).max())
    print(json.dumps({k: v for k, v in out.items() if k.startswith(("subdivided_max", "filter_"))}), flush=True)
    assert out["subdivided_max_abs_diff_verts"] <= 0.1 * out["filter_largest_move"] and out["subdivided_max_abs_diff_regressor"] <= 1e-6
    assert max(out["filter_device_vs_fp64_twin_16k"], out["filter_device_vs_fp64_twin_65k"]) <= 1e-6      # (a guard against a gross error)
    betas = torch.from_numpy(np.random.RandomState(1).normal(0, 1, B).astype(np.float32)).to(dev)

    def reference_joints():
        v_shaped = fine.v_template + torch.einsum("l,mkl->mk", betas, fine.shapedirs)          # blend_shapes
        return torch.einsum("ik,ji->jk", v_shaped, fine.J_regressor)                             # vertices2joints

    fine.joint_basis()
    out["joints_max_abs_diff"] = float((reference_joints() - fine.joints_rest(betas)).abs().max())
    assert out["joints_max_abs_diff"] <= 1e-5
    # ---- timings
    t = blocks({"device": lambda: base.subdivided(2), "torch_scipy": lambda: torch_subdivided(base, 2)}, 2, a.reps)
    j = blocks({"basis": lambda: fine.joints_rest(betas), "reference": reference_joints}, 200, a.reps)
    fresh = BM.BodyModel(v_template=fine.v_template, shapedirs=fine.shapedirs, J_regressor=fine.J_regressor, lbs_weights=fine.lbs_weights,
                         parents=fine.parents, faces=fine.faces, vertex_label=fine.vertex_label, device=dev)

    def basis_once():
        fresh._basis = None
        fresh.joint_basis()

    k = blocks({"joint_basis": basis_once}, 20, a.reps)
    fine52 = fine                                                 # (J = 52: the 'smplh' layout of the canonical pose)
    c = blocks({"canonical": lambda: fine52.canonical(betas, "da_pose", "smplh")}, 20, a.reps)
    summary = lambda b: {"median": statistics.median(b), "min": min(b), "max": max(b), "blocks": b}
    out["subdivided_ms"] = {"device": summary(t["device"]), "torch_scipy": summary(t["torch_scipy"]),
                            "verdict": verdict(t["device"], t["torch_scipy"])}
    out["joints_rest_ms"] = {"basis": summary(j["basis"]), "reference": summary(j["reference"]), "verdict": verdict(j["basis"], j["reference"])}
    out["joint_basis_once_ms"] = summary(k["joint_basis"])
    out["canonical_ms"] = summary(c["canonical"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}))
    for key in ("subdivided_ms", "joints_rest_ms"):
        print(key, json.dumps({kk: (vv if kk == "verdict" else vv["median"]) for kk, vv in out[key].items()}))
    print("joint_basis_once_ms", out["joint_basis_once_ms"]["median"], "canonical_ms", out["canonical_ms"]["median"])


if __name__ == "__main__":
    main()
