"""Generates tests/golden/topology_golden.npz by IMPORTING the reference's own ``geometry_ops.subdivide_meshes`` (read-only at
/root/reference; the function is pure torch, ``trimesh`` -- which the module imports and this function never calls -- is a placeholder
module here).  The reference source never ships; only these vectors do.  CPU only.

    python tests/golden/gen_topology_golden.py

Per case ``<c>``: ``<c>_verts``, ``<c>_faces``, ``<c>_face_index`` (absent: every face), ``<c>_attr_<key>`` in; ``<c>_new_verts``,
``<c>_new_faces``, ``<c>_new_attr_<key>`` out.  Integer arrays are stored as int32.

    s1_all / s1_five / s1_one / s1_dup      bumpy_sphere(8, 5): 34 vertices, 64 faces; attribute rows 1, 3, 5, 24 and 55 wide, labels
    pole                                    bumpy_sphere(80, 3): a pole of valence 80 (a row of 160 edge instances), every face
    big                                     bumpy_sphere(48, 24): 1 106 vertices; the selected faces straddle vertex 1024
    again                                   s1_five's output subdivided again (T-junctions in the input)
    flip                                    s1's faces, each under a random cyclic shift and flip, five selected
    comp / comp_cap                         the composite of sings_hybrid.py:1026-1147 restated around the imported function (as
                                            gen_lbs_golden.py restates its composite): seeded statistics, scales, labels and
                                            max_radii2D in; the masks, the selected faces, the subdivision and the old rows' new
                                            scaling_multiplier out.  comp_cap: ``max_n_gs`` bites (distinct face scores: no ties)
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))

tm = types.ModuleType("trimesh")
tm.grouping = types.ModuleType("trimesh.grouping")
tm.geometry = types.ModuleType("trimesh.geometry")
tm.geometry.faces_to_edges = None
sys.modules.update({"trimesh": tm, "trimesh.grouping": tm.grouping, "trimesh.geometry": tm.geometry})
from sings.rec.utils.geometry_ops import subdivide_meshes        # noqa: E402
from mesh_case import bumpy_sphere                               # noqa: E402  (inputs only)

out = {}


def store(name, a):
    a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
    out[name] = a.astype(np.int32) if a.dtype.kind in "iu" else a


def attributes(V, lab, rs):
    w24 = rs.rand(V, 24).astype(np.float32) ** 4
    w55 = rs.rand(V, 55).astype(np.float32) ** 4
    return {"vertex_label": torch.from_numpy(lab), "vertex_id": torch.arange(V) * 3 + 1,
            "lbs_weights": torch.from_numpy(w24 / w24.sum(1, keepdims=True)), "w55": torch.from_numpy(w55 / w55.sum(1, keepdims=True)),
            "scales": torch.from_numpy(np.exp(rs.normal(-5, 0.5, V)).astype(np.float32)),
            "col1": torch.from_numpy(rs.normal(size=(V, 1)).astype(np.float32)),
            "c5": torch.from_numpy(rs.normal(size=(V, 5)).astype(np.float32))}


def case(name, verts, faces, face_index, attrs):
    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    nv, nf, na = subdivide_meshes(verts, faces, face_index, attrs)
    store(name + "_verts", verts); store(name + "_faces", faces)
    if face_index is not None:
        store(name + "_face_index", face_index)
    store(name + "_new_verts", nv); store(name + "_new_faces", nf)
    for k, v in attrs.items():
        store(f"{name}_attr_{k}", v); store(f"{name}_new_attr_{k}", na[k])
    return nv, nf, na


rs = np.random.RandomState(4321)
v1, f1, l1 = bumpy_sphere(8, 5)
a1 = attributes(len(v1), l1, rs)
five = torch.tensor([3, 17, 18, 40, 63])
case("s1_all", v1, f1, None, a1)
nv5, nf5, na5 = case("s1_five", v1, f1, five, a1)
case("s1_one", v1, f1, torch.tensor([29]), a1)
case("s1_dup", v1, f1, torch.tensor([40, 3, 3, 63, 17, 40, 18, 3]), a1)

vp, fp, lp = bumpy_sphere(80, 3)
case("pole", vp, fp, None, {"vertex_label": torch.from_numpy(lp)})

vb, fb, lb = bumpy_sphere(48, 24)
straddle = torch.from_numpy(((fb >= 1000) & (fb < 1050)).any(1).nonzero()[0])
case("big", vb, fb, straddle, {"vertex_label": torch.from_numpy(lb)})

again = torch.from_numpy(np.sort(rs.choice(len(nf5), 23, replace=False)))
case("again", nv5, nf5, again, {k: na5[k] for k in ("vertex_label", "lbs_weights", "scales")})

ff = f1.copy()
for i in range(len(ff)):
    ff[i] = np.roll(ff[i], rs.randint(3))
    if rs.rand() < 0.5:
        ff[i] = ff[i][::-1]
case("flip", v1, ff, five, {"vertex_label": torch.from_numpy(l1)})

# ---- the composite, sings_hybrid.py:1026-1147 (what does not need the network: up to the rescale of the old rows)
vc, fc, lc = bumpy_sphere(12, 8)
N = len(vc)
for name, max_n_gs in (("comp", 100000), ("comp_cap", N + 40)):
    rc = np.random.RandomState(99)
    accum = torch.from_numpy(rc.gamma(2.0, 1e-4, (N, 1)).astype(np.float32))
    denom = torch.from_numpy(rc.randint(0, 4, (N, 1)).astype(np.float32))                # zeros: 0 / 0 = NaN -> 0, x / 0 = inf
    scales_canon = torch.from_numpy(np.exp(rc.normal(-4.6, 0.4, (N, 1))).astype(np.float32)).repeat(1, 3)
    max_radii2D = torch.from_numpy(rc.gamma(2.0, 8.0, N).astype(np.float32))
    lbs_weights = attributes(N, lc, rc)["lbs_weights"]
    vertex_label = torch.from_numpy(lc).int()
    faces_c = torch.from_numpy(fc)
    xyz_canon = torch.from_numpy(vc)
    scaling_multiplier = torch.ones(N, 1)
    grad_threshold, scale_threshold, max_screen_size = 1.5e-4, 0.009, 40.0
    for k, v in (("accum", accum), ("denom", denom), ("scales_canon", scales_canon), ("max_radii2D", max_radii2D),
                 ("lbs_weights", lbs_weights), ("vertex_label", vertex_label), ("faces", faces_c), ("xyz_canon", xyz_canon)):
        store(f"{name}_{k}", v)
    out[f"{name}_params"] = np.array([grad_threshold, scale_threshold, max_screen_size, max_n_gs], np.float64)
    # :1026-1036
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    scales = scales_canon[:, :1]
    grad_cond = torch.norm(grads, dim=-1) > grad_threshold
    scale_cond = torch.max(scales, dim=1).values > scale_threshold
    mean_scales = scales.mean()
    scales_ratio = (mean_scales / scales.mean(-1)).detach()
    # :1042-1056
    selected_pts_mask = torch.where(grad_cond, True, False)
    selected_pts_mask = torch.logical_and(selected_pts_mask, scale_cond)
    if max_screen_size:
        big_points_vs = max_radii2D > max_screen_size
        selected_pts_mask = torch.logical_or(selected_pts_mask, big_points_vs)
    exclude = torch.tensor([6, 7]).long()
    non_densified = torch.isin(vertex_label, exclude)
    selected_pts_mask = torch.logical_and(selected_pts_mask, ~non_densified)
    # :1060-1087
    selected_pts_idx = selected_pts_mask.nonzero(as_tuple=False).view(-1)
    selected_faces = torch.isin(faces_c, selected_pts_idx).any(dim=1)
    selected_faces_idx = selected_faces.nonzero(as_tuple=False).view(-1)
    e = faces_c[selected_faces_idx][:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2)
    e = torch.sort(e, dim=1)[0]
    ue, counts = torch.unique(e, dim=0, return_counts=True)
    num_to_add = counts.shape[0]
    num_left = max_n_gs - N
    capped = False
    if num_left > 0:
        if num_to_add < num_left:
            pass
        else:
            face_scores = scales[faces_c[selected_faces_idx]].sum(dim=[1, 2])
            assert len(torch.unique(face_scores)) == len(face_scores), "ties in the face scores"
            sorted_idx = torch.argsort(face_scores, descending=True)
            selected_faces_idx = selected_faces_idx[sorted_idx[:num_left // 3]]
            capped = True
    assert capped == (name == "comp_cap") and 0 < len(selected_faces_idx) < len(faces_c)
    # :1090-1101 (without "shs": interpolated and never read)
    sub_vertices, sub_faces, attr = subdivide_meshes(
        vertices=xyz_canon, faces=faces_c, face_index=selected_faces_idx,
        vertex_attributes={"vertex_label": vertex_label, "lbs_weights": lbs_weights, "scales": torch.clip(scales.mean(-1), max=0.008)})
    # :1127
    scaling_multiplier[selected_pts_mask] *= scales_ratio[selected_pts_mask].unsqueeze(1)
    store(f"{name}_selected_pts_mask", selected_pts_mask.to(torch.uint8)); store(f"{name}_selected_faces_idx", selected_faces_idx)
    store(f"{name}_sub_vertices", sub_vertices); store(f"{name}_sub_faces", sub_faces)
    store(f"{name}_new_vertex_label", attr["vertex_label"]); store(f"{name}_new_lbs_weights", attr["lbs_weights"])
    store(f"{name}_new_scales", attr["scales"]); store(f"{name}_scaling_multiplier_old", scaling_multiplier)
    # the unique edges of the new faces as the sorted unique rows (trimesh.edges_unique as a set)
    en = torch.sort(sub_faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    store(f"{name}_new_edges", torch.unique(en, dim=0))
    print(name, "N", N, "selected points", int(selected_pts_mask.sum()), "faces", len(selected_faces_idx), "new vertices",
          len(sub_vertices) - N)

dst = os.path.join(ROOT, "tests", "golden", "topology_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst) // 1024, "KiB")
