"""Generates tests/golden/avatar_init_golden.npz: the initial values of ``SinGS.initialize`` (sings_hybrid.py:674-741) on two meshes of
tests/mesh_case.py.  IMPORTS the reference's own ``torch_rotation_matrix_from_vectors``, ``matrix_to_rotation_6d`` and
``matrix_to_quaternion`` (read-only at /root/reference, utils/geometry/rotations.py: pure torch, no third-party module to stand in
for) and restates around them, in this file's own words, the scale rule of :687-702 and trimesh's angle-weighted vertex normals.  The
reference source never ships; only these vectors do.  CPU only.

    python tests/golden/gen_avatar_init_golden.py

    s24      bumpy_sphere(24, 16): 362 vertices (no multiple of 64), 720 faces, 1 080 edges; thickness_factor 1.0
    pole     bumpy_sphere(80, 3): poles of valence 80, the widest accumulation; thickness_factor 0.75 (a factor on the LOGARITHM)

Per case ``<c>``: the inputs ``<c>_verts`` (fp32), ``<c>_faces``, ``<c>_edges`` (int32: the unique sorted rows a < b, lexicographic),
``<c>_params`` (init_scale_multiplier, thickness_factor, init_opacity); the integer outputs ``<c>_first`` / ``<c>_second`` (the first two
rows of the edge list that contain each vertex); every float output twice, ``<c>_<name>_f32`` from fp32 torch arithmetic as the
reference runs it and ``<c>_<name>_f64`` from the same expressions in fp64 (name: scales, scales_aux, normals, rotmat, rot6d_canon,
rotq); ``<c>_bound_<name>``: the largest |f32 - f64| of the array -- a test of another fp32 implementation allows FOUR times that (it
carries a few roundings the reference's does not, in another order); ``<c>_rot_mask``: the vertices the rotation outputs are
compared on, ``1 + c >= 0.05`` with c the fp64 normal's z (near -z no fp32 evaluation of the rotation means anything), and the
bounds of rotmat / rot6d_canon / rotq are taken over those rows only.

Asserted here: at most 10 % of a mesh's vertices are left out (s24: the pole and the 12 vertices of the last ring whose bumpy normal
stays that close to -z, 13 of 362); everything compared is finite; on the compared rows the two largest of matrix_to_quaternion's
four candidates' denominators differ by more than 1e-4, a hundred times their fp32 rounding (the candidates agree only up to a
sign: no implementation picks another one within rounding).
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sings.rec.utils.geometry.rotations import (matrix_to_quaternion, matrix_to_rotation_6d,          # noqa: E402
                                                torch_rotation_matrix_from_vectors)
from mesh_case import bumpy_sphere                               # noqa: E402  (inputs only)

out = {}


def unique_edges(faces):
    e = np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    return np.unique(e, axis=0)                                  # lexicographic


def scale_rule(verts, edges, mult, thickness):
    """sings_hybrid.py:687-702 in the dtype of ``verts``: per vertex the rows of the edge list that contain it (:689); rows [0] and [1]
    of THOSE -- two rows (a0, b0), (a1, b1), not the endpoints of one edge (:691); the norms of x[a0] - x[a1] and x[b0] - x[b1] (:690-693)
    times the multiplier (:694); the log of the larger for all three components (:696); the last times the thickness factor (:699);
    exp (:701); log(exp(.) - 1) (:702)."""
    V = verts.shape[0]
    scales = torch.zeros_like(verts)
    first, second = np.zeros(V, np.int32), np.zeros(V, np.int32)
    for v in range(V):
        rows = torch.nonzero(torch.any(edges == v, dim=-1)).reshape(-1)
        assert rows.numel() >= 2
        first[v], second[v] = int(rows[0]), int(rows[1])
        lens = torch.norm(verts[edges[rows[0]]] - verts[edges[rows[1]]], dim=-1)
        lens = lens * mult
        scales[v] = torch.log(torch.max(lens))
    scales[..., 2] *= thickness
    scales = torch.exp(scales)
    return scales, torch.log(torch.exp(scales) - 1), first, second


def vertex_normals(verts, faces):
    """trimesh's default for a mesh without stored normals: the normalised sum over a vertex' faces of the unit face normal weighted by
    the corner angle at the vertex (angle = arccos of the clipped dot product of the two unit edge vectors), in the dtype of ``verts``."""
    tri = verts[faces]                                           # [F,3,3]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn = fn / np.linalg.norm(fn, axis=1, keepdims=True)
    acc = np.zeros_like(verts)
    for k in range(3):
        u, w = tri[:, (k + 1) % 3] - tri[:, k], tri[:, (k + 2) % 3] - tri[:, k]
        u = u / np.linalg.norm(u, axis=1, keepdims=True)
        w = w / np.linalg.norm(w, axis=1, keepdims=True)
        angle = np.arccos(np.clip((u * w).sum(1), -1, 1)).astype(verts.dtype)
        np.add.at(acc, faces[:, k], fn * angle[:, None])
    return (acc / np.linalg.norm(acc, axis=1, keepdims=True)).astype(verts.dtype)


def evaluate(verts, faces, edges, mult, thickness, dtype):
    v = torch.from_numpy(verts.astype(dtype))
    # torch multiplies an fp32 tensor by a Python scalar in fp32: the fp64 evaluation uses the same two fp32 constants
    scales, aux, first, second = scale_rule(v, torch.from_numpy(edges).long(), float(np.float32(mult)), float(np.float32(thickness)))
    n = torch.from_numpy(vertex_normals(verts.astype(dtype), faces))
    z = torch.zeros_like(n)
    z[:, 2] = 1.0                                                # gs_normals (:710-711)
    R = torch_rotation_matrix_from_vectors(z, n)                 # :713
    return {"scales": scales, "scales_aux": aux, "normals": n, "rotmat": R, "rot6d_canon": matrix_to_rotation_6d(R),
            "rotq": matrix_to_quaternion(R)}, first, second


def case(name, nu, nv, mult, thickness, init_opacity, left_out=None):
    verts, faces, _ = bumpy_sphere(nu, nv)
    edges = unique_edges(faces)
    f32, first, second = evaluate(verts, faces, edges, mult, thickness, np.float32)
    f64, first64, second64 = evaluate(verts, faces, edges, mult, thickness, np.float64)
    assert np.array_equal(first, first64) and np.array_equal(second, second64)
    V = len(verts)
    mask = (1.0 + f64["normals"][:, 2].numpy()) >= 0.05
    n_out = int((~mask).sum())
    assert n_out <= 0.1 * V, (name, n_out, V)
    assert left_out is None or n_out == left_out, (name, n_out)
    R = f64["rotmat"][mask].numpy()
    q_abs = np.sqrt(np.maximum(np.stack([1 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], 1 + R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2],
                                         1 - R[:, 0, 0] + R[:, 1, 1] - R[:, 2, 2], 1 - R[:, 0, 0] - R[:, 1, 1] + R[:, 2, 2]], 1), 0))
    top = np.sort(q_abs, axis=1)
    assert (top[:, 3] - top[:, 2]).min() > 1e-4, (name, (top[:, 3] - top[:, 2]).min())
    out[f"{name}_verts"], out[f"{name}_faces"], out[f"{name}_edges"] = verts, faces.astype(np.int32), edges.astype(np.int32)
    out[f"{name}_params"] = np.array([mult, thickness, init_opacity], np.float64)
    out[f"{name}_first"], out[f"{name}_second"], out[f"{name}_rot_mask"] = first, second, mask.astype(np.uint8)
    print(f"{name}: V {V} F {len(faces)} E {len(edges)} rotation rows left out {n_out}")
    for k in f32:
        a, b = f32[k].numpy(), f64[k].numpy()
        rows = mask if k in ("rotmat", "rot6d_canon", "rotq") else np.ones(V, bool)
        assert np.isfinite(a[rows]).all() and np.isfinite(b[rows]).all(), (name, k)
        bound = float(np.abs(a[rows].astype(np.float64) - b[rows]).max())
        assert bound > 0.0
        out[f"{name}_{k}_f32"], out[f"{name}_{k}_f64"], out[f"{name}_bound_{k}"] = a, b, np.float64(bound)
        print(f"    {k:<12} bound {bound:.3e}  (largest |value| {np.abs(b[rows]).max():.3g})")


case("s24", 24, 16, 0.8, 1.0, 0.8, left_out=13)
case("pole", 80, 3, 0.8, 0.75, 0.83)
dst = os.path.join(ROOT, "tests", "golden", "avatar_init_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst) // 1024, "KiB")
