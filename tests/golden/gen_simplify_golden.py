"""Generates tests/golden/simplify_golden.npz by IMPORTING the reference's own ``geometry_ops.collapse_edges`` (read-only at
/root/reference; pure torch but for ``trimesh.grouping.unique_rows``, for which a placeholder module carries a stand-in: the
first-occurrence indices of ``numpy.unique(axis=0, return_index=True)`` -- only the face SET is compared, so the stand-in's row order
does not matter).  The reference source never ships; only these vectors do.  CPU only.

    python tests/golden/gen_simplify_golden.py

Per case ``<c>``: ``<c>_verts``, ``<c>_faces``, ``<c>_sel`` (the selected edges), ``<c>_rate``, ``<c>_attr`` in; ``<c>_prune_mask``,
``<c>_new_faces`` (the reference's rows, in ITS order), ``<c>_new_faces_ordered`` (the same set of rows in the ORIGINAL order of the
faces they come from, from the restatement below), ``<c>_collapses``, ``<c>_margin``, ``<c>_depth`` out.  Integer arrays are int32.

    s1_all        bumpy_sphere(8, 5), every vertex selected: 96 edges, 17 collapses, degenerate and duplicate faces
    s1_all_sel_shuffled   s1_all's edge rows, each twice, shuffled (the outputs are s1_all's)
    pole          bumpy_sphere(80, 3), every vertex: poles of valence 80
    half          bumpy_sphere(12, 8), the upper half (z > 0) selected: the region's boundary edges are excluded
    half_full     the same at collapse_rate 1.0: the edge list is exhausted before the count is reached
    rand60        bumpy_sphere(48, 24), a random 60 % of the vertices: long chains, isolated vertices
    big_all       bumpy_sphere(48, 24), every vertex: 3 312 edges (more than three per lane of the kernel), 553 collapses
    comp_prune / comp_skip_min / comp_skip_none / comp_skip_many
                  sings_hybrid.py:1157-1224 restated around the imported function: seeded statistics, opacity, scales and labels in;
                  the vertex mask, the selected edges, the skip rule that fired (0: none, 1: N <= min_n_gs, 2: no edge, 3: too many
                  edges) and, for comp_prune, the collapse out.  Its positions are the anchors of tests/test_gpu_subdivide_train.py.

Selected edges are what sings_hybrid.py:1203-1210 makes of a vertex mask: the unique sorted edges, shared by exactly two of them, of
the faces with ALL corners selected.

The generator also runs the loop restated as a quotient graph in fp64 (a class is its smallest vertex, which never moves) and
ASSERTS (1) that it reproduces the imported function's prune mask and face set, winding included, and (2) that at every iteration of
every case the longest and the second-longest live edge differ by at least 16 * 2^-23 relative: an fp32 length carries about four
roundings per implementation, so under this condition every correct fp32 implementation picks the reference's edges, and a test may
demand equality.  A case that fails (2) gets another ``bumpy_sphere`` seed, recorded in SEEDS -- the condition is not loosened.
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


def _unique_rows(data):
    _, index, inverse = np.unique(np.asarray(data), axis=0, return_index=True, return_inverse=True)
    return index, inverse


tm = types.ModuleType("trimesh")
tm.grouping = types.ModuleType("trimesh.grouping")
tm.grouping.unique_rows = _unique_rows
tm.geometry = types.ModuleType("trimesh.geometry")
tm.geometry.faces_to_edges = None
sys.modules.update({"trimesh": tm, "trimesh.grouping": tm.grouping, "trimesh.geometry": tm.geometry})
from sings.rec.utils.geometry_ops import collapse_edges          # noqa: E402
from mesh_case import bumpy_sphere                               # noqa: E402  (inputs only)

MARGIN = 16 * 2.0 ** -23
SEEDS = {"s1": 0, "pole": 0, "half": 0, "big": 0}                # bumpy_sphere seeds (changed only when the margin assertion asks)
out = {}


def store(name, a):
    a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
    out[name] = a.astype(np.int32) if a.dtype.kind in "iu" else a


def selected_edges(faces, vert_mask):
    """sings_hybrid.py:1203-1210"""
    faces = torch.as_tensor(faces)
    idx = torch.where(torch.as_tensor(vert_mask))[0]
    face_mask = torch.isin(faces, idx).all(dim=1)
    e = torch.sort(faces[face_mask][:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1)[0]
    unique, counts = torch.unique(e, dim=0, return_counts=True)
    return unique[counts == 2]


def quotient(verts, sel, faces, rate):
    """The loop as a quotient graph, lengths in fp64 from the INPUT positions -> (prune_mask, new_faces in original order, collapses,
    smallest relative gap between the two longest live edges, deepest chain of the map)."""
    V, P = len(verts), np.asarray(verts, np.float64)
    live = set(map(tuple, np.asarray(sel).tolist()))
    num = int(len(np.unique(np.asarray(sel))) * rate)
    parent, done, margin = np.arange(V), 0, np.inf
    for _ in range(num):
        if not live:
            break
        E = np.array(sorted(live))
        L = np.linalg.norm(P[E[:, 0]] - P[E[:, 1]], axis=1)
        order = np.lexsort((E[:, 1], E[:, 0], -L))
        if len(E) > 1:
            margin = min(margin, (L[order[0]] - L[order[1]]) / L[order[0]])
        v1, v2 = (int(x) for x in E[order[0]])
        parent[v2] = v1
        done += 1
        new = set()
        for a, b in live:
            a, b = (v1 if a == v2 else a), (v1 if b == v2 else b)
            if a != b:
                new.add((min(a, b), max(a, b)))
        live = new
    cmap, depth = np.arange(V), 0
    for v in range(V):
        p, d = v, 0
        while parent[p] != p:
            p, d = parent[p], d + 1
        cmap[v], depth = p, max(depth, d)
    mapped = cmap[np.asarray(faces)]
    seen, keep = set(), []
    for f, row in enumerate(mapped.tolist()):
        key = tuple(sorted(row))
        if len(set(row)) == 3 and key not in seen:
            seen.add(key)
            keep.append(f)
    kept = mapped[keep]
    used = np.zeros(V, bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    return ~used, renumber[kept], done, margin, depth


def by_vertex_set(faces):
    """rows ordered by their sorted-corner triple (no two kept faces share one)"""
    faces = np.asarray(faces)
    key = np.sort(faces, axis=1)
    assert len(np.unique(key, axis=0)) == len(key)
    return faces[np.lexsort((key[:, 2], key[:, 1], key[:, 0]))]


def case(name, verts, faces, sel, rate, attr):
    verts, faces, sel = np.asarray(verts, np.float32), np.asarray(faces, np.int64), np.asarray(sel, np.int64)
    nv, nf, na, prune = collapse_edges(torch.from_numpy(verts).clone(), torch.from_numpy(attr).clone(), torch.from_numpy(sel).clone(),
                                       torch.from_numpy(faces).clone(), collapse_rate=rate)
    q_prune, q_faces, done, margin, depth = quotient(verts, sel, faces, rate)
    assert np.array_equal(prune.numpy(), q_prune), name
    assert np.array_equal(by_vertex_set(nf.numpy()), by_vertex_set(q_faces)), name
    assert np.array_equal(nv.numpy().view(np.uint32), verts[~q_prune].view(np.uint32)), name
    assert np.array_equal(na.numpy().view(np.uint32), attr[~q_prune].view(np.uint32)), name
    assert margin >= MARGIN, f"{name}: the two longest edges come within {margin:.3g} relative: take another bumpy_sphere seed"
    mapped_deg = len(faces) - len(q_faces)
    for k, v in (("verts", verts), ("faces", faces), ("sel", sel), ("attr", attr), ("prune_mask", q_prune.astype(np.uint8)),
                 ("new_faces", nf), ("new_faces_ordered", q_faces), ("rate", np.float64(rate)), ("collapses", np.int32(done)), ("margin", np.float64(margin)),
                 ("depth", np.int32(depth))):
        store(f"{name}_{k}", v)
    print(f"{name}: V {len(verts)} F {len(faces)} edges {len(sel)} collapses {done} faces dropped {mapped_deg} pruned {int(q_prune.sum())} "
          f"chain {depth} margin {margin:.3g}")
    return q_prune, q_faces, done


def attr_rows(V, rs):
    w = rs.rand(V, 5).astype(np.float32) ** 4
    return w / w.sum(1, keepdims=True)


rs = np.random.RandomState(2468)
v1, f1, _ = bumpy_sphere(8, 5, seed=SEEDS["s1"])
sel1 = selected_edges(f1, np.ones(len(v1), bool)).numpy()
_, _, n1 = case("s1_all", v1, f1, sel1, 0.5, attr_rows(len(v1), rs))
assert len(sel1) == 96 and n1 == 17
shuffled = np.concatenate([sel1, sel1])[rs.permutation(2 * len(sel1))]
store("s1_all_sel_shuffled", shuffled)

vp, fp, _ = bumpy_sphere(80, 3, seed=SEEDS["pole"])
case("pole", vp, fp, selected_edges(fp, np.ones(len(vp), bool)).numpy(), 0.5, attr_rows(len(vp), rs))

vh, fh, _ = bumpy_sphere(12, 8, seed=SEEDS["half"])
selh = selected_edges(fh, vh[:, 2] > 0).numpy()
case("half", vh, fh, selh, 0.5, attr_rows(len(vh), rs))
_, _, nh = case("half_full", vh, fh, selh, 1.0, attr_rows(len(vh), rs))
assert nh == 48 and int(len(np.unique(selh)) * 1.0) == 49             # exhausted one collapse early

vb, fb, _ = bumpy_sphere(48, 24, seed=SEEDS["big"])
case("rand60", vb, fb, selected_edges(fb, rs.rand(len(vb)) < 0.6).numpy(), 0.5, attr_rows(len(vb), rs))
selb = selected_edges(fb, np.ones(len(vb), bool)).numpy()
_, _, nb = case("big_all", vb, fb, selb, 0.5, attr_rows(len(vb), rs))
assert len(selb) == 3312 and nb == 553

# ---- the composite, sings_hybrid.py:1157-1224
vc, fc, lc = bumpy_sphere(12, 8)
xyz_canon = (vc * np.array([0.2, 0.42, 0.15])).astype(np.float32)      # the anchors of tests/test_gpu_subdivide_train.py
N = len(vc)
for name, (opacity_threshold, scale_threshold, prune_max, min_n_gs), fired in (
        ("comp_prune", (0.8, 0.0075, 5000, 40), 0), ("comp_skip_min", (0.8, 0.0075, 5000, N), 1),
        ("comp_skip_none", (0.02, 0.001, 5000, 40), 2), ("comp_skip_many", (0.8, 0.0075, 4, 40), 3)):
    rc = np.random.RandomState(77)
    accum = torch.from_numpy(rc.gamma(2.0, 4e-4, (N, 1)).astype(np.float32))
    denom = torch.from_numpy(rc.randint(0, 4, (N, 1)).astype(np.float32))                # zeros: 0 / 0 = NaN (not dead), x / 0 = inf
    accum[denom[:, 0] == 0] *= torch.from_numpy((rc.rand(int((denom == 0).sum())) < 0.5).astype(np.float32)).unsqueeze(1)
    opacity = torch.from_numpy(rc.rand(N, 1).astype(np.float32))
    scales = torch.from_numpy(np.exp(rc.normal(-4.9, 0.45, (N, 1))).astype(np.float32)).repeat(1, 3)
    vertex_label = torch.from_numpy(lc).int()
    faces_c = torch.from_numpy(fc)
    lbs_weights = torch.from_numpy(attr_rows(N, rc))
    dead_grad, large_scale = 0.0005, 0.01
    for k, v in (("accum", accum), ("denom", denom), ("opacity", opacity), ("scales", scales), ("vertex_label", vertex_label),
                 ("faces", faces_c), ("xyz_canon", xyz_canon), ("lbs_weights", lbs_weights)):
        store(f"{name}_{k}", v)
    out[f"{name}_params"] = np.array([opacity_threshold, scale_threshold, dead_grad, large_scale, prune_max, min_n_gs], np.float64)
    rule, vert_mask, sel = 0, torch.zeros(N, 1, dtype=torch.bool), torch.zeros(0, 2, dtype=torch.int64)
    if N <= min_n_gs:                                                                     # :1157
        rule = 1
    else:
        vert_mask = torch.where(opacity < opacity_threshold, True, False)                # :1172-1184
        vert_mask = torch.logical_and(vert_mask, scales[:, :1] < scale_threshold)
        grads = accum / denom
        dead_large_mask = scales[:, :1] > large_scale
        dead_large_mask = torch.logical_and(dead_large_mask, grads < dead_grad)
        vert_mask = torch.logical_or(vert_mask, dead_large_mask)
        exclude = torch.tensor([6, 7]).long()                                             # :1187-1190
        non_decimate = torch.isin(vertex_label, exclude).unsqueeze(1)
        vert_mask = torch.logical_and(vert_mask, ~non_decimate)
        if vert_mask.sum() == 0:                                                          # :1195
            rule = 2
        else:
            sel = selected_edges(faces_c, vert_mask[:, 0])                                # :1203-1210
            if sel.shape[0] == 0:                                                         # :1217-1222
                rule = 2
            elif sel.shape[0] > 2 * prune_max:
                rule = 3
    assert rule == fired, (name, rule, int(vert_mask.sum()), sel.shape)
    store(f"{name}_vert_mask", vert_mask.reshape(-1).to(torch.uint8)); store(f"{name}_selected_edges", sel.reshape(-1, 2))
    out[f"{name}_rule"] = np.int32(rule)
    print(name, "N", N, "selected points", int(vert_mask.sum()), "edges", int(sel.shape[0]), "rule", rule)
    if rule == 0:
        assert bool(torch.isnan(grads).any()) and bool((dead_large_mask & ~non_decimate).any())
        case(name + "_collapse", xyz_canon, fc, sel.numpy(), 0.5, lbs_weights.numpy())   # :1224

dst = os.path.join(ROOT, "tests", "golden", "simplify_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst) // 1024, "KiB")
