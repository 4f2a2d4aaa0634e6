"""Generates tests/golden/body_golden.npz by IMPORTING the reference's own Python (a checkout beside this repository, or where
``SINGS_REFERENCE`` points).  The reference source never ships; only these vectors do.

    python tests/golden/gen_body_golden.py

The mesh: an octahedron (6 vertices, 8 outward faces), every vertex moved by a seeded 5 % so that nothing is symmetric or tied.  Its
attributes follow ``oracle.lbs_oracle.synthetic_body_model`` with V = 6, plus seeded ``vertex_label`` in 0..14 and a non-zero seeded
``posedirs``.  For J in {24, 52} and B in {1, 10, 16} (key prefix ``J<J>_B<B>_``):

G-a  two levels of the loop at smpl_layer.py:306-351 WITHOUT the filter, restated with the imported ``geometry_ops.subdivide_meshes``
     (``trimesh`` stubbed as a module: the function does not call it): the level-2 vertices and attributes (the level-1 arrays are
     their first 18 rows), the faces and the renormalised regressor of both levels.
G-b  the eight outputs of the imported ``utils/body_model/lbs.lbs`` (``smplx.lbs`` stubbed with the reference's vendored copy of the same
     functions, as gen_lbs_golden.py does) for the t-pose, ``da_pose`` and one AMASS pose, ``disable_posedirs`` both ways, two betas, on the
     level-0 and level-1 models.  Outputs that do not depend on a switch are stored once, after a check that they are indeed equal:
     ``v_shaped`` / ``shape_offsets`` per (level, betas); ``J_transformed`` / ``A`` / ``T`` per pose; ``verts`` / ``v_posed`` / ``pose_offsets``
     per (pose, switch).  The arrays of one (J, B) are packed into ``gb_pack`` with their names and shapes in ``gb_index`` (JSON).  On
     level 1 ``posedirs`` is the zeros the reference's loop leaves (smpl_layer.py:351).
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("SINGS_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")     # a checkout of the reference
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

tm = types.ModuleType("trimesh")
tm.grouping = types.ModuleType("trimesh.grouping")
tm.geometry = types.ModuleType("trimesh.geometry")
tm.geometry.faces_to_edges = None
sys.modules.update({"trimesh": tm, "trimesh.grouping": tm.grouping, "trimesh.geometry": tm.geometry})
from sings.rec.utils.geometry_ops import subdivide_meshes        # noqa: E402
from sings.rec.utils.body_model import smpl as vsmpl             # noqa: E402  (vendored SMPL math)

stub = types.ModuleType("smplx.lbs")
for fn in ("batch_rodrigues", "blend_shapes", "vertices2joints", "batch_rigid_transform"):
    setattr(stub, fn, getattr(vsmpl, fn))
sys.modules["smplx"] = types.ModuleType("smplx")
sys.modules["smplx.lbs"] = stub
from sings.rec.utils.body_model import lbs as rlbs               # noqa: E402

from oracle.lbs_oracle import synthetic_body_model               # noqa: E402  (inputs only)

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)


def test_model(J, B):
    """The level-0 model of one (J, B): dict of numpy arrays."""
    rs = np.random.RandomState(1000 * J + B)
    bm = synthetic_body_model(seed=J + B, V=6, J=J, nbetas=B)
    bm["v_template"] = (OCTA_V + 0.05 * rs.uniform(-1, 1, (6, 3))).astype(np.float32)
    bm["shapedirs"] = (bm["shapedirs"] * 5).astype(np.float32)
    bm["faces"] = OCTA_F
    bm["vertex_label"] = rs.randint(0, 15, 6).astype(np.int64)
    bm["posedirs"] = rs.normal(0, 0.01, ((J - 1) * 9, 18)).astype(np.float32)
    return bm


def poses_for(J):
    amass = np.load(os.path.join(REF, "data/animation/AMASS/SFU/0008/0008_Walking002_poses.npz"))["poses"][100].astype(np.float32)
    da = np.zeros(3 * J, np.float32); da[3 + 2] = 1.0; da[3 + 5] = -1.0                # get_predefined_pose('da_pose') on body_pose
    if J == 24:
        rows = np.arange(0, 156).reshape((-1, 3))[list(range(23)) + [37]].reshape(-1)
        am = amass[rows]
    else:
        am = amass[:156]
    return np.stack([np.zeros(3 * J, np.float32), da, am])


out = {"octa_verts": OCTA_V, "octa_faces": OCTA_F}
for J in (24, 52):
    for B in (1, 10, 16):
        pre = f"J{J}_B{B}_"
        bm = test_model(J, B)
        for k in ("v_template", "shapedirs", "J_regressor", "lbs_weights", "parents", "vertex_label", "posedirs"):
            out[pre + k] = bm[k]
        rs = np.random.RandomState(7 * J + B)
        betas = rs.normal(0, 1, (2, B)).astype(np.float32)
        poses = poses_for(J)
        out[pre + "betas"] = betas; out[pre + "poses"] = poses
        # ---- G-a: the loop of smpl_layer.py:306-351 without the filter
        v, f = T(bm["v_template"]), T(bm["faces"])
        vid, lab, w, sd, Jr = torch.arange(6), T(bm["vertex_label"]), T(bm["lbs_weights"]), T(bm["shapedirs"]), T(bm["J_regressor"])
        levels = [dict(v=v, w=w, sd=sd, Jr=Jr, posedirs=T(bm["posedirs"]))]
        for level in (1, 2):
            n0 = v.shape[0]
            v, f, at = subdivide_meshes(vertices=v, faces=f, vertex_attributes={
                "vertex_id": vid, "vertex_label": lab, "lbs_weights": w, "shapedirs": sd.reshape(n0, -1), "J_regressor": Jr.transpose(1, 0)})
            vid, lab, w = at["vertex_id"], at["vertex_label"], at["lbs_weights"]
            sd = at["shapedirs"].reshape(-1, 3, B)
            Jr = at["J_regressor"].transpose(1, 0)
            Jr = Jr / Jr.sum(dim=1, keepdim=True)
            out[pre + f"ga_faces_{level}"] = f.numpy().astype(np.int32)
            out[pre + f"ga_J_regressor_{level}"] = Jr.numpy()
            levels.append(dict(v=v, w=w, sd=sd, Jr=Jr.contiguous(), posedirs=torch.zeros((J - 1) * 9, v.shape[0] * 3)))
        out[pre + "ga_verts"] = v.numpy(); out[pre + "ga_vertex_id"] = vid.numpy().astype(np.int32)
        out[pre + "ga_vertex_label"] = lab.numpy().astype(np.int32)
        out[pre + "ga_lbs_weights"] = w.numpy(); out[pre + "ga_shapedirs"] = sd.numpy()
        # ---- G-b: lbs() on the level-0 and level-1 models, packed into one array with an index (hundreds of small members would
        # cost more in archive headers than in data)
        parents = T(bm["parents"])
        combo_out, out = out, {}
        for lv in (0, 1):
            m = levels[lv]
            for ib in range(2):
                for ip in range(3):
                    res = {}
                    for off in (False, True):
                        res[off] = [t.numpy()[0] for t in rlbs.lbs(T(betas[ib:ib + 1]), T(poses[ip:ip + 1]), m["v"][None], m["sd"], m["posedirs"],
                                                                   m["Jr"], parents, m["w"], pose2rot=True, disable_posedirs=off)]
                    key = pre + f"gb_L{lv}_b{ib}_p{ip}_"
                    names = ("verts", "J_transformed", "A", "T", "v_posed", "v_shaped", "shape_offsets", "pose_offsets")
                    for i, name in enumerate(names):
                        if name in ("J_transformed", "A", "T", "v_shaped", "shape_offsets"):
                            assert np.array_equal(res[False][i], res[True][i]), name
                    if ip == 0:
                        out[pre + f"gb_L{lv}_b{ib}_v_shaped"] = res[False][5]; out[pre + f"gb_L{lv}_b{ib}_shape_offsets"] = res[False][6]
                    else:
                        assert np.array_equal(out[pre + f"gb_L{lv}_b{ib}_v_shaped"], res[False][5])
                        assert np.array_equal(out[pre + f"gb_L{lv}_b{ib}_shape_offsets"], res[False][6])
                    out[key + "J_transformed"] = res[False][1]; out[key + "A"] = res[False][2]; out[key + "T"] = res[False][3]
                    for off in (False, True):
                        for i in (0, 4, 7):
                            out[key + f"{names[i]}_off{int(off)}"] = res[off][i]
        names_shapes = [(k[len(pre):], list(a.shape)) for k, a in out.items()]
        combo_out[pre + "gb_index"] = np.array(json.dumps(names_shapes))
        combo_out[pre + "gb_pack"] = np.concatenate([a.astype(np.float32).ravel() for a in out.values()])
        out = combo_out

dst = os.path.join(ROOT, "tests", "golden", "body_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst) // 1024, "KiB,", len(out), "arrays")
