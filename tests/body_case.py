"""What the body-model tests share: the fixture of tests/golden/gen_body_golden.py unpacked, the test models as keyword arguments of
``BodyModel``, the plain octahedron levels the filter tests run on, and the tolerance rule of the device results.

The tolerance rule (floats of the body model): with the fp64 twin evaluated on the same inputs, the device result may lie at most
twice as far from it as the reference's own fp32 result does, with a floor of one ulp of the array's scale (its largest magnitude)."""
import json
import os

import numpy as np

from sings_amd import body_model as BM

JS, BS = (24, 52), (1, 10, 16)
COMBOS = [(J, B) for J in JS for B in BS]
_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "body_golden.npz"))
    return _G


def gb(J, B):
    """The packed G-b arrays of one (J, B): dict name -> fp32 array."""
    g, pre = golden(), f"J{J}_B{B}_"
    pack, out, at = g[pre + "gb_pack"], {}, 0
    for name, shape in json.loads(str(g[pre + "gb_index"])):
        n = int(np.prod(shape))
        out[name] = pack[at:at + n].reshape(shape)
        at += n
    assert at == pack.shape[0]
    return out


def model_arrays(J, B, level=0):
    """The keyword arguments of ``BodyModel`` for the level-0 model of (J, B), or for the reference's level-1 / level-2 model (G-a:
    its arrays, its renormalised regressor; ``posedirs`` dropped)."""
    g, pre = golden(), f"J{J}_B{B}_"
    if level == 0:
        return dict(v_template=g[pre + "v_template"], shapedirs=g[pre + "shapedirs"], J_regressor=g[pre + "J_regressor"],
                    lbs_weights=g[pre + "lbs_weights"], parents=g[pre + "parents"], faces=g["octa_faces"],
                    vertex_label=g[pre + "vertex_label"], posedirs=g[pre + "posedirs"])
    V = (6, 18, 66)[level]
    return dict(v_template=g[pre + "ga_verts"][:V], shapedirs=g[pre + "ga_shapedirs"][:V], J_regressor=g[pre + f"ga_J_regressor_{level}"],
                lbs_weights=g[pre + "ga_lbs_weights"][:V], parents=g[pre + "parents"], faces=g[pre + f"ga_faces_{level}"],
                vertex_label=g[pre + "ga_vertex_label"][:V], posedirs=None)


def octa_level(level, seed=5):
    """The octahedron, every vertex moved by a seeded 5 %, subdivided ``level`` times without a filter -> (verts fp32, faces, edges)."""
    g = golden()
    rs = np.random.RandomState(seed)
    v = (g["octa_verts"] + 0.05 * rs.uniform(-1, 1, (6, 3))).astype(np.float32)
    f = g["octa_faces"].astype(np.int64)
    for _ in range(level):
        v, f, _, _ = BM.subdivide_host(v, f, {})
    e = np.unique(np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)
    return v, f, e


def held(device, reference32, twin64, what):
    """The tolerance rule; prints both errors.  -> (device error, reference error, allowed)."""
    d = np.asarray(device, np.float64)
    t = np.asarray(twin64, np.float64)
    assert d.shape == t.shape == np.asarray(reference32).shape, (what, d.shape, t.shape, np.asarray(reference32).shape)
    e_ref = float(np.abs(np.asarray(reference32, np.float64) - t).max())
    e_dev = float(np.abs(d - t).max())
    ulp = float(np.spacing(np.float32(np.abs(t).max())))
    allowed = max(2 * e_ref, ulp)
    print(f"{what}: device {e_dev:.3e}, reference fp32 {e_ref:.3e}, one ulp of the scale {ulp:.3e}, allowed {allowed:.3e}")
    assert e_dev <= allowed, (what, e_dev, e_ref, ulp)
    return e_dev, e_ref, allowed
