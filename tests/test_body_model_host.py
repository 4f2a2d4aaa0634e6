"""Host tests of the body model (include/sings_body.h, ``_lib._PROTOTYPES_BODY``, sings_amd/body_model.py): the fourteenth header is held
to its table and to the library's exports; the numpy twins -- the stated definitions the device is held to in
tests/test_gpu_body_model.py -- are held to the reference's own outputs (tests/golden/gen_body_golden.py: G-a, the subdivision loop;
G-b, ``lbs``), and the filter twin to the properties its definition promises."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import body_case as bc
from sings_amd import _lib
from sings_amd import body_model as BM


# ---- the header and its table ------------------------------------------------------------------------------------------------------
def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_body.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_BODY) and len(protos) == 5
    assert all(n.startswith("sg_body_") for n in _lib._PROTOTYPES_BODY)
    others = set()
    for name in dir(_lib):
        if name.startswith("_PROTOTYPES") and name != "_PROTOTYPES_BODY":
            others |= set(getattr(_lib, name))
    assert not set(_lib._PROTOTYPES_BODY) & others and not set(_lib._PROTOTYPES_BODY) & set(_lib.EXPORTS) and _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert _lib.HAS_BODY
    scalars = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}
    for ret, name, params in protos:
        fn = getattr(lib, name)
        params = [p.strip() for p in params.split(",")]
        assert fn.restype is scalars[ret] and len(fn.argtypes) == len(params), name
        for p, t in zip(params, fn.argtypes):
            if "*" in p or "[" in p:
                assert issubclass(t, (C._Pointer, C.c_void_p)), (name, p)
            else:
                assert t is scalars[[w for w in re.findall(r"\w+", p) if w != "const"][0]], (name, p)
    for name in ("MAX_JOINTS", "MAX_BETAS", "MAX_VERTS", "MAX_ROWS", "MAX_ITERATIONS", "INFO_INTS", "ISOLATED", "NOT_FINITE", "BAD_SLOPE",
                 "BAD_FACE"):
        assert int(re.search(rf"#define\s+SG_BODY_{name}\s+(\d+)", text).group(1)) == getattr(_lib, "BODY_" + name), name
    make = open(os.path.join(repo_root, "sings_amd", "csrc", "Makefile")).read()
    assert "sg_body.hip" in make and "sings_body.h" in make


def test_refusals_come_before_any_hip_call():
    """Every argument error is answered before a HIP call, so without a device.  (The pointers are never followed.)"""
    lib = _lib.load()
    p = C.c_void_p(4096)
    assert lib.sg_body_smooth_ws_bytes(0, 8) == 0 and lib.sg_body_smooth_ws_bytes(6, 0) == 0
    assert lib.sg_body_smooth_ws_bytes(_lib.BODY_MAX_VERTS + 1, 8) == 0
    # x, nrm, delta [3V] and a [V] fp64, two rows of partials, eight scalars, the accumulators [3V]
    assert lib.sg_body_smooth_ws_bytes(6, 8) == (9 * 6 + 6 + 2 + 8 + 18) * 8
    assert lib.sg_body_smooth_ws_bytes(1026, 2048) == (9 * 1026 + 1026 + 2 * 8 + 8 + 3 * 1026) * 8
    cases = (
        (lib.sg_body_renorm, (65, 6, p, p, None), b"J = 65"), (lib.sg_body_renorm, (24, 0, p, p, None), b"V = 0"),
        (lib.sg_body_renorm, (24, 6, None, p, None), b"null pointer"),
        (lib.sg_body_joint_basis, (6, 24, 33, p, p, p, p, p, None), b"B = 33"),
        (lib.sg_body_joint_basis, (_lib.BODY_MAX_VERTS + 1, 24, 10, p, p, p, p, p, None), b"V = 4194305"),
        (lib.sg_body_joint_basis, (6, 24, 10, p, p, p, None, p, None), b"null pointer"),
        (lib.sg_body_shaped, (6, 10, 0, 0, p, p, p, None, None, p, p, p, p, None), b"K = 0"),
        (lib.sg_body_shaped, (6, 10, 1025, 0, p, p, p, None, None, p, p, p, p, None), b"K = 1025"),
        (lib.sg_body_shaped, (6, 10, 1, -1, p, p, p, None, None, p, p, p, p, None), b"P = -1"),
        (lib.sg_body_shaped, (6, 10, 1, 207, p, p, p, None, p, p, p, p, p, None), b"null pointer"),
        (lib.sg_body_smooth, (0, 8, 5, 0.5, p, p, p, p, p, C.c_void_p(8192), p, None), b"V = 0"),
        (lib.sg_body_smooth, (6, 8, 65, 0.5, p, p, p, p, p, C.c_void_p(8192), p, None), b"65 iterations"),
        (lib.sg_body_smooth, (6, 8, 5, float("nan"), p, p, p, p, p, C.c_void_p(8192), p, None), b"not finite"),
        (lib.sg_body_smooth, (6, 8, 5, 0.5, p, p, p, p, p, p, p, None), b"alias"),
        (lib.sg_body_smooth, (6, 8, 5, 0.5, p, p, p, p, None, C.c_void_p(8192), p, None), b"null pointer"),
    )
    for fn, args, word in cases:
        assert fn(*args) == 1 and word in lib.sg_last_error(), (args, lib.sg_last_error())


# ---- the twins against the reference's subdivision loop (G-a) --------------------------------------------------------------------------
@pytest.mark.parametrize("J,B", bc.COMBOS)
def test_subdivision_twin_equals_the_reference(J, B):
    g, pre = bc.golden(), f"J{J}_B{B}_"
    m = bc.model_arrays(J, B)
    v, f = m["v_template"], m["faces"]
    at = {"vertex_id": np.arange(6, dtype=np.int32), "vertex_label": m["vertex_label"].astype(np.int32), "lbs_weights": m["lbs_weights"],
          "shapedirs": m["shapedirs"].reshape(6, -1), "J_regressor": np.ascontiguousarray(m["J_regressor"].T)}
    for level in (1, 2):
        v, f, at, _ = BM.subdivide_host(v, f, at)
        assert np.array_equal(f, g[pre + f"ga_faces_{level}"])
        want = g[pre + f"ga_J_regressor_{level}"]
        got64 = BM.renorm_host(at["J_regressor"])
        # fp32 against fp64: a sum of V values and a division, each a rounding of at most 2^-24 relative
        assert np.abs(want - got64).max() <= (len(v) + 2) * 2.0 ** -24 * np.abs(got64).max()
        assert np.abs(got64.sum(axis=1) - 1).max() <= 1e-14
        at["J_regressor"] = np.ascontiguousarray(want.T)            # (the reference's own values go into the next level)
    # a mean of two fp32 values is rounded once: equal as fp32 values
    assert v.dtype == np.float32 and np.array_equal(v, g[pre + "ga_verts"])
    for k in ("vertex_id", "vertex_label", "lbs_weights"):
        assert np.array_equal(at[k], g[pre + "ga_" + k]), k
    assert np.array_equal(at["shapedirs"].reshape(-1, 3, B), g[pre + "ga_shapedirs"])


# ---- the twins against the reference's lbs (G-b) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("J,B", bc.COMBOS)
def test_shape_joint_and_skinning_twins_equal_the_reference(J, B, level):
    g, pre, gb = bc.golden(), f"J{J}_B{B}_", bc.gb(J, B)
    m = bc.model_arrays(J, B, level)
    betas, poses = g[pre + "betas"], g[pre + "poses"]
    J0, JS = BM.joint_basis_host(m["v_template"], m["shapedirs"], m["J_regressor"])
    parents = [int(p) for p in m["parents"]]
    close = lambda a, b, tol, what: np.testing.assert_allclose(a, b, rtol=tol, atol=tol * max(1.0, float(np.abs(b).max())), err_msg=what)
    for ib in range(2):
        key = f"gb_L{level}_b{ib}_"
        for ip in range(3):
            vs, so, po, vp = (a[0] for a in BM.shaped_host(m["v_template"], m["shapedirs"], betas[ib:ib + 1], m["posedirs"], poses[ip:ip + 1]))
            close(vs, gb[key + "v_shaped"], 1e-6, "v_shaped"); close(so, gb[key + "shape_offsets"], 1e-6, "shape_offsets")
            kp = key + f"p{ip}_"
            close(po, gb[kp + "pose_offsets_off0"], 1e-6, "pose_offsets"); close(vp, gb[kp + "v_posed_off0"], 1e-6, "v_posed")
            assert float(np.abs(gb[kp + "pose_offsets_off1"]).max()) == 0.0
            jr = BM.joints_rest_host(J0, JS, betas[ib])
            # the joints are affine in betas: the folded basis gives what regressing the shaped vertices gives
            np.testing.assert_allclose(jr, m["J_regressor"].astype(np.float64) @ vs, rtol=0, atol=1e-13)
            A = BM.joint_transforms_host(poses[ip], jr, parents)
            close(A, gb[kp + "A"], 1e-5, "A")
            for off, v_in in ((0, vp), (1, vs)):
                verts, T = BM.skin_host(A, m["lbs_weights"], v_in)
                close(verts, gb[kp + f"verts_off{off}"], 1e-5, "verts"); close(T, gb[kp + "T"], 1e-5, "T")
        # the rest joints themselves: the posed joints of the t-pose (its rotations are the identity to 1e-8)
        close(BM.joints_rest_host(J0, JS, betas[ib]), gb[key + "p0_J_transformed"], 1e-6, "joints_rest")
    K3 = BM.joints_rest_host(J0, JS, np.stack([betas[0], betas[1], betas[0]]))
    assert K3.shape == (3, J, 3) and np.array_equal(K3[0], K3[2]) and np.array_equal(K3[1], BM.joints_rest_host(J0, JS, betas[1]))


# ---- the filter twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 4])
def test_filter_twin_properties(level):
    v, f, e = bc.octa_level(level)
    trace = []
    x64 = BM.smooth_host(v, f, e, lamb=0.5, iterations=5, trace=trace)
    x32 = BM.smooth_host(v, f, e, lamb=0.5, iterations=5, dtype=np.float32)
    assert x64.dtype == np.float64 and x32.dtype == np.float32 and np.isfinite(x64).all()
    # fp32 against fp64: d = |n . (x - L x)| is a difference that cancels to the local sagitta, ~ 1e-2 of the coordinates at level 4, so
    # lambda carries ~ 100 roundings' worth (1e-5) of relative error on steps of ~ 5e-2, five times over: a few 1e-6.  Bound: 2e-5.
    err = float(np.abs(x32 - x64).max())
    print(f"level {level}: fp32 evaluation {err:.3e} from fp64")
    assert err <= 2e-5
    assert len(trace) == 5
    for lam, vol_before, vol_after, vol0 in trace:
        assert lam.shape == (len(v),) and float(lam.min()) >= 0.2 * 0.5 and float(lam.max()) <= 1.0
        # The correction is one secant step with D = vol0 - vol: vol(x + t n) = vol + a1 t + a2 t^2 + ..., t = slope D, and
        # 1 / slope = a1 + a2 eps + ... measured once, at iteration 0.  Two things are left.  The second-order term a2 t^2: for a
        # round shape of radius r, vol (1 + t / r)^3 with the linear step 3 (t / r) vol = D leaves D (u + u^2 / 3), u = D / (3 vol)
        # -- at level 1, where the Laplacian step takes almost half the volume of 18 vertices, that is a third of D; half as much
        # again is allowed for a shape that is not round.  And D times the relative error of the slope: eps a2 / a1 (eps times the mean
        # curvature, below 2 %) and the drift of a1 (the area along n) over the later iterations: 5 %.
        D = abs(vol_before - vol0)
        u = D / (3 * vol_before)
        assert abs(vol_after - vol0) <= D * (1.5 * (u + u * u / 3) + 0.05) + 1e-13 * abs(vol0), (vol_before, vol_after, vol0)
    assert BM.smooth_host(v, f, e, iterations=0).astype(np.float32).tobytes() == v.tobytes()


def test_filter_twin_keeps_the_centroid_of_a_sphere():
    g = bc.golden()
    v, f = g["octa_verts"].astype(np.float64), g["octa_faces"].astype(np.int64)
    for _ in range(3):
        v, f, _, _ = BM.subdivide_host(v, f, {})
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    e = np.unique(np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)
    x = BM.smooth_host(v, f, e)
    assert np.abs(v.mean(axis=0)).max() <= 1e-15 and np.abs(x.mean(axis=0)).max() <= 1e-14
    assert np.abs(np.linalg.norm(x, axis=1) - 1).max() < 0.05


def test_filter_twin_refuses():
    v, f, e = bc.octa_level(1)
    with pytest.raises(ValueError, match="no neighbour"):
        BM.smooth_host(np.concatenate([v, [[2, 2, 2]]]), f, e)
    bad = v.copy(); bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        BM.smooth_host(bad, f, e)
    flat_v, flat_f, flat_e = flat_two_sided()
    with pytest.raises(ValueError, match="does not change"):
        BM.smooth_host(flat_v, flat_f, flat_e)


def flat_two_sided():
    """A square of two triangles and the same two triangles turned over: every vertex' face normals cancel, so the volume does not
    change along n."""
    v = np.array([[0, 0, 0.5], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0.5]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 2, 1], [0, 3, 2]], np.int64)
    e = np.unique(np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)
    return v, f, e


# ---- the loader -----------------------------------------------------------------------------------------------------------------------
def test_loader_refuses_what_it_must(tmp_path):
    with pytest.raises(ValueError, match="chumpy.*arbitrary code"):
        BM.load_body_arrays(str(tmp_path / "SMPLH_NEUTRAL.pkl"))
    m = bc.model_arrays(24, 10)
    ok = dict(v_template=m["v_template"], shapedirs=m["shapedirs"], J_regressor=m["J_regressor"], weights=m["lbs_weights"],
              kintree_table=np.stack([m["parents"], np.arange(24)]), f=m["faces"], posedirs=np.zeros((6, 3, 207), np.float32))
    np.savez(tmp_path / "sparse.npz", **dict(ok, J_regressor=np.array({"a sparse": "matrix"}, dtype=object)))
    with pytest.raises(ValueError, match="object array"):
        BM.load_body_arrays(str(tmp_path / "sparse.npz"))
    np.savez(tmp_path / "short.npz", **{k: v for k, v in ok.items() if k != "weights"})
    with pytest.raises(ValueError, match="lacks weights"):
        BM.load_body_arrays(str(tmp_path / "short.npz"))
    np.savez(tmp_path / "ok.npz", **ok)
    with pytest.raises(ValueError, match="cannot give 11 betas"):
        BM.load_body_arrays(str(tmp_path / "ok.npz"), num_betas=11)
    a = BM.load_body_arrays(str(tmp_path / "ok.npz"), num_betas=4)
    assert a["shapedirs"].shape == (6, 3, 4) and np.array_equal(a["shapedirs"], m["shapedirs"][:, :, :4]) and a["pose_mean"] is None
    assert a["posedirs"].shape == (207, 18) and a["parents"].tolist() == m["parents"].tolist()
