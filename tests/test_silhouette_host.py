"""Host tests of the soft silhouette and the pose refinement's host pieces (include/sings_silhouette.h, ``_lib._PROTOTYPES_SILHOUETTE``,
sings_amd/silhouette.py, ``pose_refine.write_refined_poses``): the fifteenth header is held to its table and the Makefile, the numpy
twin of the binning to a brute-force count from the definition's own ``on`` sets, the workspace plan to its sizes, and the
division-free gradient the backward kernel computes to the twin's autograd.  The device is held to the twins in
tests/test_gpu_silhouette.py and tests/test_gpu_pose_refine.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import silhouette_case as sc
from sings_amd import _lib
from sings_amd import pose_refine as PR
from sings_amd import silhouette as S


def test_header_is_bound_with_its_types(repo_root):
    text = open(os.path.join(repo_root, "include", "sings_silhouette.h")).read()
    assert re.search(r'#include\s+"sings_hip.h"', text)
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = re.findall(r"\b(int|size_t)\s*(sg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr)
    assert [n for _, n, _ in protos] == list(_lib._PROTOTYPES_SILHOUETTE) and len(protos) == 4
    assert all(n.startswith("sg_sil_") for n in _lib._PROTOTYPES_SILHOUETTE)
    others = set()
    for name in dir(_lib):
        if name.startswith("_PROTOTYPES") and name != "_PROTOTYPES_SILHOUETTE":
            others |= set(getattr(_lib, name))
    assert not set(_lib._PROTOTYPES_SILHOUETTE) & others and not set(_lib._PROTOTYPES_SILHOUETTE) & set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 8
    main = open(os.path.join(repo_root, "include", "sings_hip.h")).read()
    assert "sg_sil_" not in main
    lib = _lib.load()
    assert _lib.HAS_SILHOUETTE
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
    for name in ("TILE", "CHUNK", "SORT_LDS", "MAX_FRAMES", "GUARD_WORDS", "INFO_WORDS", "POSE"):
        assert int(re.search(rf"#define\s+SG_SIL_{name}\s+(\d+)", text).group(1)) == getattr(_lib, "SIL_" + name), name
    pieces = re.findall(r"#define\s+SG_SIL_L_([A-Z_]+)\s+(\d+)", text)
    assert [p.lower() for p, _ in pieces] == [p.lower() for p in _lib.SIL_LAYOUT] and [int(i) for _, i in pieces] == list(range(len(pieces)))
    assert int(re.search(r"#define\s+SG_SIL_LAYOUT_WORDS\s+(\d+)", text).group(1)) == len(_lib.SIL_LAYOUT)
    make = open(os.path.join(repo_root, "sings_amd", "csrc", "Makefile")).read()
    assert "sg_silhouette.hip" in make and "sings_silhouette.h" in make and "sg_sil_pair.h" in make


def test_refusals_come_before_any_hip_call():
    lib = _lib.load()
    p, out = C.c_void_p(4096), (C.c_size_t * len(_lib.SIL_LAYOUT))()
    cases = (
        (lib.sg_sil_layout, (0, 6, 8, 56, 40, 100, out), b"K = 0"), (lib.sg_sil_layout, (65, 6, 8, 56, 40, 100, out), b"K = 65"),
        (lib.sg_sil_layout, (1, 6, 0, 56, 40, 100, out), b"F = 0"), (lib.sg_sil_layout, (1, 6, 8, 56, 40, 0, out), b"capacity 0"),
        (lib.sg_sil_forward, (1, 6, 8, 56, 40, 56.0, 56.0, 20.0, 28.0, 0.0, 100, p, p, p, p, None, None), b"sigma"),
        (lib.sg_sil_forward, (1, 6, 8, 56, 40, 56.0, 56.0, 20.0, 28.0, 1e-4, 100, p, p, C.c_void_p(4100), p, None, None), b"aligned"),
        (lib.sg_sil_forward, (1, 6, 8, 56, 40, 56.0, 56.0, 20.0, 28.0, 1e-4, 100, None, p, p, p, None, None), b"null pointer"),
        (lib.sg_sil_backward, (1, 6, 8, 56, 40, 56.0, 56.0, 20.0, 28.0, 1e-4, 100, p, p, p, p, p, None, p, None), b"null pointer"),
        (lib.sg_sil_pose_update, (0, 5e-3, p, p, p, p, p, p, p, p, None, None, 0, None), b"K = 0"),
        (lib.sg_sil_pose_update, (1, 5e-3, p, p, p, p, p, p, p, None, None, None, 0, None), b"null pointer"),
        (lib.sg_sil_pose_update, (1, 5e-3, p, p, p, p, p, p, p, p, p, None, 4, None), b"come together"),
    )
    for fn, args, word in cases:
        assert fn(*args) == 1 and word in lib.sg_last_error(), (args, lib.sg_last_error())


def test_workspace_plan_sizes_and_the_int32_refusal():
    K, V, F, H, W, cap = 3, 66, 128, 56, 40, 1000
    plan = S.workspace_plan(K, V, F, H, W, cap)
    assert plan["tiles"] == (3, 4)
    T = 12
    words = {"info": _lib.SIL_INFO_WORDS + K, "rec": 8 * K * F, "rect": 4 * K * F, "tile_count": K * T, "tile_start": K * T + 1, "cursor": K * T,
             "Q": K * H * W, "face_grad": 6 * K * F, "list": cap + _lib.SIL_GUARD_WORDS, "partial": 6 * cap + _lib.SIL_GUARD_WORDS}
    at = 0
    for piece in _lib.SIL_LAYOUT[:-1]:
        assert plan[piece] == at and at % 256 == 0, piece
        at += (4 * words[piece] + 255) // 256 * 256
    assert plan["bytes"] == at
    # the counters the forward zeroes in one go lie one behind the other, in front of Q
    assert plan["tile_count"] < plan["tile_start"] < plan["cursor"] < plan["Q"]
    S.workspace_plan(8, 6890, 13776, 896, 512, 2 * 8 * 110000)       # a kit's size
    for bad in ((64, 6890, 13776, 8192, 8192, 1000),                  # K H W
                (64, 100, 5000000, 64, 64, 1000),                     # 8 K F
                (1, 100, 100, 64, 64, (2 ** 31) // 6)):               # 6 capacity
        with pytest.raises(ValueError, match="does not fit int32"):
            S.workspace_plan(*bad)


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("level", [2, 3])
def test_pair_counts_twin_against_the_definitions_on_sets(level, sigma):
    verts, faces = sc.mesh(level)
    pairs, lengths = S.pair_counts_host(verts, faces, sc.INTR, sc.H, sc.W, sigma)
    valid, x0, y0, x1, y1 = S._host_rects(verts, faces, sc.INTR, sc.H, sc.W, sigma)
    gx, gy = (sc.W + 15) // 16, (sc.H + 15) // 16
    assert pairs.shape == (3,) and lengths.shape == (3, gy, gx)
    for k in range(3):
        brute = np.zeros((gy, gx), np.int64)
        for f in range(len(faces)):
            brute[y0[k, f]:y1[k, f] + 1, x0[k, f]:x1[k, f] + 1] += 1
        assert np.array_equal(brute, lengths[k]) and pairs[k] == brute.sum()
        # every tile that has an `on` pixel of a face lists that face (the definition in fp64)
        table = sc.pair_table(verts[k], faces, sc.INTR, sc.H, sc.W, sigma)
        assert np.array_equal(table["valid"], valid[k])
        on = table["on"]
        pad = np.zeros((gy * 16, gx * 16, len(faces)), bool)
        pad[:sc.H, :sc.W] = on
        tile_on = pad.reshape(gy, 16, gx, 16, -1).any((1, 3))        # [gy,gx,F]
        ty, tx, ff = np.nonzero(tile_on)
        assert len(ff) > 0 and len(ff) <= pairs[k]
        assert ((x0[k, ff] <= tx) & (tx <= x1[k, ff]) & (y0[k, ff] <= ty) & (ty <= y1[k, ff])).all()
        print(f"level {level} sigma {sigma} frame {k}: {pairs[k]} pairs, {len(ff)} with an on pixel, longest list {lengths[k].max()} "
              f"(of on pixels: {tile_on.sum(-1).max()})")


def test_pair_counts_twin_skips_what_the_definition_skips():
    verts, faces = sc.mesh(2, K=1)
    v = verts[0].copy()
    v = np.concatenate([v, [[0.0, 0.0, 5e-4], [np.nan, 0.0, 4.0]]]).astype(np.float32)
    n = len(verts[0])
    extra = np.array([[0, 0, 1], [0, 1, n], [2, 3, n + 1], [0, 1, n + 7], [-1, 0, 1]])
    pairs, lengths = S.pair_counts_host(v, np.concatenate([faces, extra]), sc.INTR, sc.H, sc.W)
    base, base_len = S.pair_counts_host(verts[0], faces, sc.INTR, sc.H, sc.W)
    assert np.array_equal(pairs, base) and np.array_equal(lengths, base_len)
    behind = verts.copy(); behind[..., 2] -= 10.0
    assert S.pair_counts_host(behind, faces, sc.INTR, sc.H, sc.W)[0].tolist() == [0]


def test_corner_csr():
    faces = np.array([[0, 1, 2], [2, 1, 3], [0, 3, 9]])
    row_ptr, corner = S.corner_csr(faces, 4)
    assert row_ptr.tolist() == [0, 2, 4, 6, 8] and corner.tolist() == [0, 6, 1, 4, 2, 3, 5, 7]


def test_division_free_gradient_equals_the_twins_autograd():
    """d alpha / d x_f = -Q prob_f, chained through the nearest edge's clamped parameter: what the backward kernel computes, stated in
    numpy fp64, against autograd through the definition (which goes through torch.prod, min, clamp and where)."""
    tw = sc.case(2, 1e-4)
    verts, faces = tw["verts"], tw["faces"]
    fx, fy, cx, cy = sc.INTR
    for k in range(verts.shape[0]):
        t = sc.pair_table(verts[k], faces, sc.INTR, sc.H, sc.W, 1e-4)
        on = t["on"]
        x = np.where(on, np.where(t["inside"], -t["d2n"], t["d2n"]) / 1e-4, 0.0)
        with np.errstate(over="ignore"):
            prob = np.where(on, 1.0 / (1.0 + np.exp(x)), 0.0)
        Q = np.prod(1.0 - prob, -1)
        assert np.abs((1 - Q) - tw["alpha64"][k]).max() <= 1e-14
        dx_f = -(tw["g"][k].astype(np.float64) * Q)[..., None] * prob              # dL/dx_f [H,W,F]
        coef = dx_f * np.where(t["inside"], -1.0, 1.0) * t["s2"] / 1e-4 * -2.0     # times d d2 / d corner = -2 (1 - t | t) (dx, dy)
        guv = np.zeros((len(faces), 3, 2))
        for e in range(3):
            sel = (t["edge"] == e) & on
            for corner, w in ((e, 1.0 - t["t"]), ((e + 1) % 3, t["t"])):
                guv[:, corner, 0] += np.where(sel, coef * w * t["dx"], 0.0).sum((0, 1))
                guv[:, corner, 1] += np.where(sel, coef * w * t["dy"], 0.0).sum((0, 1))
        grad = np.zeros((verts.shape[1], 3))
        p = verts[k].astype(np.float64)[faces]                       # [F,3,3]
        np.add.at(grad, (faces, 0), guv[..., 0] * fx / p[..., 2])
        np.add.at(grad, (faces, 1), guv[..., 1] * fy / p[..., 2])
        np.add.at(grad, (faces, 2), -(guv[..., 0] * fx * p[..., 0] + guv[..., 1] * fy * p[..., 1]) / p[..., 2] ** 2)
        scale = np.abs(tw["grad64"][k]).max()
        err = np.abs(grad - tw["grad64"][k]).max()
        print(f"frame {k}: gradient scale {scale:.3e}, division-free against autograd {err:.3e}")
        assert scale > 1.0 and err <= 1e-9 * scale


def test_write_refined_poses(tmp_path):
    rs = np.random.RandomState(0)
    betas, go, bp, tr = rs.randn(1, 10), rs.randn(5, 3), rs.randn(5, 69), rs.randn(5, 3)
    path = tmp_path / "score_demo_video" / "poses_optimized.npz"
    assert PR.write_refined_poses(path, betas, go, bp, tr) == str(path)
    z = np.load(path)
    assert sorted(z.files) == ["betas", "body_pose", "global_orient", "transl"]
    assert z["betas"].shape == (10,) and z["global_orient"].shape == (5, 3) and z["body_pose"].shape == (5, 69) and z["transl"].shape == (5, 3)
    assert all(z[k].dtype == np.float32 for k in z.files) and np.array_equal(z["body_pose"], bp.astype(np.float32))
    from sings_amd import kit
    back = kit.load_smpl_param(path)
    assert back["betas"].shape == (1, 10) and np.array_equal(back["global_orient"], go.astype(np.float32))
    with pytest.raises(FileExistsError):
        PR.write_refined_poses(path, betas, go, bp, tr)
    assert np.array_equal(np.load(path)["body_pose"], bp.astype(np.float32))
    PR.write_refined_poses(path, betas, go, 2 * bp, tr, overwrite=True)
    assert np.array_equal(np.load(path)["body_pose"], (2 * bp).astype(np.float32))
    # atomic: a refused or failed write leaves the file as it was and nothing beside it
    with pytest.raises(ValueError, match="must be"):
        PR.write_refined_poses(path, betas, go, bp[:, :60], tr, overwrite=True)
    bad = bp.copy(); bad[2, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        PR.write_refined_poses(path, betas, go, bad, tr, overwrite=True)
    assert np.array_equal(np.load(path)["body_pose"], (2 * bp).astype(np.float32))
    assert os.listdir(path.parent) == ["poses_optimized.npz"]


def test_the_op_and_the_engine_refuse_host_tensors():
    verts, faces = sc.mesh(2, K=1)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        S.soft_silhouette(torch.from_numpy(verts), torch.from_numpy(faces), sc.INTR, sc.H, sc.W)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        S.soft_silhouette(verts, faces, sc.INTR, sc.H, sc.W)
    with pytest.raises(RuntimeError, match="lives on the GPU"):
        S.SilhouetteWorkspace(1, verts.shape[1], torch.from_numpy(faces).int(), sc.H, sc.W, 1000, "cpu")
    import pose_refine_case as prc
    spec = PR.RefineSpec.smpl()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        PR.RefineEngine(prc.model(), torch.zeros(10), prc.CAMERA, spec, prc.extra_ids(66))
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU tensor"):
        PR.refine_pose(prc.model(), z(10), z(2, 3), z(2, 69), z(2, 3), prc.CAMERA, z(2, sc.H, sc.W), z(2, 133, 2), z(2, 133), spec,
                       prc.extra_ids(66))
