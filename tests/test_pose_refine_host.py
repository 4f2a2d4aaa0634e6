"""Host tests of the pose refinement (sings_amd/pose_refine.py, sings_amd/kit.py ``load_keypoints``): the presets against the results of
the reference's own functions (tests/golden/gen_pose_refine_golden.py), the shipped pose pair, the keypoint parser, and the fp64 twin
of the soft silhouette -- analytic cases, its gradient against central differences, degenerate faces, the loss normalisations and the
gate."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import body_case as bc
import pose_refine_case as pc
from sings_amd import kit
from sings_amd import pose_refine as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64 = torch.float64


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "pose_refine_golden.npz"))


@pytest.mark.parametrize("preset,prefix,rows,lr,iters", (("smpl", "smpl_", 45, 5e-3, 100), ("smplh", "smplh_", 73, 2e-3, 50)))
def test_presets_equal_the_reference_s_tables(g, preset, prefix, rows, lr, iters):
    spec = getattr(PR.RefineSpec, preset)()
    assert spec.n_joint_rows == rows and spec.lr == lr and spec.iterations == iters
    assert spec.score_threshold == 0.8 and spec.sigma == 1e-4
    assert spec.grad_mask.dtype == np.float64 and np.array_equal(spec.grad_mask, g[prefix + "grad_mask"])
    assert spec.limits.shape == (72, 2) and np.array_equal(spec.limits, g[prefix + "limits"])
    src = torch.arange(133, dtype=F64)[:, None].repeat(1, 2)
    assert np.array_equal(spec.rows_of(src)[:, 0].numpy().astype(np.int64), g[prefix + "map"])


def test_the_shipped_pose_pair_moves_exactly_the_enabled_entries(g):
    before = np.concatenate([g["poses_global_orient"], g["poses_body_pose"]], 1)
    after = np.concatenate([g["opt_global_orient"], g["opt_body_pose"]], 1)
    assert before.shape == (80, 72)
    moved = (before.view(np.int32) != after.view(np.int32)).any(0)
    expected = {(4, 0), (5, 0)} | {(j, a) for j in (7, 8, 18, 19) for a in range(3)}
    assert {(i // 3, i % 3) for i in np.nonzero(moved)[0]} == expected
    assert np.array_equal(moved, PR.RefineSpec.smpl().enabled())
    assert np.array_equal(g["poses_transl"], g["opt_transl"])


def _mini_kit(tmp_path, n=3):
    src = os.path.join(GOLDEN, "pose_refine_keypoints_000000.json")
    os.makedirs(tmp_path / "images")
    os.makedirs(tmp_path / kit.KEYPOINT_DIR)
    for i in range(n):
        (tmp_path / "images" / f"{i:06d}.png").write_bytes(b"")
        shutil.copyfile(src, tmp_path / kit.KEYPOINT_DIR / f"{i:06d}.json")
    return tmp_path


def test_load_keypoints(g, tmp_path):
    root = _mini_kit(tmp_path)
    kp, sc = kit.load_keypoints(root)
    assert kp.shape == (3, 133, 2) and sc.shape == (3, 133) and kp.dtype == sc.dtype == np.float32
    assert np.array_equal(kp[1], g["keypoints"][0].astype(np.float32)) and np.array_equal(sc[2], g["scores"][0].astype(np.float32))
    kp1, _ = kit.load_keypoints(root, indices=[2])
    assert kp1.shape == (1, 133, 2)
    path = root / kit.KEYPOINT_DIR / "000001.json"
    whole = json.load(open(path))
    for breaker in (lambda d: d["instance_info"][0].pop("keypoints"), lambda d: d["instance_info"][0].pop("keypoint_scores"),
                    lambda d: d.pop("instance_info"), lambda d: d["instance_info"].clear(),
                    lambda d: d["instance_info"][0].__setitem__("keypoints", d["instance_info"][0]["keypoints"][:17])):
        d = json.loads(json.dumps(whole))
        breaker(d)
        path.write_text(json.dumps(d))
        with pytest.raises(ValueError, match="000001.json"):
            kit.load_keypoints(root)
    path.write_text(json.dumps(whole))
    (root / "images" / "000009.png").write_bytes(b"")
    with pytest.raises(ValueError, match="3 keypoint files for 4 images"):
        kit.load_keypoints(root)


# ---- the twin of the silhouette: analytic cases -------------------------------------------------------------------------------------------
H = W = 32
INTR = (1.0, 1.0, 0.0, 0.0)                      # with z = 1: x and y ARE pixels
TRI = [[4.0, 4.0, 1.0], [28.0, 4.0, 1.0], [4.0, 28.0, 1.0]]


def _alpha(verts, faces, sigma=1e-4, **kw):
    return PR.silhouette_host(torch.tensor(verts, dtype=F64), np.asarray(faces), INTR, H, W, sigma, **kw)


def test_one_triangle_analytic_cases():
    sigma = 1e-4
    a, counts = _alpha(TRI, [[0, 1, 2]], sigma, return_counts=True)
    s = 2.0 / 32
    assert float(a[10, 10]) == 1.0                                   # deep inside: exp(-d2 / sigma) underflows against 1
    band_px = np.sqrt(PR.LOGIT * sigma) / s                          # 0.4856 px
    assert 0.48 < band_px < 0.49
    assert float(a[30, 30]) == 0.0 and float(a[3, 10]) == 0.0        # beyond the band: exactly 0 (row 3's centres are 0.5 px off the edge)
    assert int(counts) == 1
    # a pixel centre ON an edge: d2 = 0, neither strictly inside nor beyond the band -> exactly 0.5
    tri = [[4.5, 4.5, 1.0], [28.5, 4.5, 1.0], [4.5, 28.5, 1.0]]
    a = _alpha(tri, [[0, 1, 2]], sigma)
    assert float(a[4, 10]) == 0.5 and float(a[10, 4]) == 0.5
    # a pixel in the band, inside and outside: the definition's number
    tri = [[4.25, 4.25, 1.0], [28.25, 4.25, 1.0], [4.25, 28.25, 1.0]]
    a = _alpha(tri, [[0, 1, 2]], sigma)
    d2 = (0.25 * s) ** 2
    assert float(a[4, 10]) == pytest.approx(1 / (1 + np.exp(-d2 / sigma)), rel=1e-12)       # centre 4.5: 0.25 px inside
    assert float(a[3, 10]) == 0.0                                                            # centre 3.5: 0.75 px outside, beyond
    # two coincident faces (one of them the back face): 1 - (1 - p)^2
    p = float(a[4, 10])
    a2, counts = _alpha(tri, [[0, 1, 2], [0, 2, 1]], sigma, return_counts=True)
    assert float(a2[4, 10]) == pytest.approx(1 - (1 - p) ** 2, rel=1e-12) and int(counts) == 2


def test_degenerate_faces_change_nothing():
    verts = TRI + [[10.0, 10.0, -1.0], [12.0, 10.0, -1.0], [10.0, 12.0, -1.0], [16.0, 16.0, 1.0]]
    base = torch.tensor(verts, dtype=F64, requires_grad=True)
    w = torch.randn(H, W, dtype=F64, generator=torch.Generator().manual_seed(2))
    a0 = PR.silhouette_host(base, np.array([[0, 1, 2]]), INTR, H, W, 4e-3)
    g0, = torch.autograd.grad((a0 * w).sum(), base)
    faces = np.array([[0, 1, 2], [3, 4, 5], [0, 0, 6], [0, 1, 5]])   # behind the camera, zero area, one corner behind the camera
    a1 = PR.silhouette_host(base, faces, INTR, H, W, 4e-3)
    g1, = torch.autograd.grad((a1 * w).sum(), base)
    # (the gradient to within the rounding of autograd's scatter, whose order of additions changes with the number of faces)
    assert torch.equal(a0, a1) and bool(torch.isfinite(g1).all()) and float((g0 - g1).abs().max()) <= 1e-13 * float(g0.abs().max())
    assert not g1[3:].any()
    nan = base.detach().clone()
    nan[6, 0] = float("nan")
    assert torch.equal(PR.silhouette_host(nan, faces, INTR, H, W, 4e-3), a0.detach())


def test_the_twin_s_gradient_against_central_differences():
    m = bc.model_arrays(24, 10, level=1)
    v0 = torch.tensor(np.asarray(m["v_template"], np.float64)) + torch.tensor([0.05, 0.02, 4.0], dtype=F64)
    faces, Wd, Hd, intr, sigma = m["faces"], 24, 20, (40.0, 42.0, 11.5, 10.3), 4e-3
    w = torch.randn(Hd, Wd, dtype=F64, generator=torch.Generator().manual_seed(1))
    f = lambda v: (PR.silhouette_host(v, faces, intr, Hd, Wd, sigma) * w).sum()
    v = v0.clone().requires_grad_(True)
    grad, = torch.autograd.grad(f(v), v)
    eps, num = 1e-6, torch.zeros_like(v0)
    with torch.no_grad():
        for i in range(v0.shape[0]):
            for j in range(3):
                vp, vm = v0.clone(), v0.clone()
                vp[i, j] += eps
                vm[i, j] -= eps
                num[i, j] = (f(vp) - f(vm)) / (2 * eps)
    scale = float(grad.abs().max())
    assert scale > 1.0 and float((grad - num).abs().max()) < 1e-7 * scale


# ---- the two terms and the gate -------------------------------------------------------------------------------------------------------------
def test_loss_normalisations_on_a_hand_computed_case():
    spec = PR.RefineSpec.smpl()
    kp = torch.zeros(1, 133, 2, dtype=F64)
    sc = torch.ones(1, 133, dtype=F64)
    kp[0, 13], kp[0, 14], kp[0, 15] = torch.tensor([10.0, 20.0]), torch.tensor([30.0, 40.0]), torch.tensor([5.0, 6.0])
    sc[0, 15] = 0.79                                                 # below the threshold: dropped
    target, used = PR.keypoint_targets(kp, sc, spec)
    assert used[0].nonzero().flatten().tolist() == [4, 5] and target[0, 4].tolist() == [10.0, 20.0]
    proj = torch.zeros(1, 45, 2, dtype=F64)
    proj[0, 4], proj[0, 5], proj[0, 7] = torch.tensor([11.0, 22.0]), torch.tensor([30.0, 37.0]), torch.tensor([100.0, 100.0])
    term, n = PR.keypoint_term(proj, target, used)
    # mse over 2 rows x 2 coordinates = (1 + 4 + 0 + 9) / 4, then / 2 rows
    assert int(n) == 2 and float(term) == (1 + 4 + 0 + 9) / 4 / 2
    ref = torch.nn.functional.mse_loss(proj[0][used[0]], target[0][used[0]]) / used[0].sum()
    assert float(term) == float(ref)
    none, n0 = PR.keypoint_term(proj, target, torch.zeros_like(used))
    assert float(none) == 0.0 and int(n0) == 0
    a, m = torch.tensor([[[0.5, 1.0], [0.0, 0.25]]], dtype=F64), torch.tensor([[[1.0, 1.0], [0.0, 0.0]]], dtype=F64)
    assert float(PR.silhouette_term(a, m)) == (0.25 + 0 + 0 + 0.0625) / 4
    # the projection's crop: behind the camera, u < 0, u >= W - 1, v >= H - 1 -> (0, 0); v < 0 is kept, as the reference keeps it
    pts = torch.tensor([[1.0, 1.0, -1.0], [-1.0, 1.0, 1.0], [31.0, 1.0, 1.0], [1.0, 31.0, 1.0], [1.0, -3.0, 1.0], [2.0, 3.0, 1.0]], dtype=F64)
    assert PR.project_joints(pts, INTR, 32, 32).tolist() == [[0, 0], [0, 0], [0, 0], [0, 0], [1.0, -3.0], [2.0, 3.0]]


def test_the_gate_keeps_masked_and_out_of_limit_entries_bit_equal():
    k = pc.kit(1)
    spec = PR.RefineSpec.smpl()
    start = k["start"].copy()
    start[0, 12] = -0.05                                             # the left knee's x below its limit [0, 160 deg]: frozen where it is
    start[0, 21] = 2.0                                               # the left ankle's x above 90 deg
    go, bp, rep = PR.refine_pose_host(k["model"], k["betas"], start[:, :3], start[:, 3:], k["transl"], pc.CAMERA, k["masks"],
                                      k["keypoints"], k["scores"], spec, k["extra"], iterations=10)
    out = np.concatenate([go, bp], 1)
    frozen = ~spec.enabled()
    frozen[[12, 21]] = True
    assert np.array_equal(out[0, frozen], start[0, frozen].astype(np.float64))
    moving = ~frozen
    assert (out[0, moving] != start[0, moving]).all()
    assert rep["keypoints_used"].tolist() == [14] and rep["last_loss"][0] < rep["first_loss"][0]
