"""The soft silhouette on the GPU (sings_amd/silhouette.py, csrc/sg_silhouette.hip) against ``pose_refine.silhouette_host``: alpha and
dL/dverts_cam follow ``body_case.held`` (at most twice as far from the fp64 twin as the fp32 twin is, floor one ulp of the scale;
both errors are measured here, from the twins); pairs per frame, tile list lengths, the lists themselves and the largest number of
blended faces of a pixel are integers and equal the host twin's.  Borderline pixels: tests/silhouette_case.py.

The camera is 40 x 56: three tile columns and four tile rows, the last of each partial.  The host count of the parity cases' lists runs
from about 80 (level 2) over 330 / 460 (level 3) to over 1 100 / 1 600 (level 4): below the staging chunk of 256, across it, across
the 1 024 up to which a list is sorted in LDS."""
import numpy as np
import pytest
import torch

import body_case as bc
import silhouette_case as sc
from sings_amd import pose_refine as PR
from sings_amd import silhouette as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W, INTR = sc.H, sc.W, sc.INTR


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def run(verts, faces, sigma, g=None, counts=False, capacity=None, check=True, intr=INTR, H=H, W=W):
    """One forward (and backward with ``g``) in a workspace of the test's own -> dict of numpy arrays and the workspace."""
    single = verts.ndim == 2
    K, V = (1, verts.shape[0]) if single else verts.shape[:2]
    f32 = _t(faces, torch.int32)
    cap = S.default_capacity(K, len(faces)) if capacity is None else capacity
    work = S.SilhouetteWorkspace(K, V, f32, H, W, cap, DEV)
    v = _t(verts).requires_grad_(True)
    out = S.soft_silhouette(v, f32, intr, H, W, sigma, return_counts=counts, workspace=work, check=check)
    alpha, cnt = out if counts else (out, None)
    res = dict(alpha=alpha.detach().cpu().numpy(), alpha_t=alpha.detach(), work=work)
    if cnt is not None:
        res["counts"] = cnt.cpu().numpy()
    if g is not None:
        alpha.backward(_t(g).reshape(alpha.shape))
        res["grad"], res["grad_t"] = v.grad.cpu().numpy(), v.grad
    return res


def check_integers(res, verts, faces, sigma, twin_counts=None, intr=INTR, H=H, W=W):
    work = res["work"]
    pairs, lengths = S.pair_counts_host(verts, faces, intr, H, W, sigma)
    over, total, per_frame = work.info()
    assert not over and total == pairs.sum() and np.array_equal(per_frame, pairs)
    assert np.array_equal(work.tile_lengths(), lengths)
    _, x0, y0, x1, y1 = S._host_rects(verts, faces, intr, H, W, sigma)
    gx, gy = work.plan["tiles"]
    for k, lists in enumerate(work.tile_lists()):
        for t, lst in enumerate(lists):
            ty, tx = divmod(t, gx)
            want = np.nonzero((x0[k] <= tx) & (tx <= x1[k]) & (y0[k] <= ty) & (ty <= y1[k]))[0]
            assert np.array_equal(lst, want), (k, t)                 # ascending face index, nothing lost, nothing twice
    if twin_counts is not None:
        assert np.array_equal(res["counts"], twin_counts)
    assert work.guards_intact()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("level", sc.LEVELS)
def test_parity(level, sigma, K):
    tw = sc.case(level, sigma)
    sel = slice(0, K)
    verts, faces = tw["verts"][sel], tw["faces"]
    res = run(verts, faces, sigma, tw["g"][sel], counts=True)
    what = f"level {level} sigma {sigma} K {K}"
    print(f"{what}: longest list {res['work'].tile_lengths().max()}, max faces per pixel {res['counts'].tolist()}")
    sc.check_alpha(res["alpha"], tw, what, sel)
    bc.held(res["grad"], tw["grad32"][sel], tw["grad64"][sel], what + " dL/dverts_cam")
    check_integers(res, verts, faces, sigma, tw["counts"][sel])


def test_degenerate_faces_near_plane_and_non_finite_vertex():
    verts, faces = sc.mesh(2, K=1)
    n = verts.shape[1]
    v = np.concatenate([verts[0], [[0.0, 0.0, 5e-4], [np.nan, 0.0, 4.0]]]).astype(np.float32)[None]
    f = np.concatenate([faces, [[0, 0, 1], [5, 5, 5], [0, 1, n], [2, 3, n + 1]]])
    tw = sc.twins(v, f, INTR, H, W, 1e-4)
    base = sc.case(2, 1e-4)
    assert np.array_equal(tw["alpha64"][0], base["alpha64"][0])      # (the appended faces are skipped by the definition too)
    res = run(v, f, 1e-4, tw["g"], counts=True)
    sc.check_alpha(res["alpha"], tw, "appended faces")
    assert np.isfinite(res["grad"]).all() and (res["grad"][0, n:] == 0).all()
    bc.held(res["grad"][:, :n], tw["grad32"][:, :n], tw["grad64"][:, :n], "appended faces dL/dverts_cam")
    check_integers(res, v, f, 1e-4, tw["counts"])
    # the rest is unchanged, bit for bit: the lists hold the same faces in the same order
    plain = run(verts, faces, 1e-4, tw["g"])
    assert torch.equal(plain["alpha_t"], res["alpha_t"]) and torch.equal(plain["grad_t"][0], res["grad_t"][0, :n])


def test_partly_outside_on_each_side():
    v0, faces = sc.mesh(2, K=1)
    shifts = np.array([[1.35, 0, 0], [-1.35, 0, 0], [0, 1.9, 0], [0, -1.9, 0]], np.float32)
    verts = v0[0][None] + shifts[:, None]
    tw = sc.twins(verts, faces, INTR, H, W, 1e-4)
    inside = tw["alpha64"].reshape(4, -1).max(1)
    assert (inside > 0.99).all() and (tw["alpha64"][0][:, -1].max() > 0.5) and (tw["alpha64"][1][:, 0].max() > 0.5) \
        and (tw["alpha64"][2][-1].max() > 0.5) and (tw["alpha64"][3][0].max() > 0.5)          # each crosses its edge of the picture
    res = run(verts, faces, 1e-4, tw["g"], counts=True)
    sc.check_alpha(res["alpha"], tw, "partly outside")
    bc.held(res["grad"], tw["grad32"], tw["grad64"], "partly outside dL/dverts_cam")
    check_integers(res, verts, faces, 1e-4, tw["counts"])


def test_a_frame_behind_the_camera():
    v0, faces = sc.mesh(2, K=2)
    verts = v0.copy()
    verts[1, :, 2] -= 10.0
    g = np.random.RandomState(0).randn(2, H, W).astype(np.float32)
    res = run(verts, faces, 1e-4, g, counts=True)
    assert (res["alpha"][1] == 0).all() and (res["grad"][1] == 0).all() and res["counts"][1] == 0
    assert res["alpha"][0].max() > 0.99 and np.abs(res["grad"][0]).max() > 0
    check_integers(res, verts, faces, 1e-4)


def test_a_far_mesh_in_one_tile():
    """Level 4 (2 048 faces) at z = 9 spans about 12.5 pixels, centred in the tile [16, 32) x [16, 32): one list of 2 048 entries, the
    long-list path (sorted in place, staged in eight chunks) on a single workgroup."""
    v, faces, _ = bc.octa_level(4)
    verts = (v + np.array([(24 - INTR[2]) / INTR[0] * 9, (24 - INTR[3]) / INTR[1] * 9, 9.0])).astype(np.float32)[None]
    pairs, lengths = S.pair_counts_host(verts, faces, INTR, H, W, 1e-4)
    assert pairs[0] == 2048 and lengths[0, 1, 1] == 2048
    tw = sc.twins(verts, faces, INTR, H, W, 1e-4)
    res = run(verts, faces, 1e-4, tw["g"], counts=True)
    sc.check_alpha(res["alpha"], tw, "one tile")
    bc.held(res["grad"], tw["grad32"], tw["grad64"], "one tile dL/dverts_cam")
    check_integers(res, verts, faces, 1e-4, tw["counts"])


def test_single_mesh_input_and_the_plain_call():
    tw = sc.case(2, 1e-4)
    v = _t(tw["verts"][0]).requires_grad_(True)
    alpha, cnt = S.soft_silhouette(v, _t(tw["faces"]), INTR, H, W, return_counts=True)
    assert tuple(alpha.shape) == (H, W) and tuple(cnt.shape) == (1,) and cnt.dtype == torch.int32
    alpha.backward(_t(tw["g"][0]))
    ref = run(tw["verts"][:1], tw["faces"], 1e-4, tw["g"][:1])
    assert torch.equal(alpha.detach(), ref["alpha_t"][0]) and torch.equal(v.grad, ref["grad_t"][0])
    with pytest.raises(RuntimeError, match="float32"):
        S.soft_silhouette(v.detach().double(), _t(tw["faces"]), INTR, H, W)
    # a capacity that is too small is found and the call run again: never a silhouette with pairs missing
    again = S.soft_silhouette(v.detach(), _t(tw["faces"]), INTR, H, W, capacity=50)
    assert torch.equal(again, alpha.detach())


@pytest.mark.parametrize("level,sigma", [(3, 1e-4), (4, 4e-3)])
def test_bit_reproducible_and_frames_independent(level, sigma):
    tw = sc.case(level, sigma)
    a = run(tw["verts"], tw["faces"], sigma, tw["g"])
    b = run(tw["verts"], tw["faces"], sigma, tw["g"])
    assert torch.equal(a["alpha_t"], b["alpha_t"]) and torch.equal(a["grad_t"], b["grad_t"])
    for k in range(3):
        one = run(tw["verts"][k:k + 1], tw["faces"], sigma, tw["g"][k:k + 1])
        assert torch.equal(one["alpha_t"][0], a["alpha_t"][k]) and torch.equal(one["grad_t"][0], a["grad_t"][k]), k


def test_half_the_capacity_drops_pairs_and_writes_nothing_out_of_bounds():
    tw = sc.case(3, 4e-3)
    need = int(S.pair_counts_host(tw["verts"], tw["faces"], INTR, H, W, 4e-3)[0].sum())
    res = run(tw["verts"], tw["faces"], 4e-3, tw["g"], capacity=need // 2, check=False)
    work = res["work"]
    over, total, _ = work.info()
    assert over and total == need and work.peak() == (True, need)
    assert work.guards_intact() and np.isfinite(res["grad"]).all()
    for lists in work.tile_lists():
        for lst in lists:
            assert (np.diff(lst) > 0).all() and (lst < len(tw["faces"])).all()
    with pytest.raises(RuntimeError, match="the workspace holds"):
        S.soft_silhouette(_t(tw["verts"]), _t(tw["faces"], torch.int32), INTR, H, W, 4e-3, workspace=work)
