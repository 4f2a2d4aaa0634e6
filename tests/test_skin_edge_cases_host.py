"""CPU proof that the cases of tests/skin_edge_case.py test what tests/test_gpu_skin_edges.py claims of them, from
oracle/lbs_oracle.py and oracle/raster_oracle.py alone (the manner of tests/test_camera_general_host.py):

 * the case lists are the ones stated (every J and P edge, rotation modes and SH degrees cycling, one-hot joints);
 * visibility, the borderline-pixel cap of tests/test_gpu_raster._check_image, joint coverage;
 * every Gaussian of every case keeps its matrix_to_quaternion branch under fp32 noise;
 * the fp32 restatement's own gradient error stays within a quarter of the GPU file's bar (b) -- the measured worst ratio is the
   number quoted in skin_edge_case's docstring (``HEADROOM_MEASURED``) and in LAB.md.
"""
import functools
import math

import numpy as np
import torch

import skin_edge_case as sec
from oracle import lbs_oracle as lo
from oracle import raster_oracle as ro

BORDER = 2e-5


@functools.lru_cache(maxsize=None)
def _frames():
    return list(sec.all_frames())


def raster(s):
    """The raster oracle on the fp32 restatement's posed values of a single-frame scene."""
    _, (x, q, sc, _) = sec.deform(s)
    cam = s["cam"]
    return ro.forward(x.numpy(), s["opac"], cam["world_view_transform"], cam["full_proj_transform"], cam["camera_center"], s["W"], s["H"],
                      math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), s["bg"], scales=sc.numpy(), rotations=q.numpy(),
                      shs=s["shs"], sh_degree=s.get("deg", 0))


def view_failures(s):
    """-> list of the view conditions a scene misses (empty: none)."""
    o = raster(s)
    vis = o["radii"] > 0
    bad = []
    if s["P"] >= 63 and vis.mean() <= 0.5:
        bad.append(f"visible share {vis.mean():.2f}")
    if s["P"] == 1 and not vis[0]:
        bad.append("the lone Gaussian is out of view")
    nb = int((o["margin"] < BORDER).sum())
    if nb > 8 + 6e-4 * o["margin"].size:
        bad.append(f"{nb} borderline pixels")
    if s.get("kind") != "one_hot" and s["P"] >= 4 * s["J"]:
        idle = np.nonzero(~(s["w"][vis] > 0).any(0))[0]
        if len(idle):
            bad.append(f"joints {idle.tolist()} carry no weight on a visible Gaussian")
    return bad


def m2q_gap(s):
    """Smallest (largest - second largest candidate q_abs) of matrix_to_quaternion over the scene's Gaussians, in fp64."""
    _, (_, _, _, T) = sec.deform(s, torch.float64)
    Rc = torch.eye(3, dtype=torch.float64)[None].repeat(s["P"], 1, 1) if s["Rc"] is None else \
        lo.rotation_6d_to_matrix(torch.from_numpy(s["d6"]).double())
    m = (T[:, :3, :3] @ Rc).reshape(-1, 9)
    m00, m11, m22 = m[:, 0], m[:, 4], m[:, 8]
    q_abs = lo._sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                                1.0 - m00 - m11 + m22], -1))
    top = torch.sort(q_abs, -1, descending=True).values
    return float((top[:, 0] - top[:, 1]).min())


def headroom(s):
    """(worst ratio, array) of the fp32 restatement's gradients against the fp64 restatement's, in units of the GPU file's bar (b)."""
    gx, gq, gs = sec.upstream(s)
    g32 = sec.lbs_gradients(s, gx, gq, gs, torch.float32)
    g64 = sec.lbs_gradients(s, gx, gq, gs, torch.float64)
    worst = (0.0, "-")
    for name in sec.BAR:
        if g64[name] is None:
            continue
        worst = max(worst, (sec.bar_ratio(name, g32[name], g64[name]), name))
    return worst


def test_the_case_lists_are_the_stated_ones():
    Js = [c[1] for c in sec.SINGLE[:18]]
    assert Js == [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 42, 43, 47, 48, 49, 63, 64] and all(c[0] == 257 for c in sec.SINGLE[:18])
    assert [(c[0], c[1]) for c in sec.SINGLE[18:]] == [(P, J) for J in (17, 64) for P in (1, 63, 64, 65, 255, 256, 257, 300)]
    for i, c in enumerate(sec.SINGLE):
        assert c[3] == sec.ROTS[i % 3] and c[4] == (3 if i % 2 else 0)
    assert [(c[0], c[1], c[2]) for c in sec.FRAMES] == (
        [(3, 257, J) for J in (1, 3, 16, 17, 42, 43, 49, 63, 64)] + [(2, P, J) for J in (17, 64) for P in (1, 63, 65, 256)] + [(16, 65, 64)])
    assert [(c[0], c[1]) for c in sec.ONE_HOT] == [(65, J) for J in (1, 2, 17, 33, 64)]
    assert [(c[0], c[1]) for c in sec.SCENE_AVATARS] == [(1, 1), (65, 17), (257, 64)]
    # every J-dependent path of the kernels is taken by both lists: float4 and scalar staging, 1..4 chunks, a padded last k-step,
    # dynamic LDS on either side of 64 KiB
    for Jl in ([c[1] for c in sec.SINGLE], [c[2] for c in sec.FRAMES]):
        assert {(J + 15) >> 4 for J in Jl} == {1, 2, 3, 4}
        assert any(J % 4 == 0 for J in Jl) and any(J % 4 for J in Jl) and any(J % 16 in (1, 2, 3) for J in Jl)
        assert any(22528 + 1024 * J <= 65536 for J in Jl) and any(22528 + 1024 * J > 65536 for J in Jl)
    assert 22528 + 1024 * 42 <= 65536 < 22528 + 1024 * 43 and 22528 + 1024 * 64 == 88064


def test_scenes_follow_the_recipe():
    s = sec.scene(257, 17, 1, "6d")
    assert s["xyz"].shape == (257, 3) and s["A"].shape == (17, 4, 4) and s["rot_in"].shape == (257, 6) and s["shs"].shape == (257, 16, 3)
    assert np.allclose(s["w"].sum(1), 1.0, atol=1e-6) and (s["w"] >= 0).all() and ((s["w"] > 0).sum(1) < 17).any()
    assert ((s["w"] > 0).sum(0) > 0).all()                                       # every joint carries weight (P >= J)
    R = s["A"][:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5 and np.array_equal(s["A"][:, 3], np.tile([0, 0, 0, 1], (17, 1)))
    cam = s["cam"]
    assert (cam["image_width"], cam["image_height"]) == (64, 48) and abs(math.tan(cam["fovx"] * 0.5) - 32 / 375) < 1e-6
    m = sec.scene(257, 17, 1, "mat")
    assert m["rot_in"].shape == (257, 3, 3) and np.array_equal(m["rot_in"], s["Rc"]) and np.array_equal(m["xyz"], s["xyz"])
    i = sec.scene(257, 17, 1, "iso")
    assert i["rot_in"] is None and np.array_equal(i["scales"][:, 0], i["scales"][:, 2])
    k = sec.scene(65, 17, 1, "6d", K=3)
    assert k["A"].shape == (3, 17, 4, 4) and k["transl"].shape == (3, 3) and k["dL"].shape == (3, 3, 48, 64)
    one = sec.scene(65, 17, 1, "6d")
    assert np.array_equal(k["A"][0], one["A"]) and np.array_equal(k["transl"][0], one["transl"]) and np.array_equal(k["w"], one["w"])
    assert np.abs(k["A"][1] - k["A"][0]).max() > 0.05 and np.abs(k["A"][2] - k["A"][1]).max() > 0.05
    assert np.abs(k["transl"][1] - k["transl"][0]).max() > 1e-3


def test_one_hot_rows_use_the_stated_joints():
    for P, J, seed in sec.ONE_HOT:
        s = sec.one_hot(P, J, seed)
        w = s["w"]
        assert ((w == 0) | (w == 1)).all() and (w.sum(1) == 1).all()
        used = set(np.nonzero(w.sum(0))[0].tolist())
        assert used == set(s["used"]) and {0, J - 1} <= used
        if J > 16:
            for c in range((J + 15) // 16):
                assert {16 * c, min(16 * c + 15, J - 1)} <= used, (J, c)
        if J >= 3:
            assert len(used) < J, J


def test_view_conditions():
    """Visible share, the borderline cap of _check_image (8 + 6e-4 pixels) and joint coverage, per posed frame."""
    bad = {label: b for label, s in _frames() for b in [view_failures(s)] if b}
    assert not bad, bad


def test_matrix_to_quaternion_keeps_its_branch():
    """fp64: the largest and second-largest candidate q_abs differ by >= 1e-3 for every Gaussian, so fp32 (errors ~1e-6 in the
    deformed rotation) picks the reference's branch."""
    gaps = {label: m2q_gap(s) for label, s in _frames()}
    bad = {k: v for k, v in gaps.items() if v < 1e-3}
    assert not bad, bad


def test_fp32_restatement_stays_within_a_quarter_of_the_gpu_bar():
    worst = max((headroom(s) + (label,) for label, s in _frames()))
    print(f"fp32 restatement vs fp64, worst ratio to the bar of (b): {worst[0]:.4f} ({worst[1]}, {worst[2]})")
    assert worst[0] <= 0.25, worst
