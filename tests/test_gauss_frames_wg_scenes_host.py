"""The scenes of tests/test_gpu_gauss_frames_wg.py against the scalar oracle alone (no GPU): the blind-wave scene really has a
workgroup's 64 Gaussians that one frame's camera sees none of while every other frame sees all of them, and the P-edge scenes
really give their first and last Gaussian a gradient -- otherwise a GPU case could lose its subject silently."""
import numpy as np
import pytest

import test_gpu_gauss_frames_wg as wg


def _radii(s, cams, D=3):
    from oracle import raster_oracle as ro
    views, projs, cps = cams
    return np.stack([ro.forward(s["means3D"], s["opacities"], views[f], projs[f], cps[f], wg.W, wg.H, s["tanfovx"], s["tanfovy"],
                                s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=D)["radii"]
                     for f in range(len(views))])


@pytest.mark.parametrize("blind", [0, 2])
def test_one_frame_sees_none_of_a_workgroups_gaussians_and_the_others_see_all(blind):
    s, xs = wg.blind_scene(blind)
    assert len(s["means3D"]) == wg.BLIND_P == 3 * 64 and (wg.BLIND_BLOCK.start, wg.BLIND_BLOCK.stop) == (64, 128)
    seen = _radii(s, wg.cameras_at(s, xs)) > 0
    assert len(seen) == 3
    assert not seen[blind, wg.BLIND_BLOCK].any()
    assert np.delete(seen, blind, 0)[:, wg.BLIND_BLOCK].all()
    # the blind frame is no empty frame: it sees Gaussians of both other workgroups, which the near cameras do not
    assert seen[blind, wg.ASIDE].all() and not np.delete(seen, blind, 0)[:, wg.ASIDE].any()
    assert seen[blind, :64].any() and seen[blind, 128:].any()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_the_edge_scenes_first_and_last_gaussian_are_seen(P):
    s = wg.head_scene(P)
    assert len(s["means3D"]) == P
    seen = _radii(s, wg.gf.cameras(s, 3)) > 0
    assert seen[:, 0].any() and seen[:, P - 1].any()


@pytest.mark.parametrize("K", [5, 9, 16])
def test_every_frame_of_the_long_launches_sees_something_and_visibility_is_mixed(K):
    s = wg.gf.scene(3, 16, wg.W, wg.H)
    seen = _radii(s, wg.gf.cameras(s, K)) > 0
    n = seen.sum(0)
    assert seen.any(1).all() and (n == K).any() and ((n > 0) & (n < K)).any()
