"""The scene of tests/test_gpu_gauss_frames_bwd.py against the scalar oracle alone (no GPU): it really contains the cases its GPU
tests are about -- mixed visibility over the frames, colours clamped in some frames only, a -0 in frame 0's gradient --
otherwise a GPU case could lose its subject silently."""
import numpy as np
import pytest

import test_gpu_gauss_frames_bwd as gf

SIZES = [gf.SMALL, gf.RAGGED]


def _vis(K, D, M, size):
    _, _, fwd, _, grads, _, _ = gf.oracle(K, D, M, *size)
    return np.stack([o["radii"] > 0 for o in fwd]), np.stack([o["clamped"].astype(bool) for o in fwd]), grads


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("K", [2, 3, 8])
def test_the_crafted_gaussians_are_seen_by_the_frames_they_are_meant_for(K, size):
    vis, _, _ = _vis(K, 3, 16, size)
    assert vis[0, gf.ONLY0].all() and not vis[1:, gf.ONLY0].any()                 # visible in frame 0 only
    assert not vis[0, gf.LATER].any() and vis[1, gf.LATER].all()                  # invisible in frame 0, visible later
    assert vis[:2, gf.FLIP].all() and vis[:3, gf.MINUS0].all()
    # and the cloud itself mixes: Gaussians seen by every frame, by none, and by some
    n = vis.sum(0)
    assert (n == K).sum() > 300 and (n == 0).sum() > 10 and ((n > 0) & (n < K)).sum() > 10
    assert gf.P % 64 != 0 and gf.P % 256 != 0 and (gf.P + 255) // 256 > 1 and 256 * ((gf.P + 255) // 256) - gf.P >= 64


@pytest.mark.parametrize("D,M", [(3, 16), (2, 16), (1, 16), (2, 9), (1, 4)])
def test_colours_are_clamped_in_one_frame_and_not_in_another(D, M):
    vis, clamped, grads = _vis(3, D, M, gf.SMALL)
    c = clamped[:, gf.FLIP]
    assert not c[0].any()                                                         # camera 0 is on their unclamped side
    assert c[1][:, [0, 2]].all() and not c[1][:, 1].any()                         # camera 1 has passed them: channels 0 and 2
    # the clamped channels of frame 1 carry no SH gradient there, the open one does
    sh1 = grads[1]["dL_dsh"][gf.FLIP]
    assert not sh1[:, :, [0, 2]].any() and np.abs(sh1[:, :(D + 1) ** 2, 1]).min(1).max() > 0


def test_frame_zero_leaves_a_minus_zero():
    """MINUS0: every channel clamped in every frame, and every frame sees them -- dL/dsh = basis * (+0): row 1 (basis -C1 y,
    y > 0) is -0, row 0 +0; with a non-zero colour gradient underneath (the clamp is what zeroes it).  The first three of ONLY0
    are clamped the same way (the case of the module docstring's exception)."""
    vis, clamped, grads = _vis(3, 3, 16, gf.SMALL)
    assert clamped[:, gf.MINUS0].all() and vis[:, gf.MINUS0].all() and clamped[0, gf.ONLY0[:3]].all()
    s = gf.scene(3, 16, *gf.SMALL)
    assert (s["means3D"][gf.MINUS0, 1] > 0).all()
    for f in range(3):
        assert np.abs(grads[f]["dL_dcolor"][gf.MINUS0]).min() > 0
        shf = grads[f]["dL_dsh"][gf.MINUS0].astype(np.float32)
        assert not shf.any()
        assert np.signbit(shf[:, 1]).all() and not np.signbit(shf[:, 0]).any()


def test_the_closer_camera_sees_fewer_pairs():
    _, _, fwd, _, _, _, _ = gf.oracle(3, 3, 16, *gf.SMALL, False, False, 1)
    R = [o["R"] for o in fwd]
    assert R[1] * 1.05 < min(R[0], R[2]), R
