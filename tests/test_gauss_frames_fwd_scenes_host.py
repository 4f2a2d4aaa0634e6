"""The scenes of tests/test_gpu_gauss_frames_fwd.py against the scalar oracle alone (no GPU): per 64-Gaussian block and frame the
visible counts the GPU cases count on -- a block one frame sees none of while the others see all of it, a frame that sees nothing,
edge scenes whose first and last Gaussian have pairs, launches with mixed visibility -- the pair counts R of the capacity case
(exactly one frame above the capacity the GPU test picks), and the frames' regimes.  Otherwise a GPU case could lose its subject
silently."""
import numpy as np
import pytest

import test_gpu_gauss_frames_fwd as ff
from sings_amd import _lib
from sings_amd import work_order as wo


def _forwards(s, cams, size, D=3):
    from oracle import raster_oracle as ro
    views, projs, cps = cams
    return [ro.forward(s["means3D"], s["opacities"], views[f], projs[f], cps[f], *size, s["tanfovx"], s["tanfovy"], s["bg"],
                       scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=D, want_margin=False)
            for f in range(len(views))]


def _block_counts(fwd):
    """[K, blocks of 64]: Gaussians of the block that the frame sees"""
    seen = np.stack([o["radii"] > 0 for o in fwd])
    pad = (-seen.shape[1]) % 64
    return np.pad(seen, ((0, 0), (0, pad))).reshape(len(fwd), -1, 64).sum(2), seen


def test_the_frames_are_in_the_regimes_the_cases_are_named_for():
    assert wo.order_applies(*ff.MANY, _lib.FLAG_SHORT_LISTS)
    assert not wo.order_applies(*ff.SMALL, _lib.FLAG_SHORT_LISTS) and not wo.order_applies(*ff.RAGGED_SMALL, _lib.FLAG_SHORT_LISTS)
    assert ff.MANY[0] % 16 and ff.MANY[1] % 16 and ff.RAGGED_SMALL[0] % 16 and ff.RAGGED_SMALL[1] % 16
    assert ff.gf.P % 64 and ff.gf.P % 256


@pytest.mark.parametrize("size", ff.SIZES)
@pytest.mark.parametrize("blind", [0, 2])
def test_one_frame_sees_none_of_a_workgroups_gaussians_and_the_others_see_all(blind, size):
    s, xs = ff.blind_scene(blind, size)
    assert len(s["means3D"]) == ff.BLIND_P == 3 * 64 and (ff.BLIND_BLOCK.start, ff.BLIND_BLOCK.stop) == (64, 128)
    counts, seen = _block_counts(_forwards(s, ff.cameras_at(s, xs), size))
    assert counts.shape == (3, 3)
    assert counts[blind, 1] == 0 and (np.delete(counts, blind, 0)[:, 1] == 64).all()
    # the blind frame is no empty frame: it sees Gaussians of both other workgroups, which the near cameras do not
    assert seen[blind, ff.ASIDE].all() and not np.delete(seen, blind, 0)[:, ff.ASIDE].any()
    assert counts[blind, 0] > 0 and counts[blind, 2] > 0


@pytest.mark.parametrize("size", ff.SIZES)
def test_one_frame_sees_nothing_and_the_others_something_in_every_block(size):
    s = ff.gf.scene(3, 16, *size)
    fwd = _forwards(s, ff.cameras_at(s, ff.EMPTY_XS), size)
    counts, _ = _block_counts(fwd)
    assert not counts[1].any() and fwd[1]["R"] == 0
    assert (counts[0] > 0).all() and (counts[2] > 0).all()


@pytest.mark.parametrize("size", ff.SIZES)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_the_edge_scenes_first_and_last_gaussian_are_seen(P, size):
    s = ff.head_scene(P, size)
    assert len(s["means3D"]) == P
    _, seen = _block_counts(_forwards(s, ff.cameras_at(s, ff.gf.STEP * np.arange(3)), size))
    assert seen[:, 0].any() and seen[:, P - 1].any()


@pytest.mark.parametrize("K,size", [(K, z) for K in (2, 3, 4, 5, 8, 9, 16) for z in ff.SIZES] + [(8, ff.RAGGED_SMALL)])
def test_every_frame_of_a_launch_sees_something_and_visibility_is_mixed(K, size):
    s = ff.gf.scene(3, 16, *size)
    fwd = _forwards(s, ff.cameras_at(s, ff.gf.STEP * np.arange(K)), size)
    counts, seen = _block_counts(fwd)
    n = seen.sum(0)
    assert seen.any(1).all() and (n == K).any() and ((n > 0) & (n < K)).any()
    assert (counts < 64).any() and (counts > 0).any()
    # no list longer than a row: the short-list hint of the GPU cases is true, and the pairs fit their capacity
    for o in fwd:
        assert int((o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]).max()) <= ff.KEY_PITCH and o["R"] <= 48 * ff.gf.P + 1024
    # the Gaussians the order `beyond` drops are seen by frames 0 .. 2
    assert seen[:min(K, 3)][:, list(ff.DROPPED)].all()


@pytest.mark.parametrize("size", ff.SIZES)
def test_the_capacity_case_overflows_exactly_one_frame(size):
    s = ff.gf.scene(3, 16, *size)
    R = [o["R"] for o in _forwards(s, ff.over_cameras(s), size)]
    most = max(r for f, r in enumerate(R) if f != ff.OVER_FRAME)
    assert most * 1.05 < R[ff.OVER_FRAME], R
    cap = (most + R[ff.OVER_FRAME]) // 2                                    # what the GPU test picks
    assert [r > cap for r in R] == [f == ff.OVER_FRAME for f in range(ff.OVER_K)] and min(R) > 0


def test_the_orders_are_permutations_but_for_the_dropped_entries():
    P = ff.gf.P
    od = ff.orders(P)
    for name in ("identity", "reversed", "random"):
        assert np.array_equal(np.sort(od[name]), np.arange(P)), name
    b = od["beyond"].astype(np.int64) & 0xffffffff
    assert (b >= P).sum() == 2 and sorted(set(range(P)) - set(b.tolist())) == sorted(ff.DROPPED)
