"""The scenes of tests/test_gpu_fwd_tile_wave.py against the scalar oracle alone (no GPU): the hot tile's list has exactly the length the
case is about and its workgroup's other tiles their seven entries, the pixels within 2e-5 of a hard threshold -- excluded from the
image bar there -- are at most 0.1 % of the frame, and the two crafted saturation cases saturate where they say."""
import numpy as np

import test_gpu_fwd_tile_wave as tw


def test_scenes_are_what_the_gpu_cases_assume():
    seen = 0
    for name, s in tw.all_scenes():
        o = tw._oracle(s)
        tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
        assert tw.excluded_share(o) <= tw.EXCLUDED_MAX, (name, tw.excluded_share(o))
        assert (tl == 0).any(), name
        kind = name.split()[0]
        if kind in ("hot", "corner"):
            n = int(name.split()[1])
            tile = tw.HOT if kind == "hot" else tw.CORNER
            assert tl[tile] == n == tl.max(), (name, tl[tile], tl.max())
            others = [t for t in range(tile // 4 * 4, tile // 4 * 4 + 4) if t != tile and t < tw.T]
            assert all(tl[t] == tw.NEIGHBOUR_SPLATS for t in others), (name, [tl[t] for t in others])
        seen += 1
    assert seen == 2 * len(tw.LENGTHS) + 5


def test_the_saturation_cases_saturate_where_they_say():
    o = tw._oracle(tw.quadrant_scene())
    nc = o["n_contrib"][16:32, 16:32].reshape(2, 8, 2, 8).max(axis=(1, 3)).reshape(4)
    n = int(o["ranges"][tw.HOT, 1]) - int(o["ranges"][tw.HOT, 0])
    assert n > 256 and nc[0] <= tw.QUADRANT_BLOCKERS and min(nc[1:]) > 256, (n, nc)
    o = tw._oracle(tw.early_exit_scene())
    n = int(o["ranges"][tw.HOT, 1]) - int(o["ranges"][tw.HOT, 0])
    nc = o["n_contrib"][16:32, 16:32]
    assert n > tw.WAVE_SORT_MAX and 0 < nc.min() and nc.max() < 40, (n, nc.min(), nc.max())
