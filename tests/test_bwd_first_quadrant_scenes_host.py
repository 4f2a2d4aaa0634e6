"""The scenes of tests/test_gpu_bwd_first_quadrant.py against the scalar oracle alone (no GPU): each scene really contains the case
its GPU test is about -- otherwise a GPU case could lose its subject silently."""
import numpy as np

import test_gpu_bwd_first_quadrant as fq

RIGHT = [ty * fq.GX + fq.GX - 1 for ty in range(fq.GY)]
BOTTOM = [(fq.GY - 1) * fq.GX + tx for tx in range(fq.GX)]


def _census(o, tiles):
    """(first quadrant, reach) pairs of the tiles' list entries, and the number of entries with a skipped quadrant in front of their first."""
    pairs, skipped = set(), 0
    for t in tiles:
        geo, hit, maxq = fq.quadrant_census(o, t)
        if len(geo):
            first, reach = fq.first_and_reach(hit)
            pairs |= set(zip(first.tolist(), reach.tolist()))
            skipped += int(fq.skipped_in_front(geo, hit, maxq).sum())
    return pairs, skipped


def test_every_first_quadrant_occurs_with_every_reach():
    _, o, _, _ = fq.oracle_of("reach")
    pairs, skipped = _census(o, range(fq.GX * fq.GY))
    for q in range(4):
        for reach in range(1, 4 - q + 1):
            assert (q, reach) in pairs, (q, reach, sorted(pairs))
    assert (4, 0) in pairs, "no entry without a contribution"
    assert skipped >= len(fq.CLUSTERS)
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert tl.max() < 256, "one depth segment and live boxes of whole quadrants: the masks are the rectangles'"


def test_the_straddlers_skip_quadrant_0_and_assign_in_a_later_one():
    """Per cluster: the straddler reaches pixels of quadrant 0, lies in front of that quadrant's deepest contributor, none of the
    pixels it reaches there is live, and its first accumulating quadrant is 1 ("h") or 2 ("v")."""
    _, o, _, _ = fq.oracle_of("reach")
    for i, (tx, ty, orient) in enumerate(fq.CLUSTERS):
        tile = ty * fq.GX + tx
        geo, hit, maxq = fq.quadrant_census(o, tile)
        lo = int(o["ranges"][tile, 0])
        ids = o["point_list"][lo:lo + len(geo)].astype(int)
        e = int(np.nonzero(ids == fq.straddler_id(i))[0][0])
        first, _ = fq.first_and_reach(hit)
        want = 1 if orient == "h" else 2
        assert geo[e, 0] and not hit[e, 0] and e < maxq[0], (tx, ty, geo[e], hit[e], e, maxq)
        assert first[e] == want, (tx, ty, first[e])
        assert fq.skipped_in_front(geo, hit, maxq)[e]


def test_the_ragged_tiles_carry_both_forms_and_a_skipped_quadrant():
    """Right column and bottom row: entries whose first accumulating quadrant is not 0 (the assigning form behind the branch),
    entries accumulating in more than one quadrant (the adding form), and a quadrant skipped in front of the first."""
    _, o, _, _ = fq.oracle_of("reach")
    for name, tiles in (("right", RIGHT), ("bottom", BOTTOM)):
        pairs, skipped = _census(o, tiles)
        assert any(q in (1, 2, 3) for q, r in pairs), (name, sorted(pairs))
        assert any(q == 0 and r >= 2 for q, r in pairs), (name, sorted(pairs))
        assert skipped >= 1, name
    # the bottom row's quadrants 2 and 3 are outside the image: nothing accumulates there
    pairs, _ = _census(o, BOTTOM)
    assert all(q in (0, 1, 4) for q, _ in pairs), sorted(pairs)


def test_the_faint_entries_sit_directly_in_front_of_sums_1e12_times_larger():
    s, o, dL, g = fq.oracle_of("stale")
    for i, (tx, ty, q) in enumerate(fq.STALE):
        tile = ty * fq.GX + tx
        geo, hit, maxq = fq.quadrant_census(o, tile)
        lo = int(o["ranges"][tile, 0])
        ids = o["point_list"][lo:lo + len(geo)].astype(int)
        e = int(np.nonzero(ids == 2 * i)[0][0])
        assert e + 1 < 64 and ids[e + 1] == 2 * i + 1, (tx, ty, e, ids[:e + 2])          # one batch, the big entry filed just before
        assert hit[e].tolist() == [k == q for k in range(4)], (tx, ty, hit[e])
        assert hit[e + 1].all(), (tx, ty, hit[e + 1])
        # the faint Gaussian lies in this tile alone, so its gradient is this tile's record
        assert int(o["tiles_touched"][2 * i]) == 1
        for key in ("dL_dopacity", "dL_dcolor", "dL_dconic", "dL_dmean2D"):
            big, faint = np.abs(g[key][2 * i + 1]).max(), np.abs(g[key][2 * i]).max()
            assert faint > 0 and big / faint >= 1e11, (key, big, faint)
