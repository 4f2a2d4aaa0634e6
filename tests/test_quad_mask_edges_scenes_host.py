"""The scenes of tests/test_gpu_quad_mask_edges.py against the scalar oracle alone (no GPU): they hold the cases that file is about.
Every crafted splat's accepted pixels in the quadrant it enters are exactly the listed corner pixel, or pixels of the listed column or row only; the
hot tile's list has the length the case names and the crafted splats sit in the batch they should; the ragged tiles' boxes are
clipped (and the bottom tile's lower quadrants empty); the long list's live boxes are strict sub-rectangles at entry 256 and
entries blend behind it; a quadrant's deepest contributor lies inside a batch with mask bits behind it.  And in every one of these
tiles, walked in fp32 as the dense forward walks it (tests/quad_mask_case.py), no (entry, quadrant) that blends a pixel lacks its
bit in the facing-edges form of the quadrant test."""
import numpy as np

import quad_mask_case as qm
import test_gpu_fwd_tile_wave as tw
import test_gpu_quad_mask_edges as qe


def _accepted(o, g, tile, q):
    """Pixels (x, y) of quadrant q of `tile`, inside the image, that accept Gaussian g."""
    X0, Y0 = (tile % qe.GX) * 16 + 8 * (q & 1), (tile // qe.GX) * 16 + 8 * (q >> 1)
    out = []
    one = lambda v: np.array([v], np.float32)
    ax, ay = o["xy"][g]; A, B, C, op = o["conic_opacity"][g]
    for y in range(Y0, min(Y0 + 8, qe.H)):
        for x in range(X0, min(X0 + 8, qe.W)):
            if qm.accepts(one(ax), one(ay), one(A), one(B), one(C), one(op), one(x), one(y))[0]:
                out.append((x, y))
    return sorted(out)


def _enters_as_listed(got, want):
    """`got`: the accepted pixels; `want`: a corner pixel (x, y), ("x", column) or ("y", row)."""
    if want[0] == "x":
        return len(got) > 0 and all(x == want[1] for x, _ in got)
    if want[0] == "y":
        return len(got) > 0 and all(y == want[1] for _, y in got)
    return got == [want]


def _no_blended_pair_dropped(w, name):
    assert not (w["blended"] & ~w["masks_new"]).any(), name
    assert not (w["blended"] & ~w["masks_old"]).any(), name


def test_the_crafted_splats_enter_their_quadrants_where_they_say():
    for n, front in qe.LENGTHS:
        name = f"edges {n} {front}"
        s = qe.edge_scene(n, front)
        o = tw._oracle(s)
        assert tw.excluded_share(o) <= tw.EXCLUDED_MAX, name
        tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
        assert tl[qe.HOT] == n == tl.max(), (name, tl[qe.HOT], tl.max())
        # the crafted splats are Gaussians 0..7 (hot tile) and 8..11 (ragged tiles)
        for g, (what, p, _, q, pixels) in enumerate(qe.HOT_SPOTS):
            assert np.allclose(o["xy"][g], p, atol=2e-3), (what, o["xy"][g])
            assert _enters_as_listed(_accepted(o, g, qe.HOT, q), pixels), (name, what, _accepted(o, g, qe.HOT, q))
        w = qm.walk_tile(o, qe.HOT)
        _no_blended_pair_dropped(w, name)
        pos = {int(g): i for i, g in enumerate(w["ids"])}
        for g, (what, _, _, q, pixels) in enumerate(qe.HOT_SPOTS):
            i = pos[g]
            assert (i < 8) if front else (i >= n - 8), (name, what, i)
            assert w["blended"][i, q] and w["masks_new"][i, q], (name, what)
            # means inside one range of the entered quadrant's box and outside the other (the lines), outside both (the corners)
            x0, x1, y0, y1 = w["boxes"][i, q]
            mx, my = o["xy"][g][0] - 16, o["xy"][g][1] - 16
            inx, iny = x0 <= mx <= x1, y0 <= my <= y1
            assert (inx, iny) == {"corner": (False, False), "column": (False, True), "row": (True, False)}[what.split()[0]], (what, mx, my)
        if not front:
            assert (n - 1) // 64 * 64 <= min(pos[g] for g in range(8)) or n - 8 < (n - 1) // 64 * 64 + 1     # (the last batch holds them, or its only entry is one)
        for j, (what, tile, p, _, q, pixels) in enumerate(qe.RAGGED):
            g = 8 + j
            assert np.allclose(o["xy"][g], p, atol=2e-3), (what, o["xy"][g])
            wt = qm.walk_tile(o, tile)
            _no_blended_pair_dropped(wt, (name, what))
            i = int(np.flatnonzero(wt["ids"] == g)[0])
            assert wt["blended"][i, q] and wt["masks_new"][i, q], (name, what)
            box = wt["boxes"][i]
            if tile == qe.RIGHT:
                assert tuple(box[1]) == (8.0, 9.0, 0.0, 7.0) and tuple(box[3]) == (8.0, 9.0, 8.0, 15.0), box
            else:
                assert tuple(box[0]) == (0.0, 7.0, 0.0, 5.0) and box[2][0] > box[2][1] and box[3][0] > box[3][1], box
                assert not wt["masks_new"][:, 2:].any()
            if pixels is None:
                x0, x1, y0, y1 = box[q]
                assert x0 <= p[0] - (tile % qe.GX) * 16 <= x1 and y0 <= p[1] - (tile // qe.GX) * 16 <= y1
            else:
                assert _enters_as_listed(_accepted(o, g, tile, q), pixels), (name, what, _accepted(o, g, tile, q))
                outside = p[0] > qe.W - 1 or p[1] > qe.H - 1
                assert outside == ("outside" in what), what


def test_the_live_boxes_shrink_behind_the_opaque_front():
    o = tw._oracle(qe.shrink_scene())
    assert tw.excluded_share(o) <= tw.EXCLUDED_MAX
    w = qm.walk_tile(o, qe.HOT)
    _no_blended_pair_dropped(w, "shrink")
    assert w["n"] > 256
    first, later = w["boxes"][0], w["boxes"][256]
    shrunk = [q for q in range(4) if later[q][0] <= later[q][1] and tuple(later[q]) != tuple(first[q])]
    print("boxes at entry 256:", later.tolist())
    assert shrunk, later
    # behind entry 256 entries blend in a shrunk quadrant, and the shrunk box clears bits the whole quadrant would have kept
    assert any(w["blended"][256:, q].any() for q in shrunk)
    whole_w = qm.walk_tile(o, qe.HOT, refresh=1 << 30)                 # (the boxes never refreshed: the whole quadrants throughout)
    assert any((whole_w["masks_new"][256:, q] & ~w["masks_new"][256:, q]).any() for q in shrunk)


def test_a_deepest_contributor_inside_a_batch_has_mask_bits_behind_it():
    o = tw._oracle(tw.quadrant_scene())
    w = qm.walk_tile(o, qe.HOT)
    _no_blended_pair_dropped(w, "deepest")
    found = []
    for q in range(4):
        d = int(w["deepest"][q])
        end = min((d + 63) // 64 * 64, w["n"])
        if d % 64 and w["masks_new"][d:end, q].any():
            found.append((q, d, int(w["masks_new"][d:end, q].sum())))
    print("(quadrant, deepest contributor, bits behind it in its batch):", found)
    assert found
