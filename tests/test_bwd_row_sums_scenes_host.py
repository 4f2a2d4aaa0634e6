"""The scene of tests/test_gpu_bwd_row_sums.py against the scalar oracle alone (no GPU): it really contains the cases its GPU tests
are about -- otherwise a GPU case could lose its subject silently."""
import numpy as np

import test_gpu_bwd_first_quadrant as fq
import test_gpu_bwd_row_sums as rsum

GX, GY = rsum.GX, rsum.GY


def _list(o, tx, ty):
    tile = ty * GX + tx
    lo, hi = int(o["ranges"][tile, 0]), int(o["ranges"][tile, 1])
    return tile, o["point_list"][lo:hi].astype(np.int64)


def test_one_work_item_per_tile_and_their_count_is_no_multiple_of_four():
    _, o, _, _ = rsum.oracle()
    tl = o["ranges"][:, 1].astype(int) - o["ranges"][:, 0]
    assert tl.max() <= 256, "a list longer than a depth segment: more than one work item per tile"
    assert (GX * GY) % 4 != 0


def test_the_stacks_have_exactly_their_lengths_and_every_entry_is_filed():
    """Lists of 64, 65, 128, 129 (right column: 64, bottom row: 65) entries in list order = id order, each Gaussian in that tile
    alone, each reaching a live pixel (its row of sums is filed)."""
    _, o, _, _ = rsum.oracle()
    _, s0, _ = rsum.layout()
    assert sorted(n for _, _, n, *_ in rsum.STACKS) == [64, 64, 65, 65, 128, 129]
    assert any(tx == GX - 1 for tx, *_ in rsum.STACKS) and any(ty == GY - 1 for _, ty, *_ in rsum.STACKS)
    for (tx, ty, n, *_), first in zip(rsum.STACKS, s0):
        tile, ids = _list(o, tx, ty)
        assert ids.tolist() == list(range(first, first + n)), (tx, ty, len(ids))
        assert (o["tiles_touched"][ids] == 1).all(), (tx, ty)
        _, hit, _ = fq.quadrant_census(o, tile)
        assert hit.any(1).all(), (tx, ty, np.nonzero(~hit.any(1))[0])


def test_neighbouring_entries_of_a_stack_differ_in_opacity_conic_and_gradient():
    s, o, _, g = rsum.oracle()
    for tx, ty, n, *_ in rsum.STACKS:
        tile, ids = _list(o, tx, ty)
        co = o["conic_opacity"][ids].astype(np.float64)
        op = co[:, 3]
        assert (np.abs(op[1:] - op[:-1]) >= 0.0089).all() and op.max() / op.min() > 5, (tx, ty)
        # strongly anisotropic, and another orientation than the neighbour's: some conic element differs by more than 1
        lam = np.array([np.linalg.eigvalsh(np.array([[a, b], [b, c]])) for a, b, c in co[:, :3]])
        assert (lam[:, 1] / lam[:, 0] > 5).all(), (tx, ty, (lam[:, 1] / lam[:, 0]).min())
        assert (np.abs(co[1:, :3] - co[:-1, :3]).max(1) > 1.0).all(), (tx, ty)
        assert rsum.neighbours_differ(o, g, tile) > 1.0, (tx, ty)


def test_filed_and_unfiled_entries_alternate_and_the_unfiled_ones_have_zero_gradients():
    """Both ALTERNATE tiles: 132 entries (two full batches and four more), behind the front entries strictly (unfiled, filed) x 60;
    the unfiled entries reach no live pixel ("hidden": they reach pixels, all terminated; "faint": they reach none), and the
    oracle's gradients of their Gaussians are zeros."""
    _, o, _, g = rsum.oracle()
    _, _, a0 = rsum.layout()
    for (tx, ty, kind), first in zip(rsum.ALTERNATE, a0):
        tile, ids = _list(o, tx, ty)
        n, front = rsum.ALT_LEN[kind], rsum.ALT_FRONT[kind]
        assert n > 128 and ids.tolist() == list(range(first, first + n)), (kind, len(ids))
        geo, hit, _ = fq.quadrant_census(o, tile)
        filed = hit.any(1)
        assert filed[:front].all(), kind
        assert filed[front:].tolist() == [False, True] * rsum.PAIRS, (kind, filed[front:])
        reached = geo.any(1)[front::2]
        assert reached.all() if kind == "hidden" else not reached.any(), kind
    ids = rsum.unfiled_ids()
    assert len(ids) == 2 * rsum.PAIRS
    for key in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drots", "dL_dsh"):
        assert not np.abs(g[key][ids]).any(), key
        assert np.abs(g[key]).max() > 0, key
