"""The depth and alpha maps at crafted tile-list lengths on the internal boundaries of the path (tests/tools/fuzz_parity.py
check_aux; the colour path's twin is tests/test_gpu_fuzz.py): 256 = depth segment (the D checkpoint slot of SgAuxFwd::ckD, and the
segment a backward restarts from), 512 / 1024 = in-composite sort and, on a few-tile frame, the four-workgroup deep forward whose
split quadrants each carry a partial D, 4096 / 12 288 = bucket-sort limits, 20 000 = beyond a 16 384-key row (the long-rows promise
is refused).  Every case: the aux forward's binning, colour and radii are the plain forward's bits; the maps against
oracle/raster_aux.py; every gradient element under a loss on colour, depth and alpha; the direct-binning promise gives the same bits.

The 64x48 frame has few tiles (deep forward, sparse backward); the same tile on a 1600x1056 frame (6 600 tiles, > 4096 tile
counters) takes sg_render_fwd_aux_kernel and the dense backward.  Opacity regimes: crafted()'s own, "saturating" (pixels of the hot
tile terminate inside the list, at entries on both sides of segment boundaries: the checkpoint of a segment behind the
termination is never used) and "faint" (no pixel terminates: every segment is walked and restarted from its checkpoint)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [255, 256, 257, 511, 513, 1023, 1024, 1025, 4096, 4097, 12288, 12289, 20000]
MANY_LENGTHS = [257, 1025, 4097, 12289]


def _fp():
    from tests.tools import fuzz_parity
    return fuzz_parity


def _hot_tile_regime(o, regime):
    """The oracle's view of the hot tile (1,1): saturating -> some pixels terminate, faint -> none does."""
    fT = o["final_T"][16:32, 16:32]
    terminated = int((fT < 2e-4).sum())
    if regime == "saturating":
        assert terminated >= 10, terminated
    elif regime == "faint":
        assert terminated == 0 and fT.min() > 1e-4
    return terminated


@pytest.mark.parametrize("regime", [None, "saturating", "faint"])
@pytest.mark.parametrize("n", LENGTHS)
def test_aux_crafted_tile_list_lengths(n, regime):
    fp = _fp()
    s = fp.aux_regime(fp.crafted(n, n), n, regime, n)
    R, mx, o = fp.check_aux(s, f"aux crafted {n} {regime}")
    assert mx >= n and R >= n
    _hot_tile_regime(o, regime)


@pytest.mark.parametrize("seed", [1, 2])
def test_aux_clustered_depths(seed):
    """Equal and adjacent depth codes: ties in z inside one depth segment, and the bucket sort's every level."""
    fp = _fp()
    z = fp.clustered_depths(seed)
    R, mx, o = fp.check_aux(fp.crafted(z.size, 100 + seed, depths=z), f"aux clustered depths {seed}")
    assert mx >= z.size


@pytest.mark.parametrize("regime", ["saturating", "faint"])
@pytest.mark.parametrize("n", MANY_LENGTHS)
def test_aux_crafted_lengths_on_a_frame_of_many_tiles(n, regime):
    fp = _fp()
    W, H = 1600, 1056
    assert ((W + 15) // 16) * ((H + 15) // 16) > 4096
    s = fp.aux_regime(fp.crafted(n, n, W=W, H=H), n, regime, n)
    R, mx, o = fp.check_aux(s, f"aux crafted {n} {regime} {W}x{H}")
    assert mx >= n
    _hot_tile_regime(o, regime)
