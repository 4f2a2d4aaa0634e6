"""Host tests of the k-NN grid sizing (sings_amd/csrc/sg_knn_grid.h).  The function under test is the product's own, the one
thread 0 of sg_grid_setup2_kernel runs, compiled for the CPU (oracle/knn_grid_host.c) -- not a Python copy.  For every finite
box and every N >= 1, at both levels:  1 <= ncells <= max_cells (the workspace holds max_cells counters per level: one
cell more and the build kernels write outside their arrays), every dim >= 1, h finite and positive, and the stored dims are
those of the stored h.  Where the loop this function replaced stayed within max_cells the result is the same bit for bit,
so the grids of every cloud that worked before -- the avatar and the benchmark among them -- are unchanged."""
import numpy as np
import pytest

import knn_case
from oracle import knn_grid

NS = (1, 2, 5, 9, 17, 64, 362, 1000, 4000, 4600, 10 ** 4, 150000, 500000, 2 ** 21, 2 ** 23)
F = np.float32


def _named_boxes():
    """(label, lo, hi) of the degenerate shapes; each is sized for every N of NS at both levels."""
    out = [("square sheet, z constant", (0, 0, 0), (1, 1, 0)), ("0.6 x 1.8 sheet, z constant", (0, 0, 0), (0.6, 1.8, 0))]
    for f in range(3):
        for const in (0.0, 0.37, -5.0):
            lo = np.zeros(3); hi = np.ones(3); lo[f] = hi[f] = const
            out.append((f"sheet flat in {'xyz'[f]} at {const:g}", lo, hi))
            hi2 = np.array([0.6, 1.8, 0.3]); lo2 = np.zeros(3); lo2[f] = hi2[f] = const
            out.append((f"body sheet flat in {'xyz'[f]} at {const:g}", lo2, hi2))
    for rel in (1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 1e-1):
        for f in range(3):
            hi = np.array([1.8, 1.8, 1.8]); hi[f] = 1.8 * rel
            out.append((f"slab {rel:g} thin in {'xyz'[f]}", (0, 0, 0), hi))
            hi = np.array([0.6, 1.8, 1.0]); hi[f] = 1.8 * rel
            out.append((f"body slab {rel:g} thin in {'xyz'[f]}", (-0.3, -0.9, 0), hi + np.array([-0.3, -0.9, 0])))
    for f in range(3):
        hi = np.zeros(3); hi[f] = 1.0
        out.append((f"line along {'xyz'[f]}", (0, 0, 0), hi))
    out.append(("diagonal line", (0, 0, 0), (0.6, 1.8, 0.3)))       # (a line's box is the box of its end points)
    out.append(("single point at the origin", (0, 0, 0), (0, 0, 0)))
    out.append(("single point", (0.25, -1.5, 3.0), (0.25, -1.5, 3.0)))
    # far outside what a cloud in metres has: the volume over- or underflows in fp32
    for s in (1e-30, 1e-20, 1e-13, 1e10, 1e25, 3e38):
        out.append((f"cube of edge {s:g}", (0, 0, 0), (s, s, s)))
        out.append((f"sheet of edge {s:g}", (0, 0, 0), (s, s, 0)))
    out.append(("the whole fp32 range", (-3.4e38,) * 3, (3.4e38,) * 3))
    return [(n, np.asarray(a, F), np.asarray(b, F)) for n, a, b in out]


def _sweep(n=120000, seed=20240607):
    """Boxes with one axis of extent 1 and the others log-uniform in 1e-5 .. 1, 30 % with one axis zeroed, half of them away
    from the origin; N log-uniform in 1 .. 3e6."""
    rs = np.random.RandomState(seed)
    ext = 10.0 ** rs.uniform(-5, 0, (n, 3))
    ext[np.arange(n), rs.randint(0, 3, n)] = 1.0
    zero = rs.uniform(size=n) < 0.3
    ext[zero, rs.randint(0, 3, n)[zero]] = 0.0
    lo = np.where(rs.uniform(size=(n, 1)) < 0.5, 0.0, rs.uniform(-2, 2, (n, 3))).astype(F)
    hi = (lo + ext.astype(F)).astype(F)
    N = np.floor(10.0 ** rs.uniform(0, np.log10(3e6), n)).astype(np.int64)
    return lo, hi, N


def _max_cells(N, fine):
    return np.array([knn_grid.max_cells(int(n), fine) for n in np.atleast_1d(N)], np.int32)


def _valid(g, mc):
    """The guarantee, from the integers actually stored."""
    d = g["dim"].astype(np.int64)
    prod = d[:, 0] * d[:, 1] * d[:, 2]
    return ((d >= 1).all(1) & (prod >= 1) & (prod <= mc) & (g["ncells"].astype(np.int64) == prod) &
            np.isfinite(g["h"]) & (g["h"] > 0) & np.isfinite(g["inv_h"]) & (g["inv_h"] > 0))


def _dims_of_h(lo, hi, h):
    """dims that belong to h: (int)(ext / h) + 1 of the extents clamped to 1e-3 of the largest, in fp32 as the function does."""
    with np.errstate(over="ignore"):
        ext = (hi - lo).astype(F)                       # (the boxes beyond the fp32 range of a volume are not compared)
    emax = ext.max(1)
    emax = np.where(emax > 0, emax, F(1.0)).astype(F)
    ext = np.maximum(ext, (F(1e-3) * emax)[:, None]).astype(F)
    with np.errstate(all="ignore"):
        return (ext / h[:, None].astype(F)).astype(F).astype(np.int64) + 1


def _report(lo, hi, N, mc, g, bad):
    i = np.flatnonzero(bad)
    worst = i[np.argmax(g["ncells"][i].astype(np.float64) / mc[i])]
    return (f"{len(i)} of {len(bad)} boxes break the guarantee; worst: box {lo[worst]} .. {hi[worst]}, N {N[worst]}: dims "
            f"{g['dim'][worst]}, ncells {g['ncells'][worst]}, max_cells {mc[worst]}, h {g['h'][worst]}")


@pytest.mark.parametrize("fine", (0, 1))
def test_named_degenerate_boxes_fit_at_every_n(fine):
    boxes = _named_boxes()
    lo = np.repeat(np.stack([b[1] for b in boxes]), len(NS), 0); hi = np.repeat(np.stack([b[2] for b in boxes]), len(NS), 0)
    N = np.tile(np.array(NS, np.int64), len(boxes))
    mc = _max_cells(N, fine)
    assert mc.max() == (1 << 25 if fine else 1 << 23) and mc.min() == 4096          # both ends of the budget are reached
    g = knn_grid.size_batch(lo, hi, mc)
    bad = ~_valid(g, mc)
    assert not bad.any(), _report(lo, hi, N, mc, g, bad)
    assert (g["lo"] == lo).all()
    ordinary = np.array(["edge" not in b[0] and "whole" not in b[0] for b in boxes]).repeat(len(NS))
    assert (g["dim"][ordinary] == _dims_of_h(lo, hi, g["h"])[ordinary]).all()


TABLE = (  # the flat clouds on which the defect was found: (extent, N, level) with the grid the previous loop stored
    ((1, 1, 0), 1, 0, (83, 83, 1), 4096), ((1, 1, 0), 1000, 0, (83, 83, 1), 4096), ((1, 1, 0), 362, 1, (117, 117, 1), 11584),
    ((1, 1, 0), 2000, 0, (103, 103, 1), 8000), ((1, 1, 0), 4000, 0, (130, 130, 1), 16000),
    ((0.6, 1.8, 0), 1, 0, (40, 119, 1), 4096), ((0.6, 1.8, 0), 1000, 0, (40, 119, 1), 4096))


@pytest.mark.parametrize("ext,N,fine,dims_before,mc", TABLE)
def test_sheets_that_overflowed_before(ext, N, fine, dims_before, mc):
    """The flat clouds whose grids had more cells than the workspace holds (dims_before: what the previous loop stored, checked
    here so that the table stays a record of the defect) fit now."""
    assert knn_grid.max_cells(N, fine) == mc
    lo, hi = np.zeros((1, 3), F), np.asarray([ext], F)
    before = knn_grid.size_batch(lo, hi, [mc], previous=True)[0]
    assert tuple(before["dim"]) == dims_before and before["ncells"] > mc
    g = knn_grid.size_batch(lo, hi, [mc])
    assert _valid(g, np.array([mc]))[0], g
    assert (g["dim"] == _dims_of_h(lo, hi, g["h"])).all()
    assert g["h"][0] >= before["h"]                     # (coarser, never finer, than the grid that did not fit)


@pytest.mark.parametrize("fine", (0, 1))
def test_random_sweep_fits_and_keeps_every_grid_that_fitted(fine):
    lo, hi, N = _sweep()
    mc = _max_cells(N, fine)
    g = knn_grid.size_batch(lo, hi, mc)
    bad = ~_valid(g, mc)
    assert not bad.any(), _report(lo, hi, N, mc, g, bad)
    assert (g["dim"] == _dims_of_h(lo, hi, g["h"])).all()
    # parity: wherever the previous loop stayed within max_cells, the same bits
    p = knn_grid.size_batch(lo, hi, mc, previous=True)
    fitted = _valid(p, mc)
    assert fitted.sum() > 0.9 * len(N) and (~fitted).sum() > 1000                   # the sweep holds both kinds
    for k in ("lo", "inv_h", "h", "dim", "ncells"):
        assert (g[k][fitted].view(np.int32) == p[k][fitted].view(np.int32)).all(), k
    # the same over the named boxes of ordinary size
    boxes = [b for b in _named_boxes() if "edge" not in b[0] and "whole" not in b[0]]
    lo = np.repeat(np.stack([b[1] for b in boxes]), len(NS), 0); hi = np.repeat(np.stack([b[2] for b in boxes]), len(NS), 0)
    mc = _max_cells(np.tile(np.array(NS, np.int64), len(boxes)), fine)
    g, p = knn_grid.size_batch(lo, hi, mc), knn_grid.size_batch(lo, hi, mc, previous=True)
    fitted = _valid(p, mc)
    assert fitted.any() and not fitted.all()
    assert (g[fitted].view(np.int32) == p[fitted].view(np.int32)).all()


# h (as fp32 bits) and dims of the two full-size clouds, recorded from the sizing loop as it was before the fit was guaranteed
# (moved into the header word for word, run on the CPU): the grids of the measured workloads must not move
RECORDED = {
    "avatar": dict(coarse=(0x3C827058, (120, 118, 32)), fine=(0x3C027058, (240, 236, 64))),
    "cfg5": dict(coarse=(0x3DADE372, (108, 108, 130)), fine=(0x3D2DE372, (216, 216, 260))),
}


@pytest.mark.parametrize("which", ("avatar", "cfg5"))
def test_full_size_grids_are_the_recorded_ones(which):
    from sings_amd.scene import avatar_scene, synthetic_scene
    xyz = avatar_scene(N=150000, J=52)["xyz_canon"] if which == "avatar" else synthetic_scene(500000, 2048, 2048, 3, 5)["means3D"]
    gc, gf = knn_grid.grids_of(xyz)
    for g, key in ((gc, "coarse"), (gf, "fine")):
        bits, dims = RECORDED[which][key]
        assert (int(g["h"].view(np.uint32)), tuple(int(d) for d in g["dim"])) == (bits, dims), (which, key, float(g["h"]))
        assert int(g["ncells"]) == dims[0] * dims[1] * dims[2] <= knn_grid.max_cells(len(xyz), key == "fine")


def test_cloud_builders():
    """The clouds of the GPU test are what their names say."""
    for name in knn_case.CLOUDS:
        a = knn_case.cloud(name)
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3 and np.isfinite(a).all() and len(a) <= 5000, name
    for n in knn_case.SHEET_N:
        for f in range(3):
            for c in (0.0, 0.37):
                a = knn_case.cloud(f"sheet-N{n}-flat{'xyz'[f]}-at{c:g}")
                ext = a.max(0) - a.min(0)
                assert len(a) == n and ext[f] == 0 and (a[:, f] == np.float32(c)).all() and (np.delete(ext, f) > 0.5).all()
    for r in (1e-3, 3e-3):
        ext = np.ptp(knn_case.cloud(f"slab-{r:g}"), 0)
        assert 0.9 * r < ext[2] / ext[1] < 1.01 * r
    for name, k in (("line-x", 1), ("line-z", 1), ("line-diag", 3)):
        a = knn_case.cloud(name).astype(np.float64)
        assert np.linalg.matrix_rank(a, tol=1e-6) == 1 and (np.ptp(a, 0) > 0).sum() == k
    for n in (9, 300, 5000):
        a = knn_case.cloud(f"coincident-N{n}")
        assert len(a) == n and (a == a[0]).all()
        assert (knn_case.brute_force(f"coincident-N{n}", 9) == 0.0).all()
    assert n > knn_case.SG_KNN_DENSE
    a = knn_case.cloud("two-clusters")
    assert len(a) == 80 and len(np.unique(a, axis=0)) == 2 and np.abs(a[0] - a[40]).sum() == 1.0
    assert (knn_case.brute_force("two-clusters", 17) == 0.0).all()
    for name in ("lattice-origin", "lattice-far"):
        a = knn_case.cloud(name)
        assert len(a) == 4096
        v = knn_case.nearest(name)
        assert (v[:, 1] == 2.0 ** -4).all()                       # exact, also far from the origin
        assert ((v[:, 8] == v[:, 9]).mean() > 0.5)                # the 9th distance is tied for most points
    assert np.array_equal(knn_case.nearest("lattice-origin"), knn_case.nearest("lattice-far"))


def test_threshold_clusters_sit_on_both_sides_of_the_dense_switch():
    xyz, s16, s17 = knn_case.threshold_cloud()
    cnt = knn_case.coarse_cell_counts(xyz)
    assert (cnt[s16] == knn_case.SG_KNN_DENSE).all() and (cnt[s17] == knn_case.SG_KNN_DENSE + 1).all()
    assert cnt[:2000].max() <= knn_case.SG_KNN_DENSE              # the sparse part never takes the fine grid
    # each cluster sits in the middle of its cell: a last-place difference of the device's cbrtf does not move a point across
    gc, _ = knn_grid.grids_of(xyz)
    frac = ((xyz[2000:] - gc["lo"]) * gc["inv_h"]) % 1.0
    assert (np.abs(frac - 0.5) < 0.1).all()
