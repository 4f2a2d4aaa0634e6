"""The k-NN search (knn_mean_edge, GaussiansEdgeLoss; kernels in sings_amd/csrc/sg_knn.hip) on clouds that are flat, thin,
colinear, coincident, barely larger than K, on cell faces or at the coarse / fine threshold (tests/knn_case.py), against fp64
brute force.  Bound: the one of test_gpu_reg.py::test_knn_exact_vs_brute_force, rtol 3e-6 + atol 1e-9 -- the SET of the K
nearest distances is exact, fp32 squares, sums and square roots differ from fp64 by a few ulp -- and exactly 0.0 where all
the distances are zero.  No case is skipped or filtered.  The worst difference of every case is printed before the assertion
(pytest -s)."""
import numpy as np
import pytest
import torch

import knn_case

pytestmark = pytest.mark.gpu
RTOL, ATOL = 3e-6, 1e-9


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _close(a, b, rtol=1e-5, atol_scale=5e-6):
    """test_gpu_reg.py's bound for gradients: 1e-5 relative + 5e-6 of the gradient's scale."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b)
    assert (err <= rtol * np.abs(b) + atol_scale * scale).all(), (err.max(), scale)


def _check(name, K):
    from sings_amd.regularizers import knn_mean_edge
    ref = knn_case.brute_force(name, K)
    got = knn_mean_edge(knn_case.tensor(name).to(_dev()), K=K).cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref > 0, np.abs(got - ref) / ref, np.abs(got - ref))
    print(f"knn {name} K={K}: worst relative difference {np.nanmax(rel):.3e} (absolute where the reference is 0)")
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    if (knn_case.nearest(name)[:, :K] == 0.0).all():
        assert (got == 0.0).all()
    return got


SHEETS = [(n, k) for n in knn_case.CLOUDS if n.startswith("sheet-") for k in (5, 9, 17) if int(n.split("-")[1][1:]) >= k]


@pytest.mark.parametrize("name,K", SHEETS)
def test_sheets(name, K):
    """Flat in x, in y and in z (the query deals (y, z) rows to lanes and runs along x), at 0 and away from it; the sizes
    include those whose grids had more cells than the workspace (N <= 1 000 coarse, 362 fine, 4 000 coarse)."""
    _check(name, K)


@pytest.mark.parametrize("K", (5, 9, 17))
@pytest.mark.parametrize("name", ("slab-0.001", "slab-0.003"))
def test_slabs(name, K):
    _check(name, K)


@pytest.mark.parametrize("K", (5, 9, 17))
@pytest.mark.parametrize("name", ("line-x", "line-z", "line-diag"))
def test_lines(name, K):
    """The diagonal line leaves almost every cell empty: many rings per point."""
    _check(name, K)


@pytest.mark.parametrize("name,K", [("coincident-N9", 5), ("coincident-N9", 9), ("coincident-N300", 9), ("coincident-N300", 17),
                                    ("coincident-N5000", 5), ("coincident-N5000", 9), ("coincident-N5000", 17),
                                    ("two-clusters", 5), ("two-clusters", 9), ("two-clusters", 17)])
def test_coincident_points_give_exactly_zero(name, K):
    """All extents zero (the sizing's emax == 0 branch), every point in one cell, more than SG_KNN_DENSE of them."""
    got = _check(name, K)
    assert (got == 0.0).all()


@pytest.mark.parametrize("K", (5, 9, 17))
@pytest.mark.parametrize("extra", (0, 1))
def test_n_equal_k_and_k_plus_one(K, extra):
    """Every point's neighbours are all the other points (but one): the search covers the whole grid before it ends."""
    _check(f"tiny-N{K + extra}", K)


@pytest.mark.parametrize("K", (5, 9, 17))
@pytest.mark.parametrize("name", ("lattice-origin", "lattice-far"))
def test_lattice_ties(name, K):
    """The K-th distance is tied many ways (the mean is still well defined) and points sit at equal distances from cell
    faces: the pruning margins of the query must never drop a candidate that ties.  The translated copy has the same exact
    coordinate differences, hence the same bound."""
    _check(name, K)


@pytest.mark.parametrize("K", (5, 9, 17))
def test_cells_on_both_sides_of_the_fine_grid_threshold(K):
    """Clusters of exactly 16 and exactly 17 points in one coarse cell each (asserted on the host, test_knn_grid_host.py and
    here): the first is searched on the coarse grid, the second on the fine one."""
    xyz, s16, s17 = knn_case.threshold_cloud()
    cnt = knn_case.coarse_cell_counts(xyz)
    assert (cnt[s16] == knn_case.SG_KNN_DENSE).all() and (cnt[s17] == knn_case.SG_KNN_DENSE + 1).all()
    assert np.array_equal(xyz, knn_case.cloud("threshold"))
    _check("threshold", K)


def test_exact_where_the_cell_scan_carries_over_chunks():
    """More than 2^20 fine cells: the scan of the cells' block sums (sg_scan.h) runs its carry loop, and the points that search
    the fine grid sit in cells past the first chunk of 1 024 block sums (asserted on the host, with the product's sizing).
    K = 9 at every one of the 48 000 points against fp64 brute force in chunks of 2 000 rows."""
    from oracle import knn_grid
    from sings_amd.regularizers import knn_mean_edge
    xyz = knn_case.carry_cloud()
    gc, gf = knn_grid.grids_of(xyz)
    assert int(gf["ncells"]) > 2 ** 20
    fine = (knn_case.coarse_cell_counts(xyz) > knn_case.SG_KNN_DENSE) & (knn_grid.cell_ids(gf, xyz) >= 2 ** 20)
    assert int(fine.sum()) >= 500, int(fine.sum())
    dev = _dev()
    got = knn_mean_edge(torch.from_numpy(xyz).to(dev), K=9).cpu().numpy()
    ref = knn_case.brute_force_chunked(xyz, 9)                   # on the CPU, as every reference of this file
    rel = np.abs(got - ref) / ref
    print(f"knn carry cloud K=9: {int(gf['ncells'])} fine cells, {int(fine.sum())} points in fine cells >= 2^20, worst relative "
          f"difference {rel.max():.3e} (fine-grid points {rel[fine].max():.3e})")
    assert got.shape == (48000,) and np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)


PROPERTY_CLOUDS = ("sheet-N1000-flatx-at0.37", "coincident-N300", "lattice-origin")


@pytest.mark.parametrize("name", PROPERTY_CLOUDS)
def test_deterministic_and_permutation_invariant(name):
    from sings_amd.regularizers import knn_mean_edge
    x = knn_case.tensor(name).to(_dev())
    a = knn_mean_edge(x); b = knn_mean_edge(x)
    assert torch.equal(a, b)
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(0)).to(x.device)
    c = knn_mean_edge(x[perm].contiguous())
    assert torch.allclose(c, a[perm], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", PROPERTY_CLOUDS)
def test_edge_loss_value_and_gradient_closed_form(name):
    """loss = mean((s0 - d)^2), dL/ds0 = 2 (s0 - d) / N, other columns zero, in fp64 from the brute-force distances."""
    from sings_amd.regularizers import GaussiansEdgeLoss
    dev = _dev()
    xyz = knn_case.cloud(name)
    N = len(xyz)
    sc_n = np.random.RandomState(5).uniform(0.005, 0.08, (N, 3)).astype(np.float32)
    sc = torch.from_numpy(sc_n).to(dev).requires_grad_(True)
    loss = GaussiansEdgeLoss()({'xyz_canon': knn_case.tensor(name).to(dev), 'scales': sc})
    loss.backward()
    d = knn_case.brute_force(name, 9)
    s0 = sc_n[:, 0].astype(np.float64)
    loss_ref = ((s0 - d) ** 2).mean()
    print(f"edge loss {name}: {loss.item():.9e} vs {loss_ref:.9e}, relative {abs(loss.item() - loss_ref) / loss_ref:.3e}")
    assert abs(loss.item() - loss_ref) <= 3e-6 * abs(loss_ref)
    g_ref = np.zeros((N, 3)); g_ref[:, 0] = 2.0 * (s0 - d) / N
    _close(sc.grad.cpu().numpy(), g_ref)


@pytest.mark.parametrize("N", (362, 1000))
def test_workspace_is_not_overrun(N):
    """Through the C ABI: sg_knn_ws_bytes(N) bytes of workspace followed by a 1 MiB tail of 0xA5.  The square sheets of 362 and
    1 000 points are the sizes at which the fine (362) and the coarse (1 000) grid used to get more cells than the workspace
    holds counters for; the fine grid's arrays are the last of the workspace.  The tail must come back untouched and the
    result must be right.  (1 MiB: a fixed parameter, ten times the largest overrun that sizing could make here.)"""
    from sings_amd import _lib
    from sings_amd._marshal import _ptr, _stream
    dev = _dev()
    lib = _lib.load()
    name = f"sheet-N{N}-flatz-at0"
    x = knn_case.tensor(name).to(dev)
    nbytes, tail = int(lib.sg_knn_ws_bytes(N)), 1 << 20
    buf = torch.full((nbytes + tail,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.sg_gaussian_edge_loss(N, 9, _ptr(x), None, _ptr(buf), _ptr(out), None, None, None, _stream(dev)), "knn")
    torch.cuda.synchronize(dev)
    assert bool((buf[nbytes:] == 0xA5).all()), "the k-NN build wrote past sg_knn_ws_bytes(N)"
    np.testing.assert_allclose(out.cpu().numpy(), knn_case.brute_force(name, 9), rtol=RTOL, atol=ATOL)
