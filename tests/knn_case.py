"""Point clouds on which a uniform-grid k-NN search can go wrong -- flat, thin, colinear, coincident, barely larger than K,
on cell faces, at the coarse / fine threshold -- and the fp64 brute force they are compared with.  No GPU in here: the host
test checks the builders, the GPU test (test_gpu_knn_degenerate.py) runs the kernels on them.  Every cloud is fp32, seeded,
at most 5 000 points, but for carry_cloud's 48 000 (the smallest with more than 2^20 fine cells)."""
import functools

import numpy as np
import torch

from oracle import knn_grid

KMAX = 17
SG_KNN_DENSE = 16                      # sg_knn.hip: a point whose coarse cell holds MORE points searches the fine grid


def sheet(N, flat, const, seed=0):
    """Random points of the unit square, coordinate `flat` (0, 1, 2) constant."""
    rs = np.random.RandomState(1000 * flat + seed + N)
    xyz = rs.uniform(0.0, 1.0, (N, 3)).astype(np.float32)
    xyz[:, flat] = np.float32(const)
    return xyz


def slab(N, rel, seed=0):
    """Body-sized box 0.6 x 1.8 whose third extent is `rel` of the largest."""
    rs = np.random.RandomState(seed + 7)
    return (rs.uniform(0.0, 1.0, (N, 3)) * np.array([0.6, 1.8, 1.8 * rel])).astype(np.float32)


def line(N, direction, seed=0):
    rs = np.random.RandomState(seed + 11)
    d = np.asarray(direction, np.float64)
    return (rs.uniform(0.0, 1.0, (N, 1)) * d[None, :]).astype(np.float32)


def coincident(N, at=(0.25, -1.5, 3.0)):
    return np.tile(np.asarray(at, np.float32), (N, 1))


def two_clusters(n=40):
    a = np.tile(np.array([0.5, 0.5, 0.5], np.float32), (n, 1))
    b = np.tile(np.array([1.5, 0.5, 0.5], np.float32), (n, 1))
    return np.concatenate([a, b])


def tiny(N, seed=0):
    return np.random.RandomState(seed + 100 + N).uniform(-1.0, 1.0, (N, 3)).astype(np.float32)


def lattice(origin=(0.0, 0.0, 0.0), n=16, spacing=2.0 ** -4):
    """n^3 lattice: every coordinate and every coordinate difference is exact in fp32 (also after the translation by
    multiples of 500), the K-th distance is tied many ways."""
    i = np.arange(n, dtype=np.float64) * spacing
    g = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin, np.float64)
    out = g.astype(np.float32)
    assert (out.astype(np.float64) == g).all()
    return out


def threshold_cloud(seed=0):
    """2 000 sparse points of the unit cube plus two clusters of exactly SG_KNN_DENSE and SG_KNN_DENSE + 1 points, each at the
    centre of a coarse cell that holds no sparse point: the first stays on the coarse grid, the second takes the fine one.
    Returns (xyz, slice of the 16, slice of the 17)."""
    rs = np.random.RandomState(seed + 31)
    sparse = rs.uniform(0.0, 1.0, (2000, 3)).astype(np.float32)
    n = 2000 + 2 * SG_KNN_DENSE + 1
    mn, mx = sparse.min(0), sparse.max(0)
    g = knn_grid.size_batch([mn], [mx], [knn_grid.max_cells(n, 0)])[0]
    used = set(knn_grid.cell_ids(g, sparse).tolist())
    dim = g["dim"].astype(np.int64)
    centres = []
    for cz in range(dim[2] // 2, dim[2] - 1):                    # interior cells from the middle on: the first two empty ones
        for cy in range(dim[1] // 2, dim[1] - 1):
            for cx in range(dim[0] // 2, dim[0] - 1):
                if (cz * dim[1] + cy) * dim[0] + cx not in used and len(centres) < 2:
                    centres.append(g["lo"].astype(np.float64) + (np.array([cx, cy, cz]) + 0.5) * float(g["h"]))
    assert len(centres) == 2
    cl = [(c[None, :] + 0.05 * float(g["h"]) * rs.uniform(-1.0, 1.0, (m, 3))).astype(np.float32)
          for c, m in zip(centres, (SG_KNN_DENSE, SG_KNN_DENSE + 1))]
    xyz = np.concatenate([sparse, cl[0], cl[1]])
    assert len(xyz) == n
    return xyz, slice(2000, 2000 + SG_KNN_DENSE), slice(2000 + SG_KNN_DENSE, n)


def coarse_cell_counts(xyz):
    """Per point: how many points share its coarse cell (the grid is sized by the product's function, on the CPU)."""
    gc, _ = knn_grid.grids_of(xyz)
    ids = knn_grid.cell_ids(gc, xyz)
    return np.bincount(ids, minlength=int(gc["ncells"]))[ids]


def carry_cloud():
    """48 000 points whose fine grid has 105^3 = 1 157 625 cells -- 1 131 blocks of 1 024, so the scan of the block sums
    (sg_scan.h) takes a second chunk with a carry -- and whose dense points live in that second chunk: uniform points of the
    unit cube, rows 0-599 replaced by three tight clusters near the top (z = 0.95 .. 0.985).  550 points share a coarse cell
    with more than SG_KNN_DENSE others and search the fine grid, 549 of them cluster points, in fine cells 1 089 217 ..
    1 137 853 (the caller asserts what it relies on).  A wrong carry moves those cells' start offsets."""
    N = 48000
    rs = np.random.RandomState(11)
    xyz = rs.uniform(0.0, 1.0, (N, 3))
    for k, c in enumerate(((0.3, 0.4, 0.97), (0.7, 0.2, 0.985), (0.5, 0.8, 0.95))):
        xyz[200 * k:200 * (k + 1)] = np.array(c) + 0.003 * rs.standard_normal((200, 3))
    return xyz.astype(np.float32)


def brute_force_chunked(xyz, K, rows=2000):
    """brute_force for a cloud too large for one distance matrix: the same fp64 cdist + topk, `rows` rows at a time."""
    x = torch.as_tensor(xyz, dtype=torch.float32).double()
    out = [torch.topk(torch.cdist(x[i:i + rows], x, compute_mode="donot_use_mm_for_euclid_dist"), K, dim=1, largest=False)
           .values[:, 1:].mean(1) for i in range(0, len(x), rows)]
    return torch.cat(out).numpy()


SHEET_N = (9, 64, 362, 1000, 4000)
CLOUDS = {}
for _n in SHEET_N:
    for _f in range(3):
        for _c in (0.0, 0.37):
            CLOUDS[f"sheet-N{_n}-flat{'xyz'[_f]}-at{_c:g}"] = functools.partial(sheet, _n, _f, _c)
for _r in (1e-3, 3e-3):
    CLOUDS[f"slab-{_r:g}"] = functools.partial(slab, 3000, _r)
CLOUDS["line-x"] = functools.partial(line, 500, (1.0, 0.0, 0.0))
CLOUDS["line-z"] = functools.partial(line, 500, (0.0, 0.0, 1.0))
CLOUDS["line-diag"] = functools.partial(line, 500, (0.6, 1.8, 0.3))
for _n in (9, 300, 5000):
    CLOUDS[f"coincident-N{_n}"] = functools.partial(coincident, _n)
CLOUDS["two-clusters"] = two_clusters
for _k in (5, 9, 17):
    CLOUDS[f"tiny-N{_k}"] = functools.partial(tiny, _k)
    CLOUDS[f"tiny-N{_k + 1}"] = functools.partial(tiny, _k + 1)
CLOUDS["lattice-origin"] = lattice
CLOUDS["lattice-far"] = functools.partial(lattice, (1000.0, -2000.0, 500.0))
CLOUDS["threshold"] = lambda: threshold_cloud()[0]


@functools.lru_cache(maxsize=None)
def cloud(name):
    a = np.ascontiguousarray(CLOUDS[name](), np.float32)
    a.setflags(write=False)
    return a


def tensor(name):
    """A fresh fp32 CPU tensor of the cloud (the cached array itself stays read-only)."""
    return torch.tensor(cloud(name), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def nearest(name):
    """[N, min(N, KMAX)] fp64: the sorted distances from every point to its nearest points (itself first), by brute force --
    torch.cdist in double on the fp32 coordinates (differences, not the |x|^2 + |y|^2 - 2xy form, which is inexact), topk.
    Computed once per cloud."""
    x = tensor(name).double()
    d = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist")
    v = torch.topk(d, min(len(x), KMAX), dim=1, largest=False).values.numpy()
    v.setflags(write=False)
    return v


def brute_force(name, K):
    """Mean of the K - 1 distances after the self distance."""
    v = nearest(name)
    assert K <= v.shape[1]
    return v[:, 1:K].mean(1)
