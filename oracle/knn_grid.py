"""TEST INFRASTRUCTURE: ctypes front-end of oracle/libsgknngrid.so -- the product's own k-NN grid sizing
(sings_amd/csrc/sg_knn_grid.h) compiled for the CPU, so that the host tests run the function the kernel runs and not a
copy of it.  `previous=True` selects the loop that function replaced (kept in oracle/knn_grid_host.c for comparison)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
GRID_DTYPE = np.dtype([("lo", np.float32, 3), ("inv_h", np.float32), ("h", np.float32), ("dim", np.int32, 3),
                       ("ncells", np.int32)])           # struct SgGrid


def build(force=False):
    so = os.path.join(_HERE, "libsgknngrid.so")
    srcs = [os.path.join(_HERE, "knn_grid_host.c"), os.path.join(_HERE, "..", "sings_amd", "csrc", "sg_knn_grid.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", _HERE, "-B", "libsgknngrid.so"], stdout=subprocess.DEVNULL)
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.sgk_max_cells.restype = C.c_int
    return _LIB


def max_cells(N, fine):
    return int(lib().sgk_max_cells(C.c_int(int(N)), C.c_int(int(bool(fine)))))


def size_batch(mn, mx, mc, previous=False):
    """mn, mx [n, 3] fp32, mc [n] int -> structured array [n] of SgGrid."""
    mn = np.ascontiguousarray(mn, np.float32).reshape(-1, 3); mx = np.ascontiguousarray(mx, np.float32).reshape(-1, 3)
    mc = np.ascontiguousarray(mc, np.int32).reshape(-1)
    assert len(mn) == len(mx) == len(mc)
    out = np.zeros(len(mn), GRID_DTYPE)
    assert out.itemsize == 36
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib().sgk_size_batch(C.c_int(int(previous)), C.c_int(len(mn)), p(mn), p(mx), p(mc), p(out))
    return out


def grids_of(xyz, previous=False):
    """(coarse, fine) SgGrid records of a cloud [N, 3] fp32, as sg_gaussian_edge_prepare sizes them."""
    xyz = np.asarray(xyz, np.float32)
    mn, mx = xyz.min(0), xyz.max(0)
    g = size_batch([mn, mn], [mx, mx], [max_cells(len(xyz), 0), max_cells(len(xyz), 1)], previous)
    return g[0], g[1]


def cell_ids(g, xyz):
    """Flat cell index of every point (sg_cell_of in sg_knn.hip, restated in fp32)."""
    xyz = np.asarray(xyz, np.float32)
    c = ((xyz - g["lo"]) * g["inv_h"]).astype(np.float32)
    c = np.minimum(np.maximum(c.astype(np.int64), 0), g["dim"].astype(np.int64) - 1)
    return (c[:, 2] * int(g["dim"][1]) + c[:, 1]) * int(g["dim"][0]) + c[:, 0]
