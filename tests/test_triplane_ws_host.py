"""The tri-plane workspace sizes, on the host: ``sg_triplane_ws_bytes`` and ``sg_triplane_bwd_ws_bytes`` are pure host arithmetic
(the library loads without a GPU), and their values are ABI -- callers allocate by them and the backward carves its arrays at the
offsets they imply.  The expected numbers were recorded from a build of commit 247aa7f, the last one before the sort's prefix scan
moved to sg_scan.h: the move must not change a size.

Configurations: the five of tests/test_gpu_decode.py::test_triplane_plane_configurations and the shipped 64 / [1, 2, 4]."""
import ctypes as C

import pytest

from sings_amd import _lib

POINTS = (1, 3001, 150000)
# (resolution, multires): sg_triplane_ws_bytes, sg_triplane_bwd_ws_bytes at the three point counts
RECORDED = [
    (([8, 8, 8], [1]), 49152, (54272, 1421824, 68453376)),
    (([8, 6, 10], [1, 2]), 240640, (268544, 2932224, 133467392)),
    (([16, 12, 20], [1, 2, 4, 8]), 16363520, (41021696, 46277376, 303819776)),
    (([96, 64, 80], [1, 2, 4, 8]), 412221440, (567491072, 572746752, 830289152)),
    (([5, 7, 3], [4, 1]), 309760, (349952, 3013632, 133548800)),
    (([64, 64, 64], [1, 2, 4]), 66060288, (91242752, 95202560, 289241088)),
]


def _planes(res, multires):
    tp = _lib.SgTriplane()
    tp.n_scales, tp.feat = len(multires), 32
    for s, m in enumerate(multires):
        for a in range(3):
            tp.res[s][a] = res[a] * m
    for k in range(3):
        tp.aabb[0][k], tp.aabb[1][k] = -1.0, 1.0
    return tp


@pytest.mark.parametrize("cfg,fwd,bwd", RECORDED, ids=[f"{r}x{m}".replace(" ", "") for (r, m), _, _ in RECORDED])
def test_triplane_workspace_sizes(cfg, fwd, bwd):
    lib = _lib.load()
    tp = _planes(*cfg)
    assert int(lib.sg_triplane_ws_bytes(C.byref(tp))) == fwd
    assert tuple(int(lib.sg_triplane_bwd_ws_bytes(C.byref(tp), n)) for n in POINTS) == bwd
