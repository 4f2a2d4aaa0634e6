"""The K-camera per-Gaussian backward of the raster path as ONE kernel (sg_gauss_frames_bwd_kernel: a workgroup is 64 Gaussians x K
frames, wave f works on frame f, the K gradients of a Gaussian meet in LDS behind one workgroup barrier) at the shapes that
layout can go wrong at, each bit for bit against the chain of K single-camera calls into one gradient buffer (the rule and its one
allowed -0 case: tests/test_gpu_gauss_frames_bwd.py::_same_bits):
 (a) K outside {2, 3, 8}: 5 and 9 (K divides neither the 48 floats of a dL/dsh row nor 64), 16 (1 024 threads, 128 KiB of LDS:
     above the default limit of a kernel's dynamic LDS);
 (b) P = 1, 63, 64, 65, 129 with K = 3: one live lane in the only workgroup, a full workgroup less one, an exactly full one, one
     live lane behind a full workgroup, and the same behind two;
 (c) a BLIND wave: one frame's camera sees none of the 64 Gaussians of workgroup 1 while the other frames see all of them -- that
     wave has no records to sum and nothing to differentiate, and must still arrive at the barrier; once with frame 0 the blind one
     (the frame that would assign), once with the last.  That the scene has this property is asserted from the oracle alone in
     tests/test_gauss_frames_wg_scenes_host.py.
Every case runs 128 x 128 frames (8 x 8 tiles)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_gauss_frames_bwd as gf
from sings_amd.scene import synthetic_scene

W = H = 128
ZC = gf.ZC
FAR = 8.0                          # a camera this far along x sees nothing of what stands around x = 0 at depth ZC
BLIND_P = 192                      # three workgroups of 64
BLIND_BLOCK = slice(64, 128)       # the Gaussians of workgroup 1: an 8 x 8 grid every near camera sees whole
ASIDE = list(range(0, 8)) + list(range(128, 136))      # Gaussians of workgroups 0 and 2 that only the far camera sees


def cameras_at(s, xs):
    """one camera per entry of ``xs``: the scene's camera moved by that much along x (gf.cameras with free offsets)"""
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], len(xs), 0).copy(); views[:, 3, 0] = np.asarray(xs, np.float32)
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])
    return views.astype(np.float32), projs, cps


def head_scene(P, D=3, M=16):
    """the first P Gaussians of the scene of tests/test_gpu_gauss_frames_bwd.py (its crafted ones stand in front)"""
    s = dict(gf.scene(D, M, W, H))
    for k in ("means3D", "shs", "scales", "rotations", "opacities"):
        s[k] = np.ascontiguousarray(s[k][:P])
    if P > len(gf.FLIP + gf.ONLY0 + gf.LATER + gf.MINUS0):                 # the last one too is seen: the edge lane has work
        s["means3D"][P - 1] = (0.2, -0.4, ZC); s["scales"][P - 1] = 0.02; s["opacities"][P - 1] = 0.8
    return s


def blind_scene(blind, K=3):
    """(scene, camera offsets): frame ``blind`` stands FAR along x, the others gf.STEP apart around x = 0"""
    s = synthetic_scene(BLIND_P, W, H, 3, 41, M=16)
    g = np.arange(64)
    s["means3D"][BLIND_BLOCK] = np.stack([0.1 * (g % 8 - 3.5), 0.1 * (g // 8 - 3.5), np.full(64, ZC)], 1)
    for j, i in enumerate(ASIDE):
        s["means3D"][i] = (-FAR + 0.1 * (j - 7.5), 0.1 * (j % 4), ZC)
    crafted = list(range(64, 128)) + ASIDE
    s["scales"][crafted] = 0.02; s["opacities"][crafted] = 0.8
    near = iter(gf.STEP * np.arange(K - 1))
    return s, [FAR if f == blind else float(next(near)) for f in range(K)]


class WgHarness(gf.Harness):
    """gf.Harness for any P and any cameras, without the oracle's gradients (these tests compare bits with the single-camera
    chain): ``chain`` and ``written`` are the parent's."""

    def __init__(self, s, cams, D, M, planar=False, cov=False):
        from sings_amd import _lib
        self.dev = gf._dev()
        self.lib = _lib.load()
        self.s, (self.views, self.projs, self.cps) = s, cams
        self.P, self.K = len(s["means3D"]), len(self.views)
        self.D, self.M, self.W, self.H, self.planar, self.colors, self.cov = D, M, W, H, planar, False, cov
        t = self.t
        self.dL = t(np.random.RandomState(12).normal(0, 1, (self.K, 3, H, W)).astype(np.float32))
        self.means, self.op, self.shs, self.col = t(s["means3D"]), t(s["opacities"]), t(s["shs"]), None
        self.scales = None if cov else t(s["scales"])
        self.rots = None if cov else t(s["rotations"])
        self.cov6 = None
        if cov:
            from oracle import raster_oracle as ro
            self.cov6 = t(ro.forward(s["means3D"], s["opacities"], self.views[0], self.projs[0], self.cps[0], W, H, s["tanfovx"],
                                     s["tanfovy"], s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"],
                                     sh_degree=D)["cov3D"].astype(np.float32))
        self.cap = 48 * self.P + 1024
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def buffers(self, preload):
        P, rs = self.P, np.random.RandomState(77)
        shape = dict(means=(P, 3), op=(P, 1), sh=(self.M, P, 3) if self.planar else (P, self.M, 3), col=(P, 3), scales=(P, 3),
                     rots=(P, 4), cov=(P, 6))
        return {k: self.t(rs.normal(0, 1, v).astype(np.float32)) if preload else torch.full(v, 7.0, device=self.dev)
                for k, v in shape.items()}

    def run(self, k, lo, grads, accumulate, cap=None):
        from sings_amd import _lib
        from sings_amd._marshal import _frame_batch, _ptr, _settings_struct
        from sings_amd.rasterizer import GaussianRasterizationSettings
        lib, dev, t, P = self.lib, self.dev, self.t, self.P
        cap = self.cap if cap is None else cap
        keep = []
        rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=self.s["tanfovx"], tanfovy=self.s["tanfovy"],
                                           bg=t(self.s["bg"]), scale_modifier=1.0, viewmatrix=t(self.views[lo:lo + k]),
                                           projmatrix=t(self.projs[lo:lo + k]), sh_degree=self.D, campos=t(self.cps[lo:lo + k]),
                                           prefiltered=False, debug=False)
        st = _settings_struct(rs, dev, self.M, keep)
        if self.planar:
            st.flags |= _lib.FLAG_SH_PLANAR
        fb = _frame_batch(k, 1, 0)
        L = _lib.SgLayout(); sizes = [C.c_size_t() for _ in range(4)]
        _lib.check(lib.sg_frames_layout(P, W, H, cap, k, C.byref(L), *[C.byref(x) for x in sizes]), "layout")
        u8 = dict(dtype=torch.uint8, device=dev)
        geom, binning, img, bwd = (torch.zeros(x.value, **u8) for x in sizes)
        color = torch.empty((k, 3, H, W), device=dev); radii = torch.empty((k, P), dtype=torch.int32, device=dev)
        m2 = torch.full((k, P, 3), 5.0, device=dev)
        nr = (C.c_int64 * k)()
        ins = (_ptr(self.means), _ptr(self.shs), None, _ptr(self.op), _ptr(self.scales), _ptr(self.rots), _ptr(self.cov6))
        _lib.check(lib.sg_rasterize_forward_frames(C.byref(st), C.byref(fb), P, *ins, _ptr(geom), _ptr(binning), cap, _ptr(img),
                                                   _ptr(color), _ptr(radii), nr, self.stream), "fwd")
        _lib.check(lib.sg_rasterize_backward_records_frames(C.byref(st), C.byref(fb), P, _ptr(geom), _ptr(binning), cap, _ptr(img),
                                                            _ptr(bwd), _ptr(self.dL[lo:lo + k].contiguous()), self.stream), "records")
        _lib.check(lib.sg_rasterize_backward_gaussians_frames(
            C.byref(st), C.byref(fb), P, *ins, _ptr(radii), _ptr(geom), _ptr(binning), cap, _ptr(bwd), int(accumulate),
            _ptr(grads["means"]), _ptr(m2), _ptr(grads["sh"]), None, _ptr(grads["op"]),
            None if self.cov else _ptr(grads["scales"]), None if self.cov else _ptr(grads["rots"]),
            _ptr(grads["cov"]) if self.cov else None, self.stream), "gaussians")
        torch.cuda.synchronize()
        return color, radii, m2, [int(v) for v in nr]


def _check(h, accumulate):
    """the K-camera call against the chain: frames, radii, per-view statistic and every gradient buffer; -> (radii, gradients)"""
    ref, singles = h.chain(accumulate)
    got = h.buffers(accumulate)
    color, radii, m2, nr = h.run(h.K, 0, got, accumulate)
    assert all(r <= h.cap for r in nr), nr
    for f in range(h.K):
        assert torch.equal(gf._bits(color[f]), gf._bits(singles[f][0][0])) and torch.equal(radii[f], singles[f][1][0]), f
        assert torch.equal(gf._bits(m2[f]), gf._bits(singles[f][2][0])), ("d_means2D", f)
    gf._same_bits(h, got, ref, radii.cpu().numpy() > 0)
    return radii.cpu().numpy(), got


K_CASES = [
    # K, D, planar, covariances
    (5, 3, False, False),
    (9, 3, False, False),
    (16, 3, False, False),
    (5, 1, False, False),
    (9, 3, True, False),
    (16, 3, False, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("K,D,planar,cov", K_CASES)
def test_frame_counts_outside_the_old_set_leave_the_chains_bits(K, D, planar, cov, accumulate):
    s = gf.scene(D, 16, W, H)
    h = WgHarness(s, gf.cameras(s, K), D, 16, planar, cov)
    radii, got = _check(h, accumulate)
    n = (radii > 0).sum(0)
    assert (n == K).any() and ((n > 0) & (n < K)).any() and (radii > 0).any(1).all()      # mixed visibility, no empty frame
    if not accumulate:
        assert float(got["sh"].abs().max()) > 0 and float(got["means"].abs().max()) > 0
        if not planar:
            assert not got["sh"][:, (D + 1) ** 2:].any()                                  # rows behind (D+1)^2: zeroed


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_gaussian_counts_at_the_workgroups_edges_leave_the_chains_bits(P, accumulate):
    s = head_scene(P)
    h = WgHarness(s, gf.cameras(s, 3), 3, 16)
    radii, got = _check(h, accumulate)
    assert (radii[:, P - 1] > 0).any() and (radii[:, 0] > 0).any()                        # the edge lanes carry a gradient
    if not accumulate:
        assert float(got["means"][P - 1].abs().max()) > 0 and float(got["sh"][P - 1].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("blind", [0, 2])
def test_a_wave_whose_frame_sees_none_of_its_gaussians_still_meets_the_others(blind, accumulate):
    s, xs = blind_scene(blind)
    h = WgHarness(s, cameras_at(s, xs), 3, 16)
    radii, got = _check(h, accumulate)
    seen = radii[:, BLIND_BLOCK] > 0
    assert not seen[blind].any() and np.delete(seen, blind, 0).all()
    assert (radii[blind] > 0).any()                                                       # (the blind frame is no empty frame)
    if not accumulate:
        assert float(got["sh"][BLIND_BLOCK].abs().max()) > 0 and float(got["means"][BLIND_BLOCK].abs().max()) > 0
