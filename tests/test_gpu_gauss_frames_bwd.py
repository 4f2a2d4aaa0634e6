"""The K-camera per-Gaussian backward of the raster path (sg_gauss_frame_bwd_kernel + sg_gauss_sum_frames_kernel, reached through
sg_rasterize_backward_gaussians_frames with K > 1) against
 (a) a chain of K single-camera calls into ONE gradient buffer, the first with the caller's ``accumulate`` and the others with
     accumulate = 1 -- bit for bit, signs of zeros included (the project's rule for every K-frame path), with ONE exception that
     the K-camera path has had since it exists: a frame f > 0 that does not see a Gaussian leaves its dL/dsh sums alone, while
     the single-camera call of that frame adds +0 to the row -- so a -0 the earlier frames left there stays -0 in the K-camera
     call and reads +0 after the chain (_same_bits allows exactly this and nothing else), and
 (b) the sum over the frames of the scalar oracle's gradients at the bound of tests/test_gpu_raster.py::_grad_close.

The scene is 777 Gaussians (no multiple of 64 or 256: the last wave is partly live, the last workgroup has a dead wave) of the
synthetic cloud with twenty-one crafted ones in front: colours that are clamped in some frames only, Gaussians seen by frame 0
only, Gaussians that frame 0 does not see, and three that every frame sees with every channel clamped: their dL/dsh of every
frame holds -0, which survives only if frame 0 ASSIGNS.  That the
scene really holds these cases is asserted from the oracle alone in tests/test_gauss_frames_bwd_scenes_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sings_amd.scene import synthetic_scene

P = 777
SEED = 31
ZC = 4.0                           # depth of the crafted Gaussians
FLIP = list(range(0, 6))           # channels 0 and 2 clamped in the frames whose camera has passed them, channel 1 never
ONLY0 = list(range(6, 12))         # visible in frame 0 only (the first three with every channel clamped)
LATER = list(range(12, 18))        # frame 0 does not see them, frame 1 does
MINUS0 = list(range(18, 21))       # seen by frames 0..2, every channel clamped: dRGB = +0, dL/dsh row 1 = (basis < 0) * 0 = -0
STEP = 0.2                         # the camera moves by this much per frame (x)
SH_C0 = 0.28209479177387814

SMALL = (128, 128)                 # 8 x 8 tiles: the few-tile regime (tile counters in LDS, `rec_valid` in use)
RAGGED = (1034, 1030)              # 65 x 65 tiles, ragged right column and bottom row: the many-tile regime (`rec_valid` null)


def scene(D, M, W, H):
    s = synthetic_scene(P, W, H, D, SEED, M=M)
    half = ZC * s["tanfovx"]
    means, shs, sc, op = s["means3D"], s["shs"], s["scales"], s["opacities"]
    crafted = FLIP + ONLY0 + LATER + MINUS0
    sc[crafted] = 0.02; op[crafted] = 0.8
    for j, i in enumerate(FLIP):
        means[i] = (-0.05 - 0.02 * j, 0.1 * (j - 2.5), ZC)
        shs[i] = 0.0
        shs[i, 0] = (-0.5 / SH_C0, 1.0, -0.5 / SH_C0)
        if M > 3:
            shs[i, 3, 0] = 40.0; shs[i, 3, 2] = 40.0         # colour = -C1 * dir.x * 40: its sign is the side the camera is on
    for j, i in enumerate(ONLY0):
        means[i] = (half - 0.03, 0.08 * (j + 1), ZC)
    for j, i in enumerate(MINUS0):
        means[i] = (0.3 + 0.1 * j, 0.3 + 0.1 * j, ZC)
    for i in MINUS0 + ONLY0[:3]:
        shs[i] = 0.0
        shs[i, 0] = -10.0
    for j, i in enumerate(LATER):
        means[i] = (-half - 0.12, -0.08 * (j + 1), ZC)
    return s


def cameras(s, K, closer=None):
    """K cameras STEP apart along x; ``closer``: that frame's camera stands 1.2 nearer (it sees fewer pairs)"""
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], K, 0).copy(); views[:, 3, 0] = STEP * np.arange(K)
    if closer is not None:
        views[closer, 3, 2] = -1.2
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])
    return views.astype(np.float32), projs, cps


@functools.lru_cache(maxsize=None)
def oracle(K, D, M, W, H, colors=False, cov=False, closer=None):
    """(scene, cameras, per-frame oracle forwards, dL [K,3,H,W] zeroed at the oracle's borderline pixels, per-frame oracle
    gradients, precomputed colours / covariances or None).  Host only."""
    from oracle import raster_oracle as ro
    s = scene(D, M, W, H)
    views, projs, cps = cameras(s, K, closer)
    col = np.random.RandomState(5).uniform(0, 1, (P, 3)).astype(np.float32) if colors else None
    cov6 = None
    if cov:
        cov6 = ro.forward(s["means3D"], s["opacities"], views[0], projs[0], cps[0], W, H, s["tanfovx"], s["tanfovy"], s["bg"],
                          scales=s["scales"], rotations=s["rotations"], shs=s["shs"], sh_degree=D)["cov3D"].astype(np.float32)
    dL = np.random.RandomState(12).normal(0, 1, (K, 3, H, W)).astype(np.float32)
    fwd, grads = [], []
    for f in range(K):
        o = ro.forward(s["means3D"], s["opacities"], views[f], projs[f], cps[f], W, H, s["tanfovx"], s["tanfovy"], s["bg"],
                       scales=None if cov else s["scales"], rotations=None if cov else s["rotations"],
                       shs=None if colors else s["shs"], sh_degree=D, colors_precomp=col, cov3D_precomp=cov6)
        dL[f][:, o["margin"] < 2e-5] = 0
        fwd.append(o); grads.append(ro.backward(o, dL[f]))
    return s, (views, projs, cps), fwd, dL, grads, col, cov6


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


class Harness:
    """The K-frame entry points of the C ABI on one configuration: ``run(k, lo, grads, accumulate)`` renders and differentiates
    cameras lo .. lo + k in ONE call into the gradient buffers ``grads``."""

    def __init__(self, K, D, M, W, H, planar=False, colors=False, cov=False, closer=None):
        from sings_amd import _lib
        self.dev = _dev()
        self.lib = _lib.load()
        self.K, self.D, self.M, self.W, self.H, self.planar, self.colors, self.cov = K, D, M, W, H, planar, colors, cov
        self.s, (self.views, self.projs, self.cps), self.fwd, dL, self.grads, col, cov6 = oracle(K, D, M, W, H, colors, cov, closer)
        t = self.t
        self.dL = t(dL)
        self.means, self.op = t(self.s["means3D"]), t(self.s["opacities"])
        self.shs = None if colors else t(self.s["shs"])
        self.col = t(col) if colors else None
        self.scales = None if cov else t(self.s["scales"])
        self.rots = None if cov else t(self.s["rotations"])
        self.cov6 = t(cov6) if cov else None
        self.cap = 48 * P
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def buffers(self, preload):
        """gradient buffers: ``preload`` random non-zero values (the same for every caller), else a constant the kernels must
        overwrite wherever the single-camera chain does"""
        rs = np.random.RandomState(77)
        shape = dict(means=(P, 3), op=(P, 1), sh=(self.M, P, 3) if self.planar else (P, self.M, 3), col=(P, 3), scales=(P, 3),
                     rots=(P, 4), cov=(P, 6))
        return {k: self.t(rs.normal(0, 1, v).astype(np.float32)) if preload else torch.full(v, 7.0, device=self.dev)
                for k, v in shape.items()}

    def run(self, k, lo, grads, accumulate, cap=None):
        from sings_amd import _lib
        from sings_amd._marshal import _frame_batch, _ptr, _settings_struct
        from sings_amd.rasterizer import GaussianRasterizationSettings
        lib, dev, t, W, H = self.lib, self.dev, self.t, self.W, self.H
        cap = self.cap if cap is None else cap
        keep = []
        rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=self.s["tanfovx"], tanfovy=self.s["tanfovy"],
                                           bg=t(self.s["bg"]), scale_modifier=1.0, viewmatrix=t(self.views[lo:lo + k]),
                                           projmatrix=t(self.projs[lo:lo + k]), sh_degree=self.D, campos=t(self.cps[lo:lo + k]),
                                           prefiltered=False, debug=False)
        st = _settings_struct(rs, dev, 0 if self.colors else self.M, keep)
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
        ins = (_ptr(self.means), _ptr(self.shs), _ptr(self.col), _ptr(self.op), _ptr(self.scales), _ptr(self.rots), _ptr(self.cov6))
        _lib.check(lib.sg_rasterize_forward_frames(C.byref(st), C.byref(fb), P, *ins, _ptr(geom), _ptr(binning), cap, _ptr(img),
                                                   _ptr(color), _ptr(radii), nr, self.stream), "fwd")
        _lib.check(lib.sg_rasterize_backward_records_frames(C.byref(st), C.byref(fb), P, _ptr(geom), _ptr(binning), cap, _ptr(img),
                                                            _ptr(bwd), _ptr(self.dL[lo:lo + k].contiguous()), self.stream), "records")
        _lib.check(lib.sg_rasterize_backward_gaussians_frames(
            C.byref(st), C.byref(fb), P, *ins, _ptr(radii), _ptr(geom), _ptr(binning), cap, _ptr(bwd), int(accumulate),
            _ptr(grads["means"]), _ptr(m2), None if self.colors else _ptr(grads["sh"]), _ptr(grads["col"]) if self.colors else None,
            _ptr(grads["op"]), None if self.cov else _ptr(grads["scales"]), None if self.cov else _ptr(grads["rots"]),
            _ptr(grads["cov"]) if self.cov else None, self.stream), "gaussians")
        torch.cuda.synchronize()
        return color, radii, m2, [int(v) for v in nr]

    def chain(self, accumulate, cap=None, skip=()):
        """the K cameras as single-camera calls into one buffer, in frame order"""
        ref = self.buffers(accumulate)
        singles, first = {}, True
        for f in range(self.K):
            if f in skip:
                continue
            singles[f] = self.run(1, f, ref, accumulate or not first, cap)
            first = False
        return ref, singles

    def written(self):
        """the gradient buffers this configuration writes"""
        return ["means", "op"] + (["col"] if self.colors else ["sh"]) + (["cov"] if self.cov else ["scales", "rots"])


def _same_bits(h, got, ref, seen=None):
    """``seen`` [K,P] (bool; None: ``ref`` is no chain of single-camera calls): frame f took the Gaussian's gradient.  The one
    difference allowed (module docstring): a -0 in dL/dsh where the chain holds +0, for a Gaussian some frame f > 0 did not see."""
    for k in h.written():
        a, b = _bits(got[k]), _bits(ref[k])
        if k == "sh" and seen is not None:
            skipped = torch.from_numpy(~np.asarray(seen)[1:].all(0)).to(a.device)
            skipped = skipped[None, :, None] if h.planar else skipped[:, None, None]
            b = torch.where((a == -2 ** 31) & (b == 0) & skipped, a, b)
        assert torch.equal(a, b), (k, int((a != b).sum()))
    for k in got:
        if k not in h.written():
            assert torch.equal(_bits(got[k]), _bits(ref[k])), ("untouched", k)


def _grad_close(name, a, b, rtol=2e-4, atol=2e-6):
    from test_gpu_raster import _grad_close as close
    close(name, np.asarray(a, np.float64).reshape(b.shape), b)


CASES = [
    # K, D, M, (W, H), planar, colours, covariances
    (2, 3, 16, SMALL, False, False, False),
    (3, 3, 16, RAGGED, False, False, False),           # the staged row store; many tiles
    (8, 3, 16, SMALL, False, False, False),
    (3, 2, 16, SMALL, False, False, False),            # M = 16 with D < 3: plain rows, the rows behind (D+1)^2 zeroed
    (8, 1, 16, SMALL, False, False, False),
    (2, 0, 16, SMALL, False, False, False),
    (3, 2, 9, SMALL, False, False, False),             # M = (D+1)^2: the non-vector row path
    (2, 1, 4, RAGGED, False, False, False),
    (3, 0, 1, SMALL, False, False, False),
    (3, 3, 16, SMALL, True, False, False),             # sh_planar
    (2, 1, 16, RAGGED, True, False, False),
    (3, 0, 16, SMALL, False, True, False),             # colors_precomp
    (3, 3, 16, SMALL, False, False, True),             # cov3D_precomp
    (8, 0, 16, SMALL, False, True, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("K,D,M,size,planar,colors,cov", CASES)
def test_k_cameras_leave_the_bits_of_the_single_camera_chain_and_the_oracles_sums(K, D, M, size, planar, colors, cov, accumulate):
    h = Harness(K, D, M, *size, planar, colors, cov)
    ref, singles = h.chain(accumulate)
    got = h.buffers(accumulate)
    color, radii, m2, nr = h.run(K, 0, got, accumulate)
    assert all(0 < r <= h.cap for r in nr), nr
    for f in range(K):
        assert np.array_equal(radii[f].cpu().numpy(), h.fwd[f]["radii"]), f
        assert torch.equal(_bits(color[f]), _bits(singles[f][0][0])) and torch.equal(radii[f], singles[f][1][0]), f
        assert torch.equal(_bits(m2[f]), _bits(singles[f][2][0])), ("d_means2D", f)
    _same_bits(h, got, ref, radii.cpu().numpy() > 0)
    # a second run: the same bits
    again = h.buffers(accumulate)
    _, _, m2b, _ = h.run(K, 0, again, accumulate)
    assert torch.equal(_bits(m2b), _bits(m2))
    _same_bits(h, again, got)
    # (b) the oracle: what the buffer held + the sum of the frames' gradients
    old = {k: v.cpu().numpy().astype(np.float64) for k, v in h.buffers(True).items()} if accumulate else None
    keys = dict(means="dL_dmeans3D", op="dL_dopacity", sh="dL_dsh", col="dL_dcolor", scales="dL_dscales", rots="dL_drots", cov="dL_dcov3D")
    for k in h.written():
        want = sum(g[keys[k]].astype(np.float64) for g in h.grads)
        mine = got[k].cpu().numpy().astype(np.float64)
        if k == "sh":
            if planar:
                mine = mine.transpose(1, 0, 2)
            used = (D + 1) ** 2
            if accumulate or planar:                # rows behind (D+1)^2: left alone
                assert np.array_equal(mine[:, used:], (old["sh"].transpose(1, 0, 2) if planar else old["sh"])[:, used:]
                                      if accumulate else np.full_like(mine[:, used:], 7.0))
            else:
                assert not mine[:, used:].any()
            mine, want = mine[:, :used], want[:, :used]
            if accumulate:
                mine = mine - (old["sh"].transpose(1, 0, 2) if planar else old["sh"])[:, :used]
        elif accumulate:
            mine = mine - old[k]
        # (accumulate: the preloaded values are O(1), the difference carries their rounding: 2^-24 of them)
        _grad_close(f"{k}", mine, want, atol=2e-6) if not accumulate else \
            np.testing.assert_allclose(mine, want, rtol=2e-4, atol=2e-6 * np.abs(want).max() + 4 * 2.0 ** -24 * 4.0)
    for f in range(K):
        _grad_close(f"means2D[{f}]", m2[f].cpu().numpy(), h.grads[f]["dL_dmean2D"])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 3])
def test_a_minus_zero_of_frame_zero_survives_and_a_later_frame_assigns_nothing(K):
    """MINUS0: seen by every frame, every channel clamped -- dRGB = +0, so each frame's dL/dsh is (basis) * 0 and row 1 (basis
    -C1 y with y > 0) is -0.  Frame 0 ASSIGNS (0 + -0 would be +0) and the later frames add -0 to -0: the -0 must be in the buffer,
    as the chain of single-camera calls leaves it.  LATER: frame 0 contributes +0, the first frame that sees them adds to it."""
    h = Harness(K, 3, 16, *SMALL)
    ref, _ = h.chain(0)
    got = h.buffers(0)
    h.run(K, 0, got, 0)
    sh, shr = _bits(got["sh"]).view(P, 16, 3), _bits(ref["sh"]).view(P, 16, 3)
    for i in MINUS0:
        assert (sh[i, 1] == -2 ** 31).all(), (i, sh[i, 1])                     # the bits of -0.0f
        assert (sh[i, 0] == 0).all(), (i, sh[i, 0])                            # basis 0 is positive: +0
        assert torch.equal(sh[i], shr[i]), i
    assert float(got["sh"][LATER].abs().max()) > 0 and float(got["means"][LATER].abs().max()) > 0


@pytest.mark.gpu
def test_frames_that_overflowed_contribute_exactly_zero_and_the_other_is_unchanged():
    """Frame 1's camera stands closer and sees fewer pairs: at a capacity only IT fits in, frames 0 and 2 overflow -- header[1] != 0,
    the composite wrote no records, stale record slots must not be summed -- frame 0, the one that assigns, among them."""
    K, f_fit = 3, 1
    h = Harness(K, 3, 16, *SMALL, closer=f_fit)
    _, _, _, nr = h.run(K, 0, h.buffers(0), 0)
    others = min(r for f, r in enumerate(nr) if f != f_fit)
    assert nr[f_fit] * 1.05 < others, nr
    cap = (others + nr[f_fit]) // 2
    over = tuple(f for f in range(K) if f != f_fit)
    ref, singles = h.chain(0, cap)
    without, _ = h.chain(0, cap, skip=over)
    got = h.buffers(0)
    _, _, m2, nr2 = h.run(K, 0, got, 0, cap)
    assert nr2 == nr
    for f in range(K):
        assert torch.equal(_bits(m2[f]), _bits(singles[f][2][0])), f
        assert (float(m2[f].abs().max()) == 0.0) == (f in over), f
    _same_bits(h, got, ref, np.stack([singles[f][1][0].cpu().numpy() > 0 if f == f_fit else np.zeros(P, bool) for f in range(K)]))
    for k in h.written():
        assert torch.equal(got[k], without[k]), k                              # (values: 0 + x == x)
    assert float(got["means"].abs().max()) > 0
