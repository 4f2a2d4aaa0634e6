"""The K-camera forward head of the raster path in work order (sg_gauss_frames_fwd_kernel: a workgroup is 64 Gaussians x K frames,
wave f projects frame f from inputs the workgroup staged once in LDS and reserves its record slots with one atomic per wave;
sg_bin_ordered_kernel then gathers rectangle and depth bits from one line of the 64-byte record), each K-camera forward bit for bit
against the chain of K single-camera forwards of the same cameras: colour, radii, final_T, n_contrib, R and the overflow word,
ranges, point_list and the keys of every tile's row, then the gradients of a following backward (the rule and its one allowed -0
case: tests/test_gpu_gauss_frames_bwd.py::_same_bits).

The kernel is selected for K > 1 with a work order on a frame that is binned directly and has more than 4 096 tile counters, so
every case runs on the ragged 1034 x 1030 frame (65 x 65 tiles) of tests/test_gpu_work_order.py; the same cases also run at
128 x 128 (8 x 8 tiles), and one at the ragged 200 x 136, where the dispatch must leave the launch with the kernels it had (the
few-tile path).  Cases:
 (a) K = 2, 5, 8, 9, 16 at D = 3; one each of D = 0, D = 1, colors_precomp, cov3D_precomp, planar dL/dsh;
 (b) P = 1, 63, 64, 65, 129 at K = 3: one live lane, a workgroup less one, an exactly full one, one live lane behind one and two;
 (c) a workgroup whose 64 Gaussians one frame's camera sees none of (frame 0, then the last frame): that wave takes no slots;
 (d) a frame that sees nothing at all;
 (e) a pair capacity too small for ONE frame of the launch: it renders the background, the others are what they were;
 (f) without an order (the unordered launch), identity, reversed and random orders, and an order with entries >= P, which is held
     to the chain of single-camera ORDERED forwards (those Gaussians are binned by neither);
 (g) two runs: the same bits.
That the scenes hold these cases is asserted from the oracle alone in tests/test_gauss_frames_fwd_scenes_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_gauss_frames_bwd as gf
from sings_amd.scene import synthetic_scene

SMALL = (128, 128)                 # 8 x 8 tiles: few tiles, the launch keeps sg_preprocess_fwd_kernel
RAGGED_SMALL = (200, 136)          # 13 x 9 tiles, ragged right column and bottom row: few tiles too
MANY = (1034, 1030)                # 65 x 65 tiles, 4 624 counter words: the many-tile regime, where the new kernel runs
SIZES = [SMALL, MANY]
ZC = gf.ZC
KEY_PITCH = 1024                   # SG_TILE_KEY_PITCH: keys between the rows of a directly binned many-tile frame
FAR = 8.0                          # a camera this far along x sees nothing of what stands around x = 0 at depth ZC
NOWHERE = 60.0                     # ... and this far: nothing of the whole cloud
BLIND_P = 192                      # three workgroups of 64
BLIND_BLOCK = slice(64, 128)       # the Gaussians of workgroup 1: an 8 x 8 grid every near camera sees whole
ASIDE = list(range(0, 8)) + list(range(128, 136))      # Gaussians of workgroups 0 and 2 that only the far camera sees


# ---- scenes (numpy only: the host test reads them too) ---------------------------------------------------------------------------
def cameras_at(s, xs, closer=()):
    """one camera per entry of ``xs``: the scene's camera moved by that much along x; frames in ``closer`` stand 1.2 nearer"""
    P_T = np.linalg.inv(s["viewmatrix"]) @ s["projmatrix"]
    views = np.repeat(s["viewmatrix"][None], len(xs), 0).copy(); views[:, 3, 0] = np.asarray(xs, np.float32)
    for f in closer:
        views[f, 3, 2] = -1.2
    projs = np.stack([(v @ P_T).astype(np.float32) for v in views])
    cps = np.stack([np.linalg.inv(v)[3, :3].astype(np.float32) for v in views])
    return views.astype(np.float32), projs, cps


def head_scene(P, size):
    """the first P Gaussians of the scene of tests/test_gpu_gauss_frames_bwd.py (its crafted ones stand in front)"""
    s = dict(gf.scene(3, 16, *size))
    for k in ("means3D", "shs", "scales", "rotations", "opacities"):
        s[k] = np.ascontiguousarray(s[k][:P])
    if P > len(gf.FLIP + gf.ONLY0 + gf.LATER + gf.MINUS0):                 # the last one too is seen: the edge lane has work
        s["means3D"][P - 1] = (0.2, -0.4, ZC); s["scales"][P - 1] = 0.02; s["opacities"][P - 1] = 0.8
    return s


def blind_scene(blind, size, K=3):
    """(scene, camera offsets): frame ``blind`` stands FAR along x, the others gf.STEP apart around x = 0"""
    s = synthetic_scene(BLIND_P, *size, 3, 41, M=16)
    g = np.arange(64)
    s["means3D"][BLIND_BLOCK] = np.stack([0.1 * (g % 8 - 3.5), 0.1 * (g // 8 - 3.5), np.full(64, ZC)], 1)
    for j, i in enumerate(ASIDE):
        s["means3D"][i] = (-FAR + 0.1 * (j - 7.5), 0.1 * (j % 4), ZC)
    crafted = list(range(64, 128)) + ASIDE
    s["scales"][crafted] = 0.02; s["opacities"][crafted] = 0.8
    near = iter(gf.STEP * np.arange(K - 1))
    return s, [FAR if f == blind else float(next(near)) for f in range(K)]


EMPTY_XS = [0.0, NOWHERE, gf.STEP]                                         # frame 1 sees nothing at all
DROPPED = (gf.MINUS0[0], gf.MINUS0[1])                                     # what the order `beyond` does not list
OVER_K, OVER_FRAME = 3, 1                                                  # frames 0 and 2 stand closer and see fewer pairs


def over_cameras(s):
    return cameras_at(s, gf.STEP * np.arange(OVER_K), closer=[f for f in range(OVER_K) if f != OVER_FRAME])


def orders(P):
    """name -> order [P] (int32) or None.  ``beyond``: a permutation whose entries for the Gaussians DROPPED (two crafted ones
    that frames 0 .. 2 see) are replaced by values >= P"""
    ident = np.arange(P, dtype=np.int32)
    beyond = np.random.RandomState(4).permutation(P).astype(np.int32)
    if P > max(DROPPED):
        beyond[beyond == DROPPED[0]] = P + 7; beyond[beyond == DROPPED[1]] = -1
    return {"none": None, "identity": ident, "reversed": ident[::-1].copy(),
            "random": np.random.RandomState(12).permutation(P).astype(np.int32), "beyond": beyond}


# ---- the C ABI on one configuration ----------------------------------------------------------------------------------------------
class Harness:
    """``run(k, lo, grads, accumulate, order)``: cameras lo .. lo + k rendered and differentiated in ONE call each of the K-frame
    entry points, on fresh zeroed workspaces -> everything a caller sees and what the forward left in its workspaces."""

    def __init__(self, s, cams, size, D=3, M=16, planar=False, colors=False, cov=False):
        from sings_amd import _lib
        self.dev = gf._dev()
        self.lib = _lib.load()
        self.s, (self.views, self.projs, self.cps) = s, cams
        self.P, self.K = len(s["means3D"]), len(self.views)
        (self.W, self.H), self.D, self.M, self.planar, self.colors, self.cov = size, D, M, planar, colors, cov
        self.T = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        self.many = (((self.W + 15) // 16 + 3) // 4) * (((self.H + 15) // 16 + 3) // 4) * 16 > _lib.HIST_TILES_MAX
        t = self.t
        self.dL = t(np.random.RandomState(12).normal(0, 1, (self.K, 3, self.H, self.W)).astype(np.float32))
        self.means, self.op = t(s["means3D"]), t(s["opacities"])
        self.shs = None if colors else t(s["shs"])
        self.col = t(np.random.RandomState(5).uniform(0, 1, (self.P, 3)).astype(np.float32)) if colors else None
        self.scales = None if cov else t(s["scales"])
        self.rots = None if cov else t(s["rotations"])
        self.cov6 = None
        if cov:
            from oracle import raster_oracle as ro
            self.cov6 = t(ro.forward(s["means3D"], s["opacities"], self.views[0], self.projs[0], self.cps[0], 64, 64, s["tanfovx"],
                                     s["tanfovy"], s["bg"], scales=s["scales"], rotations=s["rotations"], shs=s["shs"],
                                     sh_degree=D)["cov3D"].astype(np.float32))
        self.cap = 48 * self.P + 1024
        self.stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def buffers(self, preload):
        P, rs = self.P, np.random.RandomState(77)
        shape = dict(means=(P, 3), op=(P, 1), sh=(self.M, P, 3) if self.planar else (P, self.M, 3), col=(P, 3), scales=(P, 3),
                     rots=(P, 4), cov=(P, 6))
        return {k: self.t(rs.normal(0, 1, v).astype(np.float32)) if preload else torch.full(v, 7.0, device=self.dev)
                for k, v in shape.items()}

    def written(self):
        return ["means", "op"] + (["col"] if self.colors else ["sh"]) + (["cov"] if self.cov else ["scales", "rots"])

    def run(self, k, lo, grads, accumulate, order=None, cap=None):
        from sings_amd import _lib
        from sings_amd._marshal import _frame_batch, _ptr, _settings_struct
        from sings_amd.rasterizer import GaussianRasterizationSettings
        lib, dev, t, P, W, H, T = self.lib, self.dev, self.t, self.P, self.W, self.H, self.T
        cap = self.cap if cap is None else cap
        keep = []
        rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=self.s["tanfovx"], tanfovy=self.s["tanfovy"],
                                           bg=t(self.s["bg"]), scale_modifier=1.0, viewmatrix=t(self.views[lo:lo + k]),
                                           projmatrix=t(self.projs[lo:lo + k]), sh_degree=self.D, campos=t(self.cps[lo:lo + k]),
                                           prefiltered=False, debug=False)
        st = _settings_struct(rs, dev, 0 if self.colors else self.M, keep)
        st.flags |= _lib.FLAG_SHORT_LISTS | (_lib.FLAG_SH_PLANAR if self.planar else 0)
        fb = _frame_batch(k, 1, 0)
        L = _lib.SgLayout(); sizes = [C.c_size_t() for _ in range(4)]
        _lib.check(lib.sg_frames_layout(P, W, H, cap, k, C.byref(L), *[C.byref(x) for x in sizes]), "layout")
        u8 = dict(dtype=torch.uint8, device=dev)
        geom, binning, img, bwd = (torch.zeros(x.value, **u8) for x in sizes)
        color = torch.empty((k, 3, H, W), device=dev); radii = torch.empty((k, P), dtype=torch.int32, device=dev)
        m2 = torch.full((k, P, 3), 5.0, device=dev)
        nr = (C.c_int64 * k)()
        ins = (_ptr(self.means), _ptr(self.shs), _ptr(self.col), _ptr(self.op), _ptr(self.scales), _ptr(self.rots), _ptr(self.cov6))
        args = (C.byref(st), C.byref(fb), P, *ins, _ptr(geom), _ptr(binning), cap, _ptr(img), _ptr(color), _ptr(radii), nr)
        if order is None:
            _lib.check(lib.sg_rasterize_forward_frames(*args, self.stream), "fwd")
        else:
            od = t(order)
            _lib.check(lib.sg_rasterize_forward_frames_ordered(*args, _ptr(od), P, self.stream), "fwd (ordered)")
        torch.cuda.synchronize()
        nr = [int(v) for v in nr]
        out = dict(color=color, radii=radii, nr=nr, frames=[])
        bw, iw = binning.view(k, L.bin_bytes), img.view(k, L.img_bytes)
        for f in range(k):
            d = dict(header=bw[f, L.bin_header:L.bin_header + 8].view(torch.int32).clone())
            if 0 <= nr[f] <= cap:                                         # (a refused frame has no lists and no image state)
                d["final_T"] = iw[f, L.img_final_T:L.img_final_T + 4 * H * W].view(torch.int32).clone()
                d["n_contrib"] = iw[f, L.img_n_contrib:L.img_n_contrib + 4 * H * W].view(torch.int32).clone()
                rg = bw[f, L.bin_ranges:L.bin_ranges + 8 * T].view(torch.int32).view(T, 2).clone()
                d["ranges"] = rg
                d["point_list"] = bw[f, L.bin_point_list:L.bin_point_list + 4 * nr[f]].view(torch.int32).clone()
                if self.many:
                    # the keys of tile t: the first (end - start) entries of row t, at whatever ranks their counting atomics returned
                    rows = bw[f, L.bin_tile_keys:L.bin_tile_keys + 8 * T * KEY_PITCH].view(torch.int64).view(T, -1).clone()
                    n = (rg[:, 1] - rg[:, 0]).to(torch.int64)
                    rows[torch.arange(rows.shape[1], device=dev)[None, :] >= n[:, None]] = torch.iinfo(torch.int64).max
                    d["keys"] = rows.sort(1).values
            out["frames"].append(d)
        _lib.check(lib.sg_rasterize_backward_records_frames(C.byref(st), C.byref(fb), P, _ptr(geom), _ptr(binning), cap, _ptr(img),
                                                            _ptr(bwd), _ptr(self.dL[lo:lo + k].contiguous()), self.stream), "records")
        _lib.check(lib.sg_rasterize_backward_gaussians_frames(
            C.byref(st), C.byref(fb), P, *ins, _ptr(radii), _ptr(geom), _ptr(binning), cap, _ptr(bwd), int(accumulate),
            _ptr(grads["means"]), _ptr(m2), None if self.colors else _ptr(grads["sh"]), _ptr(grads["col"]) if self.colors else None,
            _ptr(grads["op"]), None if self.cov else _ptr(grads["scales"]), None if self.cov else _ptr(grads["rots"]),
            _ptr(grads["cov"]) if self.cov else None, self.stream), "gaussians")
        torch.cuda.synchronize()
        out["m2"] = m2
        return out

    def chain(self, accumulate, order=None, cap=None):
        """the K cameras as single-camera calls into one gradient buffer, in frame order"""
        ref = self.buffers(accumulate)
        return ref, [self.run(1, f, ref, accumulate or f > 0, order, cap) for f in range(self.K)]


def _same_frame(a, fa, b, fb, what):
    """frame ``fa`` of run ``a`` against frame ``fb`` of run ``b``: every forward array, bit for bit"""
    assert a["nr"][fa] == b["nr"][fb], (what, a["nr"], b["nr"])
    for k in ("color", "radii", "m2"):
        assert torch.equal(gf._bits(a[k][fa]), gf._bits(b[k][fb])), (what, k)
    da, db = a["frames"][fa], b["frames"][fb]
    assert set(da) == set(db), (what, sorted(da), sorted(db))
    for k in da:
        assert torch.equal(da[k], db[k]), (what, k)


def _check(h, accumulate=0, order="identity", cap=None, ref_order=None):
    """the K-camera call against the chain, then a second run against the first; -> (the run, its gradient buffers)"""
    od = orders(h.P)[order]
    ref, singles = h.chain(accumulate, ref_order, cap)
    got = h.buffers(accumulate)
    out = h.run(h.K, 0, got, accumulate, od, cap)
    cap = h.cap if cap is None else cap
    for f in range(h.K):
        _same_frame(out, f, singles[f], 0, (order, f))
    seen = (out["radii"].cpu().numpy() > 0) & (np.asarray(out["nr"]) <= cap)[:, None]
    gf._same_bits(h, got, ref, seen)
    again = h.buffers(accumulate)
    out2 = h.run(h.K, 0, again, accumulate, od, cap)
    for f in range(h.K):
        _same_frame(out2, f, out, f, (order, f, "second run"))
    gf._same_bits(h, again, got)
    return out, got


def _mixed(out, K):
    """every frame sees something, some Gaussians are seen by all frames and some by a few"""
    seen = out["radii"].cpu().numpy() > 0
    n = seen.sum(0)
    return bool(seen.any(1).all() and (n == K).any() and ((n > 0) & (n < K)).any())


K_CASES = [
    # K, D, M, planar, colours, covariances
    (2, 3, 16, False, False, False),
    (5, 3, 16, False, False, False),
    (8, 3, 16, False, False, False),
    (9, 3, 16, False, False, False),
    (16, 3, 16, False, False, False),
    (3, 0, 16, False, False, False),                   # rows of 16 coefficients, one in use: the float path of the fill
    (3, 0, 1, False, False, False),                    # M = (D+1)^2 = 1: 3-float rows, 16-byte vectors and a tail
    (5, 1, 4, False, False, False),                    # M = (D+1)^2 = 4
    (3, 0, 16, False, True, False),                    # colors_precomp
    (3, 3, 16, False, False, True),                    # cov3D_precomp
    (3, 3, 16, True, False, False),                    # planar dL/dsh
]


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,M,planar,colors,cov,size", [c + (z,) for c in K_CASES for z in SIZES] + [K_CASES[2] + (RAGGED_SMALL,)])
def test_k_cameras_leave_the_bits_of_the_single_camera_chain(K, D, M, planar, colors, cov, size):
    s = gf.scene(D, M, *size)
    h = Harness(s, cameras_at(s, gf.STEP * np.arange(K)), size, D, M, planar, colors, cov)
    out, got = _check(h)
    assert _mixed(out, K) and all(0 < r <= h.cap for r in out["nr"])
    assert float(got["means"].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_accumulating_backward_behind_the_k_camera_forward(size):
    s = gf.scene(3, 16, *size)
    _check(Harness(s, cameras_at(s, gf.STEP * np.arange(3)), size), accumulate=1)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_gaussian_counts_at_the_workgroups_edges(P, size):
    s = head_scene(P, size)
    out, got = _check(Harness(s, cameras_at(s, gf.STEP * np.arange(3)), size))
    radii = out["radii"].cpu().numpy()
    assert (radii[:, P - 1] > 0).any() and (radii[:, 0] > 0).any()                        # the edge lanes have pairs
    assert float(got["means"][P - 1].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("blind", [0, 2])
def test_a_wave_whose_frame_sees_none_of_its_gaussians_takes_no_slots(blind, size):
    s, xs = blind_scene(blind, size)
    out, _ = _check(Harness(s, cameras_at(s, xs), size))
    seen = out["radii"].cpu().numpy()[:, BLIND_BLOCK] > 0
    assert not seen[blind].any() and np.delete(seen, blind, 0).all()
    assert out["nr"][blind] > 0                                                           # (the blind frame is no empty frame)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_a_frame_that_sees_nothing_at_all(size):
    s = gf.scene(3, 16, *size)
    h = Harness(s, cameras_at(s, EMPTY_XS), size)
    out, _ = _check(h)
    assert out["nr"][1] == 0 and not bool(out["radii"][1].any()) and out["nr"][0] > 0 and out["nr"][2] > 0
    bg = h.t(s["bg"])[:, None, None].expand(3, h.H, h.W)
    assert torch.equal(out["color"][1], bg)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_a_capacity_too_small_for_one_frame_leaves_the_others_alone(size):
    s = gf.scene(3, 16, *size)
    h = Harness(s, over_cameras(s), size)
    full = h.run(OVER_K, 0, h.buffers(0), 0, orders(h.P)["identity"])
    nr = full["nr"]
    most = max(r for f, r in enumerate(nr) if f != OVER_FRAME)
    assert most * 1.05 < nr[OVER_FRAME], nr
    cap = (most + nr[OVER_FRAME]) // 2
    out, got = _check(h, cap=cap)
    assert out["nr"] == nr
    bg = h.t(s["bg"])[:, None, None].expand(3, h.H, h.W)
    for f in range(OVER_K):
        over = f == OVER_FRAME
        assert int(out["frames"][f]["header"][1] != 0) == int(over), f                   # the overflow word
        assert torch.equal(out["color"][f], bg) == over, f
        assert (float(out["m2"][f].abs().max()) == 0.0) == over, f
        if not over:                                                                      # ... as with room for every frame
            _same_frame(out, f, full, f, ("capacity", f))
    assert float(got["means"].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("order", ["none", "reversed", "random", "beyond"])
def test_with_and_without_a_work_order(order, size):
    s = gf.scene(3, 16, *size)
    h = Harness(s, cameras_at(s, gf.STEP * np.arange(4)), size)
    # an entry >= P idles its lane in the single-camera ordered launch too: that chain is the reference
    out, _ = _check(h, order=order, ref_order=orders(h.P)[order] if order == "beyond" else None)
    assert all(r > 0 for r in out["nr"])
    if order == "beyond" and h.many:                                                      # seen, and in no list (R: the filed pairs)
        full = h.run(h.K, 0, h.buffers(0), 0)
        dropped = torch.tensor(DROPPED, dtype=torch.int32, device=h.dev)
        for f in range(3):
            d = out["frames"][f]
            assert bool((out["radii"][f, list(DROPPED)] > 0).all()), f
            assert out["nr"][f] < full["nr"][f] and int((d["ranges"][:, 1] - d["ranges"][:, 0]).sum()) == out["nr"][f], f
            assert not bool(torch.isin(d["point_list"], dropped).any()), f
            assert bool(torch.isin(dropped, full["frames"][f]["point_list"]).all()), f
